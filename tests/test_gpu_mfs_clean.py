"""
GPU tests of the joint multi-term minor cycle (`cip_mfs_clean`, through
`ska_sdp_cip_amd.mfs`).

The operator's rounding is part of its definition (include/cip_mfs.h), so every
case asserts equality of BITS with the numpy statement `_mfs_np.mfs_clean`:
residuals, models, component indices and fluxes, `niter_done`, `stop_reason`,
`peak` and `peak_index`. No tolerances.

Images are seeded standard-normal noise with a few planted spikes, a different
draw per Taylor term; PSF plane k is 0.5^k exp(-r^2 / 8) cos((0.7 + 0.1 k) r);
hinv is a seeded symmetric positive-definite matrix whose off-diagonals are
not zero, so the cross terms count. `cip_hogbom_clean` runs the T = 1 kernels,
so the shape and selection cases take T = 1 too, with a hinv that is not 1.0.
"""

import ctypes

import numpy as np
import pytest

import _clean_np
import _mfs_np
from ska_sdp_cip_amd import _lib, deconvolve, mfs

pytestmark = pytest.mark.gpu


def _t(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _hinv(nterms, seed=11):
    a = np.random.default_rng(seed).standard_normal((nterms, nterms))
    h = a @ a.T / nterms + np.eye(nterms)
    assert nterms == 1 or np.abs(h[~np.eye(nterms, dtype=bool)]).min() > 0.05
    return h


def _psfs(nterms, px, py, centre=None):
    cx, cy = (px // 2, py // 2) if centre is None else centre
    r = np.hypot(np.arange(px)[:, None] - cx, np.arange(py)[None, :] - cy)
    return np.stack([0.5 ** k * np.exp(-r * r / 8.0) * np.cos((0.7 + 0.1 * k) * r) for k in range(2 * nterms - 1)])


def _images(nterms, nx, ny, seed=3, spikes=True):
    img = np.random.default_rng(seed).standard_normal((nterms, nx, ny))
    if spikes:  # corners and centre: the PSF window clips on every side
        for n, (i, j) in enumerate(((0, 0), (nx - 1, ny - 1), (0, ny - 1), (nx // 2, ny // 2))):
            for t in range(nterms):
                img[t, i, j] = (9.0 - n) * (-1.0) ** (n + t) / (1 + t)
    return img


def _same(a, b):
    """Equal bits (NaNs in the same places; no -0 / +0 confusion)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


def _same_info(info, ref_info):
    got = {k: info[k] for k in ("niter_done", "stop_reason", "peak_index")}
    assert got == {k: ref_info[k] for k in got}
    assert _same(np.float64(info["peak"]), np.float64(ref_info["peak"]))
    assert _same(info["comp_index"].cpu().numpy(), ref_info["comp_index"])
    assert _same(info["comp_flux"].cpu().numpy(), ref_info["comp_flux"])


def _check(img, psf, hinv, ref=None, **kw):
    """One device run against the numpy reference; returns the reference."""
    ref_kw = {k: v for k, v in kw.items() if k != "batch"}
    if ref is None:
        ref = _mfs_np.mfs_clean(img, psf, hinv, **ref_kw)
    ref_model, ref_res, ref_info = ref
    dev_kw = dict(kw)
    for name in ("mask", "model"):
        if dev_kw.get(name) is not None:
            dev_kw[name] = _t(dev_kw[name])
    res_in = _t(img)
    model, res, info = mfs.device_mfs_clean(res_in, _t(psf), hinv, return_components=True, **dev_kw)
    assert _same(res_in.cpu().numpy(), np.asarray(img, dtype=np.float64))  # inplace=False leaves the input alone
    _same_info(info, ref_info)
    assert _same(res.cpu().numpy(), ref_res)
    assert _same(model.cpu().numpy(), ref_model)
    return ref


def _first_record_low(info, candidates):
    """The first k of `candidates` whose peak |s| lies below every earlier peak's, so that a threshold of
    exactly that |s| is first met at k (with cross terms the peaks do not fall monotonically). The term-0
    flux of component k is gain * s_k, which orders the peaks."""
    s0 = np.abs(info["comp_flux"][:, 0])
    return next(k for k in candidates if s0[k] < s0[:k].min())


# ------------------------------------------------------- T = 1 is Hogbom ----
def test_one_term_identity_equals_hogbom():
    # both entry points run the same T = 1 kernels: this guards the two wrappers
    # (the Hogbom cases of test_gpu_clean.py against _clean_np are the check of the kernels)
    img, psf = _images(1, 70, 45), _psfs(1, 33, 21)
    h_model, h_res, h_info = deconvolve.device_hogbom_clean(_t(img[0]), _t(psf[0]), gain=0.2, niter=60,
                                                            return_components=True)
    model, res, info = mfs.device_mfs_clean(_t(img), _t(psf), np.ones((1, 1)), gain=0.2, niter=60,
                                            return_components=True)
    assert info["niter_done"] == 60
    assert _same(res[0].cpu().numpy(), h_res.cpu().numpy()) and _same(model[0].cpu().numpy(), h_model.cpu().numpy())
    assert _same(info["comp_index"].cpu().numpy(), h_info["comp_index"].cpu().numpy())
    assert _same(info["comp_flux"][:, 0].cpu().numpy(), h_info["comp_flux"].cpu().numpy())
    for key in ("niter_done", "stop_reason", "peak_index"):
        assert info[key] == h_info[key]
    assert _same(np.float64(info["peak"]), np.float64(h_info["peak"]))


# ---------------------------------------------------------------- shapes ----
@pytest.mark.parametrize("nterms", [1, 2, 3])
@pytest.mark.parametrize("pshape", [(33, 21), (70, 45), (140, 90)], ids=["patch", "equal", "covers"])
def test_odd_image_against_psf_sizes(nterms, pshape):
    ref = _check(_images(nterms, 70, 45), _psfs(nterms, *pshape), _hinv(nterms), gain=0.2, niter=60)
    assert ref[2]["niter_done"] == 60 and ref[2]["stop_reason"] == _mfs_np.NITER


@pytest.mark.parametrize("nterms", [1, 2, 3])
@pytest.mark.parametrize("ny", [300, 301], ids=["even-16B", "odd-8B"])
def test_both_tile_edges_and_both_access_widths(nterms, ny):
    # 100 x 300: 4 x 3 tiles of 32 x 128 pixels, partial on both axes; the odd width takes the 8-byte path
    ref = _check(_images(nterms, 100, ny, seed=6), _psfs(nterms, 65, 150), _hinv(nterms), gain=0.2, niter=50)
    assert ref[2]["niter_done"] == 50


@pytest.mark.parametrize("nterms", [1, 2, 3])
def test_base_misaligned_to_16_bytes(nterms):
    import torch

    img, psf, hinv = _images(nterms, 100, 300, seed=6), _psfs(nterms, 65, 150), _hinv(nterms)
    ref_model, ref_res, ref_info = _mfs_np.mfs_clean(img, psf, hinv, gain=0.2, niter=50)
    storage = torch.zeros(img.size + 1, dtype=torch.float64, device="cuda")
    view = storage[1:].view(img.shape)  # starts one double into its storage
    view.copy_(_t(img))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    model, res, info = mfs.device_mfs_clean(view, _t(psf), hinv, gain=0.2, niter=50, inplace=True,
                                            return_components=True)
    assert res is view and storage[0].item() == 0.0
    _same_info(info, ref_info)
    assert _same(res.cpu().numpy(), ref_res) and _same(model.cpu().numpy(), ref_model)


@pytest.mark.parametrize("nterms", [1, 2, 3])
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1)])
def test_degenerate_images(nterms, shape):
    img = np.random.default_rng(5).standard_normal((nterms, *shape))
    _check(img, _psfs(nterms, 5, 7), _hinv(nterms), gain=0.3, niter=25)
    _check(img, _psfs(nterms, 2 * shape[0], 2 * shape[1]), _hinv(nterms), gain=0.3, niter=25)


@pytest.mark.parametrize("nterms", [1, 2, 3])
@pytest.mark.parametrize("centre", [(0, 0), (5, 20)])
def test_psf_centre_off_the_middle(nterms, centre):
    _check(_images(nterms, 70, 45), _psfs(nterms, 33, 21, centre), _hinv(nterms), gain=0.2, niter=40,
           psf_centre=centre)


def test_full_cover_psf_2048():
    # 64 x 16 = 1024 tiles, every one inside every window; separable PSF planes (cheap to make)
    rng = np.random.default_rng(21)
    img = rng.standard_normal((2, 2048, 2048))
    for i, j in rng.integers(0, 2048, size=(12, 2)):
        img[0, i, j] += 40.0
        img[1, i, j] -= 13.0
    d = np.arange(4096) - 2048.0
    psf = np.stack([0.5 ** k * np.outer(np.exp(-d * d / 8.0) * np.cos((0.7 + 0.1 * k) * d),
                                        np.exp(-d * d / 8.0) * np.cos(0.6 * d)) for k in range(3)])
    ref = _check(img, psf, _hinv(2), gain=0.25, niter=6)
    assert ref[2]["niter_done"] == 6


def test_more_tiles_than_one_select_round():
    # 1 x 1,100,000: 8594 tiles of 128 columns, more than the 8192 entries the
    # select workgroup loads per round; the largest values sit in the last tiles
    n = 1_100_000
    img = np.random.default_rng(13).standard_normal((2, 1, n))
    hinv = _hinv(2)
    for col, v in ((n - 1, 90.0), (n - 700, -80.0), (8192 * 128 + 5, 70.0), (3, 60.0)):
        img[:, 0, col] = v, 0.25 * v
    ref = _check(img, _psfs(2, 3, 301), hinv, gain=0.5, niter=8)
    assert ref[2]["comp_index"][:3].tolist() == [n - 1, n - 700, 8192 * 128 + 5]


# ------------------------------------------------------------- selection ----
@pytest.mark.parametrize("nterms", [1, 2, 3])
def test_mask_excludes_the_global_peak(nterms):
    img, hinv = _images(nterms, 70, 45), _hinv(nterms)
    mask = (np.random.default_rng(2).random((70, 45)) < 0.5).astype(np.uint8)
    assert _mfs_np.mfs_clean(img, _psfs(nterms, 33, 21), hinv, niter=0)[2]["peak_index"] == 0  # the largest spike
    mask[0, 0] = 0
    img[:, 1, 1], mask[1, 1] = 0.95 * img[:, 0, 0], 1  # the first component, with (0, 0) in its window
    ref = _check(img, _psfs(nterms, 33, 21), hinv, gain=0.2, niter=30, mask=mask)
    assert ref[2]["comp_index"][0] == 1 * 45 + 1 and 0 not in ref[2]["comp_index"] and ref[2]["niter_done"] == 30
    assert (ref[1][:, 0, 0] != img[:, 0, 0]).all()  # not selectable, still subtracted from, in every term


def test_all_zero_mask_is_empty():
    img = _images(2, 70, 45)
    ref = _check(img, _psfs(2, 33, 21), _hinv(2), niter=10, mask=np.zeros((70, 45), dtype=np.uint8))
    assert ref[2]["stop_reason"] == _mfs_np.EMPTY and ref[2]["peak_index"] == -1 and ref[2]["niter_done"] == 0
    assert _same(ref[1], img)


@pytest.mark.parametrize("nterms", [1, 2, 3])
def test_nan_in_one_plane_only_is_never_chosen(nterms):
    img, hinv, psf = _images(nterms, 70, 45), _hinv(nterms), _psfs(nterms, 9, 9)
    would_be = _mfs_np.mfs_clean(img, psf, hinv, niter=0)[2]["peak_index"]
    img.reshape(nterms, -1)[nterms - 1, would_be] = np.nan  # the last term only
    ref = _check(img, psf, hinv, gain=0.2, niter=50)
    assert would_be not in ref[2]["comp_index"].tolist() and ref[2]["niter_done"] == 50
    assert np.isnan(ref[1]).sum() == 1  # the NaN stays where it was, in its plane
    _check(np.full((nterms, 70, 45), np.nan), psf, hinv, niter=5)  # nothing to select: EMPTY


@pytest.mark.parametrize("nterms", [1, 2, 3])
def test_equal_maxima_take_the_lower_index(nterms):
    img, hinv = _images(nterms, 70, 45, spikes=False), _hinv(nterms)
    for t in range(nterms):  # the same T values at three pixels: the same s, far above the noise
        img[t, 60, 7] = img[t, 12, 40] = img[t, 12, 41] = 60.0 / (1 + t)
    ref = _check(img, _psfs(nterms, 33, 21), hinv, gain=0.2, niter=3)
    assert ref[2]["comp_index"][0] == 12 * 45 + 40


# -------------------------------------------------------------- stopping ----
def test_niter_zero_reports_the_peak():
    img, hinv = _images(2, 70, 45), _hinv(2)
    ref = _check(img, _psfs(2, 33, 21), hinv, niter=0)
    assert ref[2]["stop_reason"] == _mfs_np.NITER and ref[2]["niter_done"] == 0 and _same(ref[1], img)
    i, j = divmod(ref[2]["peak_index"], 45)
    assert ref[2]["peak"] == hinv[0, 0] * img[0, i, j] + hinv[0, 1] * img[1, i, j]  # the signed s, not r_0


@pytest.mark.parametrize("nterms", [1, 2, 3])
def test_threshold_hit_exactly(nterms):
    img, psf, hinv = _images(nterms, 70, 45), _psfs(nterms, 33, 21), _hinv(nterms)
    k = _first_record_low(_mfs_np.mfs_clean(img, psf, hinv, gain=0.2, niter=40)[2], range(10, 40))
    _, _, at_k = _mfs_np.mfs_clean(img, psf, hinv, gain=0.2, niter=k)
    ref = _check(img, psf, hinv, gain=0.2, niter=100, threshold=abs(at_k["peak"]))
    assert ref[2]["stop_reason"] == _mfs_np.THRESHOLD and ref[2]["niter_done"] == k  # stops there: <=
    assert abs(ref[2]["peak"]) == abs(at_k["peak"])


def test_all_zero_image():
    ref = _check(np.zeros((2, 70, 45)), _psfs(2, 33, 21), _hinv(2), niter=10)
    assert ref[2]["stop_reason"] == _mfs_np.THRESHOLD and ref[2]["peak_index"] == 0 and ref[2]["niter_done"] == 0


# ------------------------------------------------------- batch invariance ----
@pytest.fixture(scope="module")
def big():
    """(2, 200, 300) (7 x 3 tiles, partial on both axes) with 65 x 129 PSF
    patches, 120 iterations; the reference is computed once."""
    img, psf, hinv = _images(2, 200, 300, seed=8), _psfs(2, 65, 129), _hinv(2)
    kw = dict(gain=0.15, niter=120)
    return img, psf, hinv, kw, _mfs_np.mfs_clean(img, psf, hinv, **kw)


@pytest.mark.parametrize("batch", [1, 7, 0])
def test_batch_invariance(big, batch):
    img, psf, hinv, kw, ref = big
    assert ref[2]["niter_done"] == 120
    _check(img, psf, hinv, ref=ref, batch=batch, **kw)


@pytest.mark.parametrize("batch", [1, 7, 0])
def test_batch_invariance_threshold_mid_batch(big, batch):
    # stop after k components, k strictly inside a batch of 7 (42..49) and of the default
    img, psf, hinv, kw, ref = big
    k = _first_record_low(ref[2], range(43, 49))
    _, _, at = _mfs_np.mfs_clean(img, psf, hinv, gain=kw["gain"], niter=k)
    got = _check(img, psf, hinv, batch=batch, gain=kw["gain"], niter=120, threshold=abs(at["peak"]))
    assert got[2]["stop_reason"] == _mfs_np.THRESHOLD and got[2]["niter_done"] == k


# ----------------------------------------------------------------- state ----
def test_second_call_continues_the_first():
    img, psf, hinv = _images(2, 70, 45), _psfs(2, 33, 21), _hinv(2)
    ref_model, ref_res, ref_info = _mfs_np.mfs_clean(img, psf, hinv, gain=0.2, niter=50)
    m1, r1, i1 = mfs.device_mfs_clean(_t(img), _t(psf), hinv, gain=0.2, niter=20, return_components=True)
    m2, r2, i2 = mfs.device_mfs_clean(r1, _t(psf), hinv, gain=0.2, niter=30, model=m1, inplace=True,
                                      return_components=True)
    assert m2 is m1 and r2 is r1
    assert _same(r2.cpu().numpy(), ref_res) and _same(m2.cpu().numpy(), ref_model)
    assert (i1["niter_done"], i2["niter_done"]) == (20, 30) and i2["comp_flux"].shape == (30, 2)
    assert _same(np.concatenate([i1["comp_flux"].cpu().numpy(), i2["comp_flux"].cpu().numpy()]), ref_info["comp_flux"])
    assert _same(np.concatenate([i1["comp_index"].cpu().numpy(), i2["comp_index"].cpu().numpy()]),
                 ref_info["comp_index"])
    assert i2["peak_index"] == ref_info["peak_index"] and i2["peak"] == ref_info["peak"]


def test_prefilled_model_is_accumulated_into():
    img, psf, hinv = _images(3, 70, 45), _psfs(3, 33, 21), _hinv(3)
    model0 = np.random.default_rng(9).standard_normal((3, 70, 45))
    ref = _check(img, psf, hinv, gain=0.2, niter=30, model=model0)
    zero = _check(img, psf, hinv, gain=0.2, niter=30)
    assert _same(ref[1], zero[1]) and not _same(ref[0], zero[0])


def test_alternating_with_hogbom_through_one_workspace_and_release():
    import torch

    a = (_images(2, 70, 45), _psfs(2, 33, 21), _hinv(2), dict(gain=0.2, niter=25))
    b = (_images(3, 300, 260, seed=4), _psfs(3, 64, 300), _hinv(3), dict(gain=0.2, niter=25))
    refs = [_mfs_np.mfs_clean(c[0], c[1], c[2], **c[3]) for c in (a, b)]
    h_img, h_psf = _images(1, 130, 200, seed=7)[0], _psfs(1, 41, 41)[0]
    h_ref = _clean_np.hogbom_clean(h_img, h_psf, gain=0.2, niter=25)

    def hogbom():
        model, res, info = deconvolve.device_hogbom_clean(_t(h_img), _t(h_psf), gain=0.2, niter=25,
                                                          return_components=True)
        assert _same(res.cpu().numpy(), h_ref[1]) and _same(model.cpu().numpy(), h_ref[0])
        assert _same(info["comp_index"].cpu().numpy(), h_ref[2]["comp_index"])

    for case, ref in ((a, refs[0]), (b, refs[1]), (a, refs[0])):
        _check(case[0], case[1], case[2], ref=ref, **case[3])
        hogbom()
    torch.cuda.synchronize()
    assert _lib.lib().cip_release_workspace() == 0
    _check(b[0], b[1], b[2], ref=refs[1], **b[3])
    hogbom()
    _check(a[0], a[1], a[2], ref=refs[0], **a[3])


def test_non_default_stream():
    import torch

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _check(_images(2, 70, 45), _psfs(2, 140, 90), _hinv(2), gain=0.2, niter=40)
    stream.synchronize()


def test_host_entry_point_numpy_and_torch():
    img, psf, hinv = _images(2, 70, 45), _psfs(2, 33, 21), _hinv(2)
    ref_model, ref_res, ref_info = _mfs_np.mfs_clean(img, psf, hinv, gain=0.2, niter=20)
    model, res, info = mfs.mfs_clean(img, psf, hinv, gain=0.2, niter=20, return_components=True)
    assert isinstance(model, np.ndarray) and _same(model, ref_model) and _same(res, ref_res)
    assert _same(info["comp_index"], ref_info["comp_index"]) and _same(info["comp_flux"], ref_info["comp_flux"])
    t_img = _t(img)
    model, res, info = mfs.mfs_clean(t_img, _t(psf), hinv, gain=0.2, niter=20)
    assert model.is_cuda and _same(res.cpu().numpy(), ref_res) and _same(t_img.cpu().numpy(), img)


# ------------------------------------------------------------ validation ----
def test_invalid_arguments_raise_and_leave_the_residual_alone():
    import torch

    img, psf, hinv = _images(2, 70, 45), _psfs(2, 33, 21), _hinv(2)
    res, p = _t(img), _t(psf)
    nan_hinv = hinv.copy()
    nan_hinv[1, 0] = np.nan
    bad = [dict(hinv=nan_hinv), dict(hinv=np.array([[1.0, np.inf], [0.0, 1.0]])), dict(hinv=np.ones((3, 3))),
           dict(gain=0.0), dict(gain=float("nan")), dict(threshold=-1.0), dict(niter=-1), dict(batch=-1),
           dict(psf_centre=(33, 0)), dict(psf_centre=(-2, 0))]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(ValueError):
            mfs.device_mfs_clean(res, p, kw.pop("hinv", hinv), inplace=True, **kw)
        assert _same(res.cpu().numpy(), img), kw
    # the C ABI itself: nterms outside 1 .. 3, one component array without the other
    so = _lib.lib()
    comp = torch.zeros(16, dtype=torch.int64, device="cuda")
    out = _lib.CleanResult()
    h9 = np.ascontiguousarray(np.eye(4)[:3, :3] + 0.1)  # finite whatever nterms says

    def call(nterms=2, ci=None, cf=None, h=h9):
        return so.cip_mfs_clean(res.data_ptr(), nterms, 70, 45, p.data_ptr(), 33, 21, -1, -1,
                                h.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, 0.1, 0.0, 4, 0, None, None,
                                ci, cf, out)

    for kw in (dict(nterms=0), dict(nterms=4), dict(ci=comp.data_ptr()), dict(cf=comp.data_ptr()),
               dict(h=np.full((3, 3), np.nan))):
        assert call(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_mfs_clean" in so.cip_last_error()
        assert _same(res.cpu().numpy(), img), kw
    assert call(h=np.ascontiguousarray(hinv)) == 0 and out.niter_done == 4
    assert not _same(res.cpu().numpy(), img)
    # tensors of the wrong kind never reach the library
    with pytest.raises(ValueError):
        mfs.device_mfs_clean(res.float(), p, hinv)
    with pytest.raises(ValueError):
        mfs.device_mfs_clean(_t(img), p[:2], hinv)  # 2 PSFs for 2 terms
    with pytest.raises(ValueError):
        mfs.device_mfs_clean(_t(img), p, hinv, mask=torch.ones((45, 70), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        mfs.device_mfs_clean(_t(img), p.cpu(), hinv)
