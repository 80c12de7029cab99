"""
GPU tests of the multiscale minor cycle (`cip_ms_clean`, through
`ska_sdp_cip_amd.multiscale`).

The operator's rounding is part of its definition (include/cip_ms.h), so every
case asserts equality of BITS with the numpy statement `_ms_np.ms_clean`:
residuals, models, component indices, scales and fluxes, `niter_done`,
`stop_reason`, `peak`, `peak_index` and `peak_scale`. No tolerances.

The recipes are those of test_gpu_mfs_clean.py: images are seeded
standard-normal noise with a few planted spikes, a different draw per scale
plane; cross PSF plane k is 0.5^k exp(-r^2 / 8) cos((0.7 + 0.1 k) r); the two
host arrays are seeded and not 1, so that selection (select_weight) and flux
(flux_scale) differ from the plain residual.
"""

import ctypes

import numpy as np
import pytest

import _clean_np
import _ms_np
from ska_sdp_cip_amd import _lib, deconvolve, multiscale

pytestmark = pytest.mark.gpu


def _t(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _weights(nscales, seed=11):
    """(select_weight, flux_scale): seeded, positive, none of them 1, no two alike."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.6, 1.4, nscales), rng.uniform(0.8, 2.5, nscales)


def _psfs(nscales, px, py, centre=None):
    cx, cy = (px // 2, py // 2) if centre is None else centre
    r = np.hypot(np.arange(px)[:, None] - cx, np.arange(py)[None, :] - cy)
    return np.stack([0.5 ** k * np.exp(-r * r / 8.0) * np.cos((0.7 + 0.1 * k) * r)
                     for k in range(nscales * (nscales + 1) // 2)])


def _images(nscales, nx, ny, seed=3, spikes=True):
    img = np.random.default_rng(seed).standard_normal((nscales, nx, ny))
    if spikes:  # corners and centre: the PSF window clips on every side
        for n, (i, j) in enumerate(((0, 0), (nx - 1, ny - 1), (0, ny - 1), (nx // 2, ny // 2))):
            for s in range(nscales):
                img[s, i, j] = (9.0 - n) * (-1.0) ** (n + s) / (1 + s)
    return img


def _same(a, b):
    """Equal bits (NaNs in the same places; no -0 / +0 confusion)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


def _same_info(info, ref_info):
    got = {k: info[k] for k in ("niter_done", "stop_reason", "peak_index", "peak_scale")}
    assert got == {k: ref_info[k] for k in got}
    assert _same(np.float64(info["peak"]), np.float64(ref_info["peak"]))
    for key in ("comp_index", "comp_scale", "comp_flux"):
        assert _same(info[key].cpu().numpy(), ref_info[key]), key


def _check(img, psf, weights, ref=None, **kw):
    """One device run against the numpy reference; returns the reference."""
    ref_kw = {k: v for k, v in kw.items() if k != "batch"}
    if ref is None:
        ref = _ms_np.ms_clean(img, psf, *weights, **ref_kw)
    ref_model, ref_res, ref_info = ref
    dev_kw = dict(kw)
    for name in ("mask", "model"):
        if dev_kw.get(name) is not None:
            dev_kw[name] = _t(dev_kw[name])
    res_in = _t(img)
    model, res, info = multiscale.device_ms_clean(res_in, _t(psf), *weights, return_components=True, **dev_kw)
    assert _same(res_in.cpu().numpy(), np.asarray(img, dtype=np.float64))  # inplace=False leaves the input alone
    _same_info(info, ref_info)
    assert _same(res.cpu().numpy(), ref_res)
    assert _same(model.cpu().numpy(), ref_model)
    return ref


def _first_record_low(info, weights, candidates):
    """The first k of `candidates` whose peak |v| lies below every earlier peak's, so that a threshold of
    exactly that |v| is first met at k. |v_k| = select_weight[s] |flux_k| / (gain flux_scale[s]) up to
    rounding, which orders the peaks well enough to pick k; the threshold itself comes from a run to k."""
    s = info["comp_scale"]
    v = np.abs(info["comp_flux"]) * weights[0][s] / weights[1][s]
    return next(k for k in candidates if v[k] < 0.999 * v[:k].min())


# ------------------------------------------------------- S = 1 is Hogbom ----
def test_one_scale_identity_equals_hogbom():
    img, psf = _images(1, 70, 45), _psfs(1, 33, 21)
    h_model, h_res, h_info = deconvolve.device_hogbom_clean(_t(img[0]), _t(psf[0]), gain=0.2, niter=60,
                                                            return_components=True)
    model, res, info = multiscale.device_ms_clean(_t(img), _t(psf), np.ones(1), np.ones(1), gain=0.2, niter=60,
                                                  return_components=True)
    assert info["niter_done"] == 60 and info["peak_scale"] == 0
    assert _same(res[0].cpu().numpy(), h_res.cpu().numpy()) and _same(model[0].cpu().numpy(), h_model.cpu().numpy())
    assert _same(info["comp_index"].cpu().numpy(), h_info["comp_index"].cpu().numpy())
    assert _same(info["comp_flux"].cpu().numpy(), h_info["comp_flux"].cpu().numpy())
    assert int(info["comp_scale"].abs().max()) == 0
    for key in ("niter_done", "stop_reason", "peak_index"):
        assert info[key] == h_info[key]
    assert _same(np.float64(info["peak"]), np.float64(h_info["peak"]))


# ---------------------------------------------------------------- shapes ----
@pytest.mark.parametrize("nscales", [1, 3, 6])
@pytest.mark.parametrize("shape", [(70, 45), (64, 130), (33, 300)], ids=["scalar", "vector-tile-edge", "wide"])
def test_image_shapes(nscales, shape):
    # 70 x 45: odd width, the 8-byte path; 64 x 130: 16-byte accesses across the 128-column tile edge
    ref = _check(_images(nscales, *shape), _psfs(nscales, 33, 21), _weights(nscales), gain=0.2, niter=40)
    assert ref[2]["niter_done"] == 40 and ref[2]["stop_reason"] == _ms_np.NITER
    if nscales > 1:
        assert len(set(ref[2]["comp_scale"].tolist())) > 1  # components of more than one scale


@pytest.mark.parametrize("nscales", [1, 3, 6])
def test_psf_larger_than_the_image(nscales):
    _check(_images(nscales, 70, 45), _psfs(nscales, 140, 90), _weights(nscales), gain=0.2, niter=30)


@pytest.mark.parametrize("nscales", [1, 3, 6])
@pytest.mark.parametrize("centre", [(0, 0), (5, 20)])
def test_psf_centre_off_the_middle(nscales, centre):
    _check(_images(nscales, 70, 45), _psfs(nscales, 33, 21, centre), _weights(nscales), gain=0.2, niter=30,
           psf_centre=centre)


def test_base_misaligned_to_16_bytes():
    import torch

    img, psf, weights = _images(3, 64, 130, seed=6), _psfs(3, 33, 21), _weights(3)
    ref_model, ref_res, ref_info = _ms_np.ms_clean(img, psf, *weights, gain=0.2, niter=40)
    storage = torch.zeros(img.size + 1, dtype=torch.float64, device="cuda")
    view = storage[1:].view(img.shape)  # starts one double into its storage
    view.copy_(_t(img))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    model, res, info = multiscale.device_ms_clean(view, _t(psf), *weights, gain=0.2, niter=40, inplace=True,
                                                  return_components=True)
    assert res is view and storage[0].item() == 0.0
    _same_info(info, ref_info)
    assert _same(res.cpu().numpy(), ref_res) and _same(model.cpu().numpy(), ref_model)


# ------------------------------------------------------------- selection ----
@pytest.mark.parametrize("nscales", [1, 3, 6])
def test_mask_and_incoming_model(nscales):
    img, weights = _images(nscales, 70, 45), _weights(nscales)
    rng = np.random.default_rng(2)
    mask = (rng.random((70, 45)) < 0.5).astype(np.uint8)
    mask[0, 0] = 0  # the largest spike of every plane
    model0 = rng.standard_normal((nscales, 70, 45))
    ref = _check(img, _psfs(nscales, 33, 21), weights, gain=0.2, niter=30, mask=mask, model=model0)
    assert 0 not in ref[2]["comp_index"].tolist() and ref[2]["niter_done"] == 30
    assert (mask.ravel()[ref[2]["comp_index"]] == 1).all()
    zero = _check(img, _psfs(nscales, 33, 21), weights, gain=0.2, niter=30, mask=mask)
    assert _same(ref[1], zero[1]) and not _same(ref[0], zero[0])


def test_all_zero_mask_is_empty():
    img = _images(3, 70, 45)
    ref = _check(img, _psfs(3, 33, 21), _weights(3), niter=10, mask=np.zeros((70, 45), dtype=np.uint8))
    assert ref[2]["stop_reason"] == _ms_np.EMPTY and ref[2]["niter_done"] == 0
    assert (ref[2]["peak_index"], ref[2]["peak_scale"], ref[2]["peak"]) == (-1, -1, 0.0)
    assert _same(ref[1], img)
    _check(np.full((3, 70, 45), np.nan), _psfs(3, 9, 9), _weights(3), niter=5)  # nothing to select: EMPTY


@pytest.mark.parametrize("nscales", [1, 3, 6])
def test_nan_pixel_is_never_chosen(nscales):
    img, weights, psf = _images(nscales, 70, 45), _weights(nscales), _psfs(nscales, 9, 9)
    probe = _ms_np.ms_clean(img, psf, *weights, niter=0)[2]
    img[probe["peak_scale"]].reshape(-1)[probe["peak_index"]] = np.nan  # the would-be first component
    ref = _check(img, psf, weights, gain=0.2, niter=40)
    taken = set(zip(ref[2]["comp_scale"].tolist(), ref[2]["comp_index"].tolist()))
    assert (probe["peak_scale"], probe["peak_index"]) not in taken and ref[2]["niter_done"] == 40
    assert np.isnan(ref[1]).sum() == 1  # the NaN stays where it was, in its plane


def test_equal_maxima_in_two_planes_take_the_lower_scale():
    img, psf = _images(3, 70, 45, spikes=False), _psfs(3, 33, 21)
    weights = (np.array([0.5, 2.0, 1.0]), np.array([1.5, 0.7, 1.1]))
    # |v| = 0.5 * 64 = 2.0 * 16 = 32 exactly, at a LATER pixel of the lower scale
    img[1, 12, 40], img[0, 60, 7] = 16.0, -64.0
    ref = _check(img, psf, weights, gain=0.2, niter=3)
    assert (ref[2]["comp_scale"][0], ref[2]["comp_index"][0]) == (0, 60 * 45 + 7)
    probe = _ms_np.ms_clean(img, psf, *weights, niter=0)[2]
    assert probe["peak"] == -32.0 and probe["peak_scale"] == 0


def test_equal_maxima_in_one_plane_take_the_lower_index():
    img, psf, weights = _images(3, 70, 45, spikes=False), _psfs(3, 33, 21), _weights(3)
    img[2, 60, 7] = img[2, 12, 40] = img[2, 12, 41] = 60.0
    ref = _check(img, psf, weights, gain=0.2, niter=3)
    assert (ref[2]["comp_scale"][0], ref[2]["comp_index"][0]) == (2, 12 * 45 + 40)


# -------------------------------------------------------------- stopping ----
def test_niter_zero_reports_the_peak():
    img, weights = _images(3, 70, 45), _weights(3)
    ref = _check(img, _psfs(3, 33, 21), weights, niter=0)
    assert ref[2]["stop_reason"] == _ms_np.NITER and ref[2]["niter_done"] == 0 and _same(ref[1], img)
    s, (i, j) = ref[2]["peak_scale"], divmod(ref[2]["peak_index"], 45)
    assert ref[2]["peak"] == weights[0][s] * img[s, i, j]  # the signed v, not r


def test_all_zero_image():
    ref = _check(np.zeros((3, 70, 45)), _psfs(3, 33, 21), _weights(3), niter=10)
    assert ref[2]["stop_reason"] == _ms_np.THRESHOLD and ref[2]["niter_done"] == 0
    assert (ref[2]["peak_index"], ref[2]["peak_scale"]) == (0, 0)


# ------------------------------------------------------- batch invariance ----
@pytest.fixture(scope="module")
def big():
    """(3, 100, 300) (4 x 3 tiles, partial on both axes) with 65 x 129 PSF
    patches, 100 iterations; the reference is computed once."""
    img, psf, weights = _images(3, 100, 300, seed=8), _psfs(3, 65, 129), _weights(3)
    kw = dict(gain=0.15, niter=100)
    return img, psf, weights, kw, _ms_np.ms_clean(img, psf, *weights, **kw)


@pytest.mark.parametrize("batch", [1, 7, 0])
def test_batch_invariance(big, batch):
    img, psf, weights, kw, ref = big
    assert ref[2]["niter_done"] == 100
    _check(img, psf, weights, ref=ref, batch=batch, **kw)


@pytest.mark.parametrize("batch", [1, 7, 0])
def test_batch_invariance_threshold_mid_batch(big, batch):
    # stop after k components, k strictly inside the first batch of 7 (0..7) and of the default. The
    # synthetic cross PSFs are no Gram matrix (plane tri(s, s) is weaker than plane tri(0, s)), so the peaks
    # of this run fall only over its first iterations: that is where a threshold can be met for the first time
    img, psf, weights, kw, ref = big
    k = _first_record_low(ref[2], weights, range(3, 7))
    _, _, at = _ms_np.ms_clean(img, psf, *weights, gain=kw["gain"], niter=k)
    got = _check(img, psf, weights, batch=batch, gain=kw["gain"], niter=100, threshold=abs(at["peak"]))
    assert got[2]["stop_reason"] == _ms_np.THRESHOLD and got[2]["niter_done"] == k


def test_two_calls_give_the_same_bits():
    img, psf, weights = _t(_images(6, 64, 130)), _t(_psfs(6, 33, 21)), _weights(6)
    a = multiscale.device_ms_clean(img, psf, *weights, gain=0.2, niter=40, return_components=True)
    b = multiscale.device_ms_clean(img, psf, *weights, gain=0.2, niter=40, return_components=True)
    assert _same(a[0].cpu().numpy(), b[0].cpu().numpy()) and _same(a[1].cpu().numpy(), b[1].cpu().numpy())
    for key in ("comp_index", "comp_scale", "comp_flux"):
        assert _same(a[2][key].cpu().numpy(), b[2][key].cpu().numpy())


# ----------------------------------------------------------------- state ----
def test_alternating_shapes_through_one_workspace_and_release():
    import torch

    a = (_images(3, 70, 45), _psfs(3, 33, 21), _weights(3), dict(gain=0.2, niter=25))
    b = (_images(6, 130, 260, seed=4), _psfs(6, 64, 150), _weights(6), dict(gain=0.2, niter=25))
    refs = [_ms_np.ms_clean(c[0], c[1], *c[2], **c[3]) for c in (a, b)]
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


def test_host_entry_point_numpy_and_torch():
    img, psf, weights = _images(3, 70, 45), _psfs(3, 33, 21), _weights(3)
    ref_model, ref_res, ref_info = _ms_np.ms_clean(img, psf, *weights, gain=0.2, niter=20)
    model, res, info = multiscale.ms_clean(img, psf, *weights, gain=0.2, niter=20, return_components=True)
    assert isinstance(model, np.ndarray) and _same(model, ref_model) and _same(res, ref_res)
    for key in ("comp_index", "comp_scale", "comp_flux"):
        assert isinstance(info[key], np.ndarray) and _same(info[key], ref_info[key])
    t_img = _t(img)
    model, res, info = multiscale.ms_clean(t_img, _t(psf), *weights, gain=0.2, niter=20)
    assert model.is_cuda and _same(res.cpu().numpy(), ref_res) and _same(t_img.cpu().numpy(), img)


# ------------------------------------------------------------ validation ----
def test_invalid_arguments_raise_and_leave_the_residual_alone():
    import torch

    img, psf, weights = _images(2, 70, 45), _psfs(2, 33, 21), _weights(2)
    res, p = _t(img), _t(psf)
    nan = np.array([1.0, np.nan])
    bad = [dict(sw=nan), dict(fs=nan), dict(sw=np.ones(3)), dict(fs=np.ones((2, 1))), dict(gain=0.0),
           dict(gain=float("nan")), dict(threshold=-1.0), dict(niter=-1), dict(batch=-1), dict(psf_centre=(33, 0)),
           dict(psf_centre=(-2, 0))]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(ValueError):
            multiscale.device_ms_clean(res, p, kw.pop("sw", weights[0]), kw.pop("fs", weights[1]), inplace=True, **kw)
        assert _same(res.cpu().numpy(), img), kw
    # the C ABI itself: one component array without the others
    so = _lib.lib()
    comp = torch.zeros(16, dtype=torch.int64, device="cuda")
    out = _lib.MsResult()
    pf64 = ctypes.POINTER(ctypes.c_double)

    def call(nscales=2, ci=None, cs=None, cf=None):
        return so.cip_ms_clean(res.data_ptr(), nscales, 70, 45, p.data_ptr(), 33, 21, -1, -1,
                               weights[0].ctypes.data_as(pf64), weights[1].ctypes.data_as(pf64), None, 0.1, 0.0, 4, 0,
                               None, None, ci, cs, cf, out)

    for kw in (dict(nscales=0), dict(nscales=7), dict(ci=comp.data_ptr()), dict(ci=comp.data_ptr(), cf=comp.data_ptr())):
        assert call(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_ms_clean" in so.cip_last_error()
        assert _same(res.cpu().numpy(), img), kw
    assert call() == 0 and out.niter_done == 4 and out.peak_scale in (0, 1)
    assert not _same(res.cpu().numpy(), img)
    # tensors of the wrong kind never reach the library
    with pytest.raises(ValueError):
        multiscale.device_ms_clean(res.float(), p, *weights)
    with pytest.raises(ValueError):
        multiscale.device_ms_clean(_t(img), p[:2], *weights)  # 2 cross PSFs for 2 scales
    with pytest.raises(ValueError):
        multiscale.device_ms_clean(_t(img), p, *weights, mask=torch.ones((45, 70), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        multiscale.device_ms_clean(_t(img), p.cpu(), *weights)
