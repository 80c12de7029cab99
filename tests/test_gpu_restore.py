"""
GPU tests of the restoring step (`cip_restore`, `cip_beam_fit`, through
`ska_sdp_cip_amd.restore`) and of `device_major_cycles(restore=True)`.

The restore's rounding and the order of its adds are part of its definition
(include/cip_restore.h), so every restore case asserts equality of BITS with the
numpy statement `_restore_np.restore`, fed the table the library itself reports
(`beam_taps`). No tolerances. The default beam is elongated and rotated
(b != 0), so a transposed or mirrored table shows.

Tiles are 32 rows x 128 columns; the shapes and component positions sit on
both sides of their edges and exactly R and R + 1 pixels away from them.
"""

import ctypes

import numpy as np
import pytest

import _restore_np as rnp
from ska_sdp_cip_amd import _lib, deconvolve
from ska_sdp_cip_amd import restore as rst
from test_gpu_clean import MAJOR, NPIX, _first_peak, _same, _t, major_scene

pytestmark = pytest.mark.gpu

BEAM = rst.beam_from_fwhm(6.0, 3.0, 0.3)
RADII = (0, 1, 5, 13, 32)
SHAPES = ((1, 1), (1, 300), (300, 1), (70, 45), (97, 391))
ROW_EDGES, COL_EDGES = (32, 64), (128, 256)


def _model(shape, R, seed=11):
    """Non-zeros at the four corners, on both sides of every tile edge, exactly
    R and R + 1 pixels before and after an edge (the halo is reached / is not),
    and a seeded sprinkle; everything else +0.0."""
    nx, ny = shape
    rng = np.random.default_rng(seed)
    model = np.zeros(shape)
    rows = {0, nx - 1, nx // 2}
    cols = {0, ny - 1, ny // 2}
    for e in ROW_EDGES:
        rows |= {e - 1, e, e - R, e - R - 1, e - 1 + R, e + R}
    for e in COL_EDGES:
        cols |= {e - 1, e, e - R, e - R - 1, e - 1 + R, e + R}
    rows = sorted(r for r in rows if 0 <= r < nx)
    cols = sorted(c for c in cols if 0 <= c < ny)
    for i in rows:
        for j in cols:
            model[i, j] = rng.standard_normal()
    extra = rng.choice(nx * ny, size=min(nx * ny, 40), replace=False)
    model.ravel()[extra] = rng.standard_normal(extra.size)
    for i, j in ((0, 0), (0, ny - 1), (nx - 1, 0), (nx - 1, ny - 1)):
        model[i, j] = 1.0 + rng.random()
    return model


def _residual(shape, seed=12):
    return np.random.default_rng(seed).standard_normal(shape)


def _check(model, residual, beam=BEAM, radius=None, **kw):
    """One device run against the numpy statement; returns the reference."""
    taps = rst.beam_taps(beam, radius)
    ref = rnp.restore(model, residual, taps)
    m, r = _t(model), _t(residual)
    out = rst.device_restore(m, r, beam, radius=radius, **kw)
    got = out.cpu().numpy()
    assert _same(m.cpu().numpy(), model)  # the inputs are left alone
    if residual is not None and not kw.get("inplace"):
        assert _same(r.cpu().numpy(), residual)
    if not _same(got, ref):
        bad = np.argwhere(got.view(np.int64) != ref.view(np.int64))
        raise AssertionError(f"{len(bad)} pixels differ, first {bad[:5].tolist()}, shape {model.shape}, R {radius}")
    return ref


# ------------------------------------------------------- shapes and radii ----
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_and_radii(shape, radius):
    model = _model(shape, radius)
    ref = _check(model, _residual(shape), radius=radius)
    if radius == 0:  # taps[0] = 1: out = residual + model
        assert _same(ref, _residual(shape) + model)


def test_dense_model_full_blocks():
    # every compaction block full, three column tiles, the order across row blocks
    model = np.random.default_rng(21).standard_normal((64, 256))
    _check(model, _residual((64, 256)), radius=32)


def test_dense_model_odd_shape():
    model = np.random.default_rng(22).standard_normal((33, 129))
    _check(model, None, radius=5)


def test_the_order_of_the_adds_is_observable():
    # the yardstick itself: reversing the component order changes most pixels of a dense case
    model = np.random.default_rng(23).standard_normal((40, 60))
    taps = rst.beam_taps(BEAM, 5)
    ref = rnp.restore(model, None, taps)
    rev = rnp.restore(model[::-1, ::-1], None, taps[::-1, ::-1])[::-1, ::-1]  # the same sums, descending order
    assert np.allclose(ref, rev, rtol=0, atol=1e-12)
    assert (ref.view(np.int64) != rev.view(np.int64)).mean() > 0.5
    _check(model, None, radius=5)


@pytest.fixture(scope="module")
def sparse():
    """1024 x 1024 with 500 seeded non-zeros, 100 of them within a few pixels of
    another one, and a seeded residual; the default radius of BEAM is 16."""
    rng = np.random.default_rng(31)
    model = np.zeros((1024, 1024))
    idx = rng.choice(1024 * 1024, size=400, replace=False)
    model.ravel()[idx] = rng.standard_normal(400)
    for k in idx[:100]:
        i, j = divmod(int(k), 1024)
        i2, j2 = min(i + int(rng.integers(0, 6)), 1023), min(j + int(rng.integers(1, 9)), 1023)
        model[i2, j2] = rng.standard_normal()
    residual = rng.standard_normal((1024, 1024))
    return model, residual, rnp.restore(model, residual, rst.beam_taps(BEAM))


def test_sparse_1024(sparse):
    model, residual, ref = sparse
    assert 490 <= np.count_nonzero(model) <= 500 and rst.beam_radius(BEAM) == 16
    out = rst.device_restore(_t(model), _t(residual), BEAM)
    assert _same(out.cpu().numpy(), ref)


# --------------------------------------------------------- special values ----
def test_all_zero_model_returns_the_residual():
    shape = (70, 45)
    residual = _residual(shape)
    model = np.zeros(shape)
    ref = _check(model, residual, radius=5)
    assert _same(ref, residual)
    r = _t(residual)
    out = rst.device_restore(_t(model), r, BEAM, radius=5, inplace=True)
    assert out is r and _same(r.cpu().numpy(), residual)


def test_no_residual():
    shape = (70, 45)
    model = _model(shape, 5)
    ref = _check(model, None, radius=5)
    assert not np.signbit(ref[ref == 0]).any()  # out starts from +0.0


def test_signed_zeros_are_skipped():
    shape = (70, 45)
    model = np.zeros(shape)
    model[::2] = -0.0
    residual = np.full(shape, -0.0)
    ref = _check(model, residual, radius=5)
    assert np.signbit(ref).all()  # -0.0 + (+-0.0 * tap) would have made +0.0
    model[40, 20] = 2.0
    ref = _check(model, residual, radius=5)
    assert np.signbit(ref[0, 0]) and ref[40, 20] == 2.0 and np.count_nonzero(ref) == 11 * 11


def test_nan_and_inf_poison_exactly_their_windows():
    shape = (97, 391)
    model = _model(shape, 5)
    model[50, 200], model[10, 380] = np.nan, np.inf
    residual = _residual(shape)
    ref = _check(model, residual, radius=5)
    want_nan = np.zeros(shape, dtype=bool)
    want_nan[45:56, 195:206] = True
    assert np.array_equal(np.isnan(ref), want_nan)
    want_inf = np.zeros(shape, dtype=bool)
    want_inf[5:16, 375:386] = True
    assert np.array_equal(np.isposinf(ref), want_inf)


# -------------------------------------------------------------- call forms ----
def test_inplace_and_out():
    import torch

    shape = (97, 391)
    model, residual = _model(shape, 13), _residual(shape)
    ref = _check(model, residual, radius=13)
    _check(model, residual, radius=13, inplace=True)
    m, r = _t(model), _t(residual)
    got = rst.device_restore(m, r, BEAM, radius=13, inplace=True)
    assert got is r and _same(r.cpu().numpy(), ref)
    out = torch.full(shape, 7.0, dtype=torch.float64, device="cuda")
    got = rst.device_restore(m, _t(residual), BEAM, radius=13, out=out)
    assert got is out and _same(out.cpu().numpy(), ref)
    got = rst.device_restore(m, None, BEAM, radius=13, out=out)  # out holds stale values: all overwritten
    assert _same(got.cpu().numpy(), rnp.restore(model, None, rst.beam_taps(BEAM, 13)))


def test_non_default_stream():
    import torch

    shape = (97, 391)
    model, residual = _model(shape, 13), _residual(shape)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _check(model, residual, radius=13)
        _check(model, residual, beam=rst.beam_from_fwhm(4.0, 4.0, 0.0), radius=7)  # another table on that stream
    stream.synchronize()
    _check(model, residual, radius=13)  # and back on the default stream, the first table again


def test_shapes_alternate_through_one_workspace_and_release(sparse):
    a = (_model((70, 45), 5), _residual((70, 45)), dict(radius=5))
    b = (sparse[0], sparse[1], dict())
    other = rst.beam_from_fwhm(5.0, 2.5, -1.2)
    for case in (a, b, a, b):
        _check(*case[:2], **case[2])
    _check(a[0], a[1], beam=other, radius=5)  # same radius, another beam: a new table
    _check(a[0], a[1], radius=5)
    assert _lib.lib().cip_release_workspace() == 0
    assert _same(rst.device_restore(_t(b[0]), _t(b[1]), BEAM).cpu().numpy(), sparse[2])
    _check(*a[:2], **a[2])


def test_identical_calls_give_identical_bits():
    model = np.random.default_rng(41).standard_normal((64, 256))
    m, r = _t(model), _t(_residual((64, 256)))
    first = rst.device_restore(m, r, BEAM, radius=13).cpu().numpy()
    for _ in range(3):
        assert _same(rst.device_restore(m, r, BEAM, radius=13).cpu().numpy(), first)


def test_host_entry_point_numpy_and_torch(sparse):
    model, residual, ref = sparse
    out = rst.restore(model, residual, BEAM)
    assert isinstance(out, np.ndarray) and _same(out, ref)
    t_model = _t(model)
    out = rst.restore(t_model, _t(residual), BEAM)
    assert out.is_cuda and _same(out.cpu().numpy(), ref) and _same(t_model.cpu().numpy(), model)


# ---------------------------------------------------------------- the beam ----
def _window(psf, centre, radius):
    """The (2 r + 1)^2 window of `psf` around `centre`, NaN outside the PSF."""
    n = 2 * radius + 1
    win = np.full((n, n), np.nan)
    cx, cy = centre
    for ia in range(n):
        for ib in range(n):
            i, j = cx - radius + ia, cy - radius + ib
            if 0 <= i < psf.shape[0] and 0 <= j < psf.shape[1]:
                win[ia, ib] = psf[i, j]
    return win


@pytest.mark.parametrize("scales", [(1.0, 1.0), (0.45, 0.8)], ids=["iso", "aniso"])
@pytest.mark.parametrize("cut", [0.5, 0.35])
def test_fit_beam_equals_the_host_fit_of_the_same_window(scales, cut):
    uvw, freq, _, wgt, pix = major_scene()
    psf = rnp.dft_psf(uvw, freq, wgt, pix, 16, *scales)  # 33 x 33, the peak at (16, 16)
    got = rst.device_fit_beam(_t(psf), cut=cut)
    assert got == rst.beam_fit_window(psf[8:25, 8:25], cut=cut)  # same host code, same bytes
    a, b, c, n = rnp.fit_window(psf[8:25, 8:25], cut)
    assert got["n_fit"] == n and abs(got["a"] - a) <= 1e-10 * max(a, c) and abs(got["c"] - c) <= 1e-10 * max(a, c)


@pytest.mark.parametrize("centre", [(0, 0), (38, 3), (12, 20), (39, 29)])
def test_fit_beam_with_clipped_windows(centre):
    form = (0.11, 0.03, 0.2)
    i, j = np.arange(40, dtype=np.float64)[:, None] - centre[0], np.arange(30, dtype=np.float64)[None, :] - centre[1]
    psf = 0.9 * np.exp(-(form[0] * i * i + 2 * form[1] * i * j + form[2] * j * j))
    got = rst.device_fit_beam(_t(psf), psf_centre=centre)
    win = _window(psf, centre, 8)
    assert np.isnan(win).any() == (centre != (12, 20))
    assert got == rst.beam_fit_window(win)
    assert abs(got["a"] - form[0]) <= 1e-10 * form[2] and abs(got["b"] - form[1]) <= 1e-10 * form[2]


def test_fit_beam_on_a_patch_smaller_than_the_window():
    psf = rnp.gaussian(0.3, 0.05, 0.25, 2)  # 5 x 5, radius 8: the window is mostly outside
    got = rst.device_fit_beam(_t(psf), cut=0.2, radius=8)
    assert got == rst.beam_fit_window(_window(psf, (2, 2), 8), cut=0.2)
    assert abs(got["a"] - 0.3) <= 3e-11 and abs(got["b"] - 0.05) <= 3e-11 and abs(got["c"] - 0.25) <= 3e-11
    assert got == rst.device_fit_beam(_t(psf), cut=0.2, radius=2)  # the same pixels
    with pytest.raises(ValueError, match="lower cut"):
        rst.device_fit_beam(_t(rnp.gaussian(0.6, 0.2, 0.5, 8)), cut=0.5)


# -------------------------------------------------------------- validation ----
def test_invalid_arguments_raise_and_leave_out_alone():
    import torch

    shape = (70, 45)
    model, residual = _t(_model(shape, 5)), _t(_residual(shape))
    stale = np.full(shape, 3.0)
    out = _t(stale)
    bad_beam = {"a": 0.1, "b": 0.2, "c": 0.1}
    cases = [
        dict(args=(model, residual, BEAM), kw=dict(out=model)),                        # out is the model
        dict(args=(model, residual, BEAM), kw=dict(out=model.view(-1).view(shape))),   # the same memory
        dict(args=(model.float(), residual, BEAM), kw=dict(out=out)),                  # dtype
        dict(args=(model, residual.float(), BEAM), kw=dict(out=out)),
        dict(args=(model, _t(_residual((45, 70))), BEAM), kw=dict(out=out)),           # shape
        dict(args=(model, residual, BEAM), kw=dict(out=_t(np.zeros((45, 70))))),
        dict(args=(model.view(-1), None, BEAM), kw=dict()),                            # not 2-D
        dict(args=(model.cpu(), residual, BEAM), kw=dict(out=out)),                    # device
        dict(args=(model, residual.cpu(), BEAM), kw=dict(out=out)),
        dict(args=(model, residual, BEAM), kw=dict(out=out, radius=33)),               # radius
        dict(args=(model, residual, BEAM), kw=dict(out=out, radius=-2)),
        dict(args=(model, residual, bad_beam), kw=dict(out=out, radius=5)),            # not positive definite
        dict(args=(model, residual, bad_beam), kw=dict(out=out)),
        dict(args=(model, residual, rst.beam_from_fwhm(13.0, 13.0, 0.0)), kw=dict(out=out)),  # needs R = 34
        dict(args=(model, residual, BEAM), kw=dict(out=out, tol=0.0)),
        dict(args=(model, residual, BEAM), kw=dict(out=out, inplace=True)),            # inplace and out
        dict(args=(model, None, BEAM), kw=dict(inplace=True)),                         # inplace without a residual
    ]
    for case in cases:
        with pytest.raises(ValueError):
            rst.device_restore(*case["args"], **case["kw"])
        assert _same(out.cpu().numpy(), stale), case["kw"]
    # the C ABI itself
    so = _lib.lib()
    beam = _lib.Beam(a=BEAM["a"], b=BEAM["b"], c=BEAM["c"])
    mp, op = model.data_ptr(), out.data_ptr()

    def call(m=mp, r=None, nx=70, ny=45, b=ctypes.byref(beam), radius=5, o=op):
        return so.cip_restore(m, r, nx, ny, b, radius, None, o)

    for kw in (dict(m=None), dict(o=None), dict(b=None), dict(o=mp), dict(nx=0), dict(ny=-3), dict(radius=33)):
        assert call(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_restore" in so.cip_last_error()
        assert _same(out.cpu().numpy(), stale), kw
    assert call() == 0
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), rnp.restore(model.cpu().numpy(), None, rst.beam_taps(BEAM, 5)))
    with pytest.raises(ValueError):
        rst.device_fit_beam(model.float())
    with pytest.raises(ValueError):
        rst.device_fit_beam(model.cpu())
    with pytest.raises(ValueError):
        rst.device_fit_beam(model, psf_centre=(70, 0))
    with pytest.raises(ValueError):
        rst.device_fit_beam(model, psf_centre=(-2, 0))


# ------------------------------------------------------------- major cycle ----
def test_major_cycles_restore():
    """The yardstick for the beam is the fit of this scene's PSF by direct DFT at
    the default cut 0.35, computed here on the CPU: a = 0.185989, c = 0.185986
    over 20 pixels, which the shape formulas turn into FWHM 3.8612 / 3.8608 px
    (2 sqrt(ln 2 / 0.185989) = 3.8612). The request for this test quoted
    3.8950 / 3.8946 beside the same a = 0.185989; those two figures do not
    follow from that a, so the test takes the DFT fit itself, with the bound
    that was asked for. The epsilon = 1e-4 gridded PSF differs from the DFT by
    about 1e-4 of the peak, which moves the FWHM by about 1e-3 px: 0.01 leaves
    a tenfold margin."""
    uvw, freq, vis, wgt, pix = major_scene()
    threshold = 1e-3 * _first_peak(uvw, freq, vis, wgt, pix)
    d = (_t(uvw), _t(freq), _t(vis), _t(wgt))
    out = deconvolve.device_major_cycles(*d, NPIX, pix, threshold=threshold, do_wstacking=False, restore=True, **MAJOR)
    plain = deconvolve.device_major_cycles(*d, NPIX, pix, threshold=threshold, do_wstacking=False, **MAJOR)
    assert set(plain) == {"model", "residual", "psf", "peaks", "components", "stop_reason"}
    assert set(out) == set(plain) | {"beam", "restored"}
    assert out["stop_reason"] == plain["stop_reason"] == "threshold" and out["components"] == plain["components"]
    for name in ("model", "residual", "psf"):
        assert _same(out[name].cpu().numpy(), plain[name].cpu().numpy()), name
    beam = out["beam"]
    print("beam", beam)
    assert beam == rst.device_fit_beam(out["psf"])
    a, b, c, n = rnp.fit_window(rnp.dft_psf(uvw, freq, wgt, pix, 8), 0.35)
    dft_major, dft_minor, _ = rnp.shape(a, b, c)
    assert abs(a - 0.185989) <= 2e-6 and n == 20
    assert abs(dft_major - 3.8612) <= 1e-4 and abs(dft_minor - 3.8608) <= 1e-4
    print("dft", (a, b, c), (dft_major, dft_minor))
    assert abs(beam["fwhm_major"] - dft_major) <= 0.01 and abs(beam["fwhm_minor"] - dft_minor) <= 0.01
    assert beam["n_fit"] == 20
    model, residual = out["model"].cpu().numpy(), out["residual"].cpu().numpy()
    assert _same(out["restored"].cpu().numpy(), rnp.restore(model, residual, rst.beam_taps(beam)))
    # a beam that is passed is used as it is
    given = rst.beam_from_fwhm(5.0, 4.0, 0.5)
    out2 = deconvolve.device_major_cycles(*d, NPIX, pix, threshold=threshold, do_wstacking=False, restore=True,
                                          beam=given, **MAJOR)
    assert out2["beam"] == given
    assert _same(out2["restored"].cpu().numpy(), rnp.restore(model, residual, rst.beam_taps(given)))
