"""
GPU tests of the degridder: `cip_dirty2ms` (through its C ABI, via
`ska_sdp_cip_amd.gridder`), the exact transpose of `cip_ms2dirty`.

References:
  * the untouched oracle's transpose, per visibility k:
        ref_k = <oracle.ms2dirty(delta_k), I> + i <oracle.ms2dirty(i delta_k), I>
    (two oracle calls per sample, so sampled visibilities only);
  * the explicit numpy DFT of the definition, for every visibility:
        vis[r,c] = sum_{i,j} I[i,j]/n exp(-2 pi i f_c/c (u l + v m - w (n - 1))).
Errors are normalised by sum |I| (each visibility is a sum of |I| terms of
modulus <= 1 times kernel errors). TIGHT is the project's fp64-class gate
(test_gpu_invert_parity.py); EXPECTED[W] the oracle-vs-DFT bounds of
test_oracle_accuracy.py - an operator and its transpose share the per-entry
bound, and the reference alone meets it.
"""

import ctypes

import numpy as np
import pytest

import oracle
from ska_sdp_cip_amd import _lib, gridder, predict, synthetic as syn
from test_oracle_accuracy import EXPECTED

pytestmark = pytest.mark.gpu

TIGHT = 1e-10
C = 299792458.0


def _t(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _geometry(n_rows, nchan, *, n_ant=16, radius=1000.0, seed=1):
    return syn.uvw_tracks(n_rows, n_ant, array_radius_m=radius, seed=seed), syn.channel_frequencies(nchan)


def _image(nx, ny, seed=11):
    return np.random.default_rng(seed).standard_normal((nx, ny))


def _gpu(uvw, f, img, wgt, px, py, **kw):
    vis, prm = gridder.device_dirty2ms(_t(uvw), _t(f), _t(img), _t(wgt), px, py, **kw)
    return vis.cpu().numpy(), prm


def _dft_predict(uvw, f, img, px, py, wstack):
    """The definition, every visibility, fp64 numpy."""
    nx, ny = img.shape
    l = (np.arange(nx) - nx // 2) * px  # noqa: E741
    m = (np.arange(ny) - ny // 2) * py
    lam = f / C
    out = np.empty((uvw.shape[0], f.size), dtype=np.complex128)
    if not wstack:  # separable: vis_k = a_k^T I b_k
        for c in range(f.size):
            a = np.exp(-2j * np.pi * lam[c] * uvw[:, 0:1] * l[None, :])
            b = np.exp(-2j * np.pi * lam[c] * uvw[:, 1:2] * m[None, :])
            out[:, c] = ((a @ img) * b).sum(axis=1)
        return out
    e = l[:, None] ** 2 + m[None, :] ** 2
    nm1 = -e / (np.sqrt(1.0 - e) + 1.0)
    scaled = (img / (nm1 + 1.0)).ravel()
    L, M, N1 = np.repeat(l, ny), np.tile(m, nx), nm1.ravel()
    for c in range(f.size):
        for r0 in range(0, uvw.shape[0], 256):
            u = uvw[r0:r0 + 256] * lam[c]
            ph = u[:, 0:1] * L + u[:, 1:2] * M - u[:, 2:3] * N1
            out[r0:r0 + 256, c] = np.exp(-2j * np.pi * ph) @ scaled
    return out


def _ref_samples(uvw, f, img, px, py, support, wstack, idx):
    """ref_k of the sampled flat visibility indices `idx` (oracle transpose)."""
    nx, ny = img.shape
    delta = np.zeros((uvw.shape[0], f.size), dtype=np.complex128)
    ref = np.empty(len(idx), dtype=np.complex128)
    for n, k in enumerate(idx):
        parts = []
        for unit in (1.0, 1.0j):
            delta.flat[k] = unit
            d = oracle.ms2dirty(uvw, f, delta, None, nx, ny, px, py, support=support, do_wstacking=wstack)
            parts.append(float((d * img).sum()))
        delta.flat[k] = 0.0
        ref[n] = parts[0] + 1j * parts[1]
    return ref


def _sample(nvis, n=24, seed=5):
    return np.sort(np.random.default_rng(seed).choice(nvis, size=min(n, nvis), replace=False))


# ------------------------------------------------------------------ cases ----
@pytest.fixture(scope="module")
def base():
    """The case of test_oracle_accuracy.py: 3000 x 2 visibilities, 64^2 image."""
    uvw, f = _geometry(3_000, 2)
    npix = 64
    px = syn.pixel_size_for_grid(uvw, f, npix, fill=0.8)
    img = _image(npix, npix)
    dft = {ws: _dft_predict(uvw, f, img, px, px, ws) for ws in (False, True)}
    return uvw, f, img, px, dft


@pytest.fixture(scope="module")
def wide():
    """The wide-field case of test_wstacking_parity_vs_oracle_and_dft."""
    uvw, f = _geometry(4_000, 4, n_ant=24, radius=2000.0, seed=3)
    npix = 192
    px = syn.pixel_size_for_grid(uvw, f, npix, fill=0.3)
    return uvw, f, _image(npix, npix), px


# ------------------------------------------------------ 1. parity, sampled ----
@pytest.mark.parametrize("support", [4, 8, 12, 16])
def test_parity_sampled_2d(gpu_device, base, support):
    uvw, f, img, px, _ = base
    idx = _sample(uvw.shape[0] * f.size)
    gpu, prm = _gpu(uvw, f, img, None, px, px, support=support)
    ref = _ref_samples(uvw, f, img, px, px, support, False, idx)
    err = float(np.abs(gpu.ravel()[idx] - ref).max() / np.abs(img).sum())
    print(f"dirty2ms 2-D W={support}: max|gpu - ref_k| / sum|I| = {err:.3e}")
    assert prm.support == support and prm.nplanes == 1
    assert err < TIGHT, err


@pytest.mark.parametrize("support", [6, 10])
def test_parity_sampled_wstacking(gpu_device, wide, support):
    uvw, f, img, px = wide
    idx = _sample(uvw.shape[0] * f.size)
    gpu, prm = _gpu(uvw, f, img, None, px, px, support=support, do_wstacking=True)
    # several plane groups, the last one partial (W = 10: the 11 planes of the
    # invert's parity test; W = 6 has 7)
    group = _lib.plane_group(prm)
    assert prm.nplanes % group != 0 and prm.nplanes > group
    if support == 10:
        assert prm.nplanes > 10
    ref = _ref_samples(uvw, f, img, px, px, support, True, idx)
    err = float(np.abs(gpu.ravel()[idx] - ref).max() / np.abs(img).sum())
    print(f"dirty2ms w-stacking W={support} nplanes={prm.nplanes} G={group}: "
          f"max|gpu - ref_k| / sum|I| = {err:.3e}")
    assert err < TIGHT, err


# ----------------------------------------------- 2. parity, every visibility ----
@pytest.mark.parametrize("support,wstack", [(8, False), (16, False), (8, True), (12, True)])
def test_parity_every_visibility_vs_dft(gpu_device, base, support, wstack):
    uvw, f, img, px, dft = base
    gpu, _ = _gpu(uvw, f, img, None, px, px, support=support, do_wstacking=wstack)
    err = float(np.abs(gpu - dft[wstack]).max() / np.abs(img).sum())
    print(f"dirty2ms vs DFT W={support} wstack={wstack}: {err:.3e}")
    assert err < EXPECTED[support], err


# ------------------------------------------------------- 3. adjointness ----
@pytest.mark.parametrize("wstack", [False, True])
def test_adjointness_on_device(gpu_device, base, wstack):
    import torch

    uvw, f, img, px, _ = base
    rng = np.random.default_rng(21)
    shape = (uvw.shape[0], f.size)
    y = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    wgt = rng.uniform(0.5, 1.5, shape).astype(np.float32)
    tu, tf, ty, tw, ti = _t(uvw), _t(f), _t(y), _t(wgt), _t(img)
    dirty, _ = gridder.device_ms2dirty(tu, tf, ty, tw, 64, 64, px, px, support=8, do_wstacking=wstack)
    vis, _ = gridder.device_dirty2ms(tu, tf, ti, tw, px, px, support=8, do_wstacking=wstack)
    lhs = float((dirty * ti).sum())
    rhs = float((ty.conj() * vis).real.sum())
    scale = float(np.abs(wgt.astype(np.float64) * y).sum() * np.abs(img).sum())
    print(f"adjointness wstack={wstack}: |lhs - rhs| / scale = {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= 1e-10 * scale
    torch.cuda.synchronize()


# ---------------------------------------------------- 4. geometry traps ----
def test_nonsquare_multichannel(gpu_device):
    # runs of 64 channels cross tile boundaries; nu != nv
    uvw, f = _geometry(150, 64, n_ant=32, radius=3000.0, seed=3)
    nx, ny = 96, 160
    px = syn.pixel_size_for_grid(uvw, f, nx)
    py = syn.pixel_size_for_grid(uvw, f, ny)
    img = _image(nx, ny)
    gpu, prm = _gpu(uvw, f, img, None, px, py, support=12)
    assert (prm.nu, prm.nv) == (192, 320)
    err = float(np.abs(gpu - _dft_predict(uvw, f, img, px, py, False)).max() / np.abs(img).sum())
    assert err < EXPECTED[12], err


@pytest.mark.parametrize("wstack", [False, True])
def test_npix_66_partial_edge_tile(gpu_device, wstack):
    # 2 * 66 = 132 has the factor 11, so the grid is the next 2/3/5/7-smooth size,
    # 140 cells: 5 tiles per axis, the last one 12 cells wide; hipFFT non-power-of-two
    uvw, f = _geometry(3_001, 3)  # 9003 visibilities: not a multiple of 256
    npix = 66
    px = syn.pixel_size_for_grid(uvw, f, npix, fill=0.95)
    img = _image(npix, npix)
    gpu, prm = _gpu(uvw, f, img, None, px, px, support=12, do_wstacking=wstack)
    assert prm.nu == 140 and -(-prm.nu // prm.tile) == 5 and (uvw.shape[0] * f.size) % 256 != 0
    err = float(np.abs(gpu - _dft_predict(uvw, f, img, px, px, wstack)).max() / np.abs(img).sum())
    assert err < EXPECTED[12], err


@pytest.mark.parametrize("wstack", [False, True])
def test_wrapped_baselines(gpu_device, wstack):
    # pixel 3x too coarse: most baselines lie beyond the grid and wrap
    # (test_oracle_wraps_periodic_uv_exactly)
    ms_uvw = syn.uvw_tracks(3_000, 16, array_radius_m=1000.0, seed=1)
    f = syn.channel_frequencies(2)
    npix = 64
    px = syn.pixel_size_for_grid(ms_uvw, f, npix) * 3.0
    img = _image(npix, npix)
    gpu, _ = _gpu(ms_uvw, f, img, None, px, px, support=12, do_wstacking=wstack)
    err = float(np.abs(gpu - _dft_predict(ms_uvw, f, img, px, px, wstack)).max() / np.abs(img).sum())
    assert err < EXPECTED[12], err


def test_hot_tile_is_split(gpu_device):
    # 80,000 single-channel visibilities of a 50 m array on the pixel grid of a
    # 1000 m one: every footprint starts in the tiles around the grid centre,
    # so a tile holds more than kChunkVis = 16384 visibilities and is split
    big, f = _geometry(100, 1)
    uvw = syn.uvw_tracks(80_000, 16, array_radius_m=50.0, seed=2)
    npix = 64
    px = syn.pixel_size_for_grid(big, f, npix)
    img = _image(npix, npix)
    _lib.profile_enable(True)
    try:
        gpu, _ = _gpu(uvw, f, img, None, px, px, support=8)
        prof = _lib.profile_last()
    finally:
        _lib.profile_enable(False)
    assert prof["visibilities"] == 80_000 and prof["chunks"] > 4
    assert prof["chunks"] <= 4 + 80_000 // 16384 + 1  # at most four tiles, split into full chunks
    err = float(np.abs(gpu - _dft_predict(uvw, f, img, px, px, False)).max() / np.abs(img).sum())
    assert err < EXPECTED[8], err


# ------------------------------------------------- 5. dtypes and weights ----
@pytest.mark.parametrize("wstack", [False, True])
def test_dtypes_weights_and_zero_weights(gpu_device, base, wstack):
    import torch

    uvw, f, img, px, _ = base
    shape = (uvw.shape[0], f.size)
    rng = np.random.default_rng(8)
    w64 = rng.uniform(0.5, 1.5, shape)
    w64[rng.uniform(size=shape) < 0.1] = 0.0
    kw = dict(support=8, do_wstacking=wstack)
    plain, _ = _gpu(uvw, f, img, None, px, px, **kw)
    scale = np.abs(plain).max()
    for wgt in (w64, w64.astype(np.float32)):
        got, _ = _gpu(uvw, f, img, wgt, px, px, **kw)
        assert got.dtype == np.complex128
        assert np.abs(got - wgt.astype(np.float64) * plain).max() <= 1e-14 * scale
        assert np.all(got[wgt == 0] == 0)  # exact zeros
    c64, _ = _gpu(uvw, f, img, w64, px, px, out_dtype=torch.complex64, **kw)
    assert c64.dtype == np.complex64
    assert np.abs(c64 - w64 * plain).max() <= 2.0 ** -23 * scale
    assert np.all(c64[w64 == 0] == 0)
    # `out` is written in place
    out = torch.full(shape, 7.0, dtype=torch.complex128, device="cuda")
    res, _ = gridder.device_dirty2ms(_t(uvw), _t(f), _t(img), None, px, px, out=out, **kw)
    assert res is out and np.array_equal(out.cpu().numpy(), plain)


def test_dropin_rules(gpu_device, base):
    import torch

    uvw, f, img, px, _ = base
    plain, _ = _gpu(uvw, f, img, None, px, px, support=8)
    # numpy in -> numpy out; ducc's positional order; nu / nv / nthreads / verbosity ignored
    got = gridder.dirty2ms(uvw, f, img, None, px, px, 0, 0, 1e-4, False, 4, 0, support=8)
    assert isinstance(got, np.ndarray) and got.dtype == np.complex128 and np.array_equal(got, plain)
    # float32 image -> complex64 (fp64 arithmetic on the float32 values)
    got32 = gridder.dirty2ms(uvw, f, img.astype(np.float32), None, px, px, support=8)
    ref32, _ = _gpu(uvw, f, img.astype(np.float32).astype(np.float64), None, px, px, support=8)
    assert got32.dtype == np.complex64 and np.array_equal(got32, ref32.astype(np.complex64))
    # torch in -> torch out, on the device
    tt, prm = gridder.dirty2ms(_t(uvw), _t(f), _t(img), None, px, px, support=8, return_params=True)
    assert torch.is_tensor(tt) and tt.is_cuda and prm.support == 8
    assert np.array_equal(tt.cpu().numpy(), plain)
    # mask zeroes weights where 0
    mask = (np.random.default_rng(2).uniform(size=plain.shape) < 0.5).astype(np.uint8)
    wgt = np.full(plain.shape, 2.0, dtype=np.float32)
    m = gridder.dirty2ms(uvw, f, img, wgt, px, px, mask=mask, support=8)
    assert np.all(m[mask == 0] == 0) and np.array_equal(m[mask == 1], 2.0 * plain[mask == 1])
    m0 = gridder.dirty2ms(uvw, f, img, None, px, px, mask=mask, support=8)
    assert np.array_equal(m0, np.where(mask == 1, plain, 0.0))
    # epsilon selects the support as in ms2dirty
    _, p4 = gridder.dirty2ms(uvw, f, img, None, px, px, epsilon=1e-4, return_params=True)
    assert p4.support == oracle.support_for_epsilon(1e-4)
    # predict.py
    asec = syn.pixel_size_asec(px)
    pix = float(np.sin(np.radians(asec / 3600.0)))
    pr = predict.ducc_predict(uvw, f, img, asec, epsilon=1e-4, do_wstacking=False, support=8)
    again, _ = _gpu(uvw, f, img, None, pix, pix, support=8)
    assert np.array_equal(pr, again)


@pytest.mark.parametrize("wstack", [False, True])
def test_nrow_zero(gpu_device, wstack):
    import torch

    uvw = torch.empty((0, 3), dtype=torch.float64, device="cuda")
    f = _t(syn.channel_frequencies(4))
    img = _t(_image(64, 64))
    vis, prm = gridder.device_dirty2ms(uvw, f, img, None, 1e-4, 1e-4, support=8, do_wstacking=wstack)
    assert tuple(vis.shape) == (0, 4) and prm.support == 8 and prm.nu == 128
    got = gridder.dirty2ms(np.empty((0, 3)), syn.channel_frequencies(4), _image(64, 64), None, 1e-4, 1e-4)
    assert got.shape == (0, 4)


# ------------------------------------------------------------ 6. subtract ----
@pytest.mark.parametrize("wstack", [False, True])
def test_subtract(gpu_device, base, wstack):
    import torch

    uvw, f, img, px, _ = base
    shape = (uvw.shape[0], f.size)
    rng = np.random.default_rng(4)
    data = 500.0 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    kw = dict(support=8, do_wstacking=wstack)
    tu, tf, ti = _t(uvw), _t(f), _t(img)
    model, _ = gridder.device_dirty2ms(tu, tf, ti, None, px, px, **kw)
    # complex128, no weights: the same two roundings as vis - model
    out = _t(data)
    gridder.device_dirty2ms(tu, tf, ti, None, px, px, out=out, subtract=True, **kw)
    assert torch.equal(out, _t(data) - model)
    # complex64: one rounding to float32 of the fp64 difference
    d32 = data.astype(np.complex64)
    out32 = _t(d32)
    gridder.device_dirty2ms(tu, tf, ti, None, px, px, out=out32, subtract=True, **kw)
    exact = d32.astype(np.complex128) - model.cpu().numpy()
    assert np.abs(out32.cpu().numpy() - exact).max() <= 2.0 ** -22 * np.abs(d32).max()
    # weighted, with zero weights left untouched
    wgt = rng.uniform(0.5, 1.5, shape).astype(np.float32)
    wgt[rng.uniform(size=shape) < 0.1] = 0.0
    outw = _t(data)
    gridder.device_dirty2ms(tu, tf, ti, _t(wgt), px, px, out=outw, subtract=True, **kw)
    want = data - wgt.astype(np.float64) * model.cpu().numpy()
    got = outw.cpu().numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(got[wgt == 0], data[wgt == 0])
    # predict.device_residual: a copy, or in place
    res = predict.device_residual(tu, tf, _t(data), ti, px, _t(wgt), **kw)
    assert torch.equal(res, outw)
    buf = _t(data)
    assert predict.device_residual(tu, tf, buf, ti, px, _t(wgt), inplace=True, **kw) is buf
    assert torch.equal(buf, outw)


# --------------------------------------------- 7. determinism and state ----
@pytest.mark.parametrize("wstack", [False, True])
def test_identical_calls_are_bit_identical(gpu_device, base, wstack):
    uvw, f, img, px, _ = base
    wgt = np.random.default_rng(3).uniform(0.5, 1.5, (uvw.shape[0], f.size)).astype(np.float32)
    a, _ = _gpu(uvw, f, img, wgt, px, px, support=8, do_wstacking=wstack)
    b, _ = _gpu(uvw, f, img, wgt, px, px, support=8, do_wstacking=wstack)
    assert np.array_equal(a, b)


def test_invert_predict_invert_keeps_the_clean_grid_state(gpu_device):
    # npix = 512: the 1024-cell grid of the pruned FFT, which relies on the
    # workspace grid being all-zero between inverts; the predict in between
    # fills that buffer with dense FFT output
    import torch

    uvw, f = _geometry(2_000, 4, n_ant=24, radius=2000.0, seed=3)
    npix = 512
    px = syn.pixel_size_for_grid(uvw, f, npix)
    rng = np.random.default_rng(6)
    vis = _t(rng.standard_normal((2_000, 4)) + 1j * rng.standard_normal((2_000, 4)))
    tu, tf = _t(uvw), _t(f)
    first, prm = gridder.device_ms2dirty(tu, tf, vis, None, npix, npix, px, px, support=8)
    assert prm.nu == 1024
    first = first.clone()
    gridder.device_dirty2ms(tu, tf, first, None, px, px, support=8)
    second, _ = gridder.device_ms2dirty(tu, tf, vis, None, npix, npix, px, px, support=8)
    assert torch.equal(first, second)


@pytest.mark.parametrize("wstack", [False, True])
def test_reuse_plan(gpu_device, base, wstack):
    import torch

    uvw, f, img, px, _ = base
    other_uvw, other_f = _geometry(1_000, 3, seed=9)
    rng = np.random.default_rng(12)
    vis = _t(rng.standard_normal((3_000, 2)) + 1j * rng.standard_normal((3_000, 2)))
    ovis = _t(rng.standard_normal((1_000, 3)) + 1j * rng.standard_normal((1_000, 3)))
    tu, tf, ti = _t(uvw), _t(f), _t(img)
    kw = dict(support=8, do_wstacking=wstack)
    fresh, _ = gridder.device_dirty2ms(tu, tf, ti, None, px, px, **kw)
    planned_invert, _ = gridder.device_ms2dirty(tu, tf, vis, None, 64, 64, px, px, **kw)
    planned_invert = planned_invert.clone()
    # after an invert of the same geometry: through its plan
    reused, _ = gridder.device_dirty2ms(tu, tf, ti, None, px, px, reuse_plan=True, **kw)
    assert torch.equal(reused, fresh)
    # after an invert of another geometry: plans as usual
    gridder.device_ms2dirty(_t(other_uvw), _t(other_f), ovis, None, 64, 64, px, px, **kw)
    replanned, _ = gridder.device_dirty2ms(tu, tf, ti, None, px, px, reuse_plan=True, **kw)
    assert torch.equal(replanned, fresh)
    # an invert reusing the plan that predict just made
    again, _ = gridder.device_ms2dirty(tu, tf, vis, None, 64, 64, px, px, reuse_plan=True, **kw)
    assert torch.equal(again, planned_invert)


# ---------------------------------------------------------- 8. validation ----
def _raw_call(uvw, f, img, out, px, *, support=8, flags=0):
    prm = _lib.GridderParams()
    return _lib.lib().cip_dirty2ms(uvw.data_ptr(), uvw.shape[0], f.data_ptr(), f.shape[0], img.data_ptr(),
                                   img.shape[0], img.shape[1], px, px, 1e-4, support, flags, None, _lib.CIP_NONE,
                                   None, out.data_ptr(), _lib.CIP_C128, ctypes.byref(prm))


def test_library_rejects_unsupported_modes(gpu_device, base):
    import torch

    uvw, f, img, px, _ = base
    tu, tf, ti = _t(uvw), _t(f), _t(img)
    out = torch.zeros((3_000, 2), dtype=torch.complex128, device="cuda")
    with pytest.raises(ValueError, match="support"):
        gridder.device_dirty2ms(tu, tf, ti, None, px, px, support=24)
    for flag, word in ((_lib.CIP_ACC_SINGLE, "CIP_ACC_SINGLE"), (_lib.CIP_PSF, "CIP_PSF"),
                       (_lib.CIP_NORMALISE, "CIP_NORMALISE"), (_lib.CIP_ASYNC, "CIP_ASYNC"),
                       (_lib.CIP_ASYNC | _lib.CIP_PIPELINE, "CIP_PIPELINE")):
        rc = _raw_call(tu, tf, ti, out, px, flags=flag)
        assert rc == _lib.CIP_EINVAL
        with pytest.raises(ValueError, match=word):
            _lib.check(rc)
    assert torch.count_nonzero(out) == 0  # nothing was launched
    assert _raw_call(tu, tf, ti, out, px, flags=1 << 20) == _lib.CIP_EINVAL


def test_python_validation_before_any_launch(gpu_device, base):
    import torch

    uvw, f, img, px, _ = base
    tu, tf, ti = _t(uvw), _t(f), _t(img)
    bad = [
        dict(dirty=ti.to(torch.float32)),  # dtype
        dict(dirty=ti[0]),  # shape
        dict(dirty=ti.cpu()),  # host tensor
        dict(dirty=ti.t()[:, ::2]),  # not contiguous
        dict(out=torch.empty((3_000, 3), dtype=torch.complex128, device="cuda")),
        dict(out=torch.empty((3_000, 2), dtype=torch.float64, device="cuda")),
        dict(out=torch.empty((3_000, 2), dtype=torch.complex128)),
        dict(subtract=True),  # needs out
        dict(wgt=torch.ones((3_000, 2), dtype=torch.float16, device="cuda")),
        dict(wgt=torch.ones((3_000, 1), dtype=torch.float32, device="cuda")),
        dict(out_dtype=torch.float64),
    ]
    for kw in bad:
        args = dict(dirty=ti, wgt=None)
        args.update(kw)
        dirty, wgt = args.pop("dirty"), args.pop("wgt")
        with pytest.raises(ValueError):
            gridder.device_dirty2ms(tu, tf, dirty, wgt, px, px, support=8, **args)
