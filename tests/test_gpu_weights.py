"""
Imaging weights on the GPU (`cip_weight_density`, `cip_weight_stats`,
`cip_weight_apply`, `cip_imaging_weights`, `weighting.py`) against the numpy
statement of the operator (`_weights_np`): the density, the counts and the
weights are compared bit for bit, no sample excluded.

Base case: 64 x 48 pixels (non-square: a swapped axis shows), 300 rows x 37
channels (37 = 16 + 16 + 5: whole and partial lane segments, rows that start
16-byte aligned and rows that do not), float32 weights, with negative v, rows
with v == 0, zero weights, about 5 % of the samples outside the grid and one
cell holding more than 5000 samples. Exact case: freq = c m and dyadic u, v,
so x and y are exact and sit on n + 0.5 boundaries and on the grid's edge.
"""

import ctypes
import math

import numpy as np
import pytest

import _weights_np as wnp
from ska_sdp_cip_amd import _lib, deconvolve, weighting

pytestmark = pytest.mark.gpu

C = 299792458.0
MODES = {"uniform": wnp.UNIFORM, "briggs": wnp.BRIGGS}


def _t(a, dev="cuda:0"):
    import torch

    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the cases' arrays are read-only


class Case:
    """One data set with its numpy density, counts and statistics (computed once, never modified)."""

    def __init__(self, npix, pix, uvw, freq, wgt, wmax):
        self.npix, self.pix = npix, pix
        self.uvw, self.freq, self.wgt = uvw, freq, wgt
        self.nvis = uvw.shape[0] * freq.shape[0]
        self.ref = wnp.Grid(*npix, *pix, wmax, self.nvis)
        self.grid = _lib.weight_grid(*npix, *pix, wmax, self.nvis)
        self.dens, self.counts = wnp.density(uvw, freq, wgt, self.ref)
        self.stats = wnp.stats(self.dens, self.ref)
        for a in (self.uvw, self.freq, self.wgt, self.dens, self.counts):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def base():
    rng = np.random.default_rng(20240)
    nrow, nchan = 300, 37
    freq = np.linspace(1.0e9, 1.3e9, nchan)
    uvw = np.zeros((nrow, 3))
    uvw[:, 0] = rng.uniform(-142.0, 142.0, nrow)
    uvw[:, 1] = rng.uniform(-97.0, 97.0, nrow)
    uvw[:, 2] = rng.uniform(-10.0, 10.0, nrow)
    uvw[:10, 1] = 0.0                       # v == 0, u of both signs
    uvw[10:12, 1] = -0.0
    uvw[20:160, 0] = rng.uniform(-0.9, 0.9, 140)   # 140 rows x 37 channels in cell (0, 0)
    uvw[20:160, 1] = rng.uniform(-0.9, 0.9, 140)
    wgt = rng.uniform(0.1, 2.0, (nrow, nchan)).astype(np.float32)
    wgt[rng.uniform(size=wgt.shape) < 0.1] = 0.0
    wgt[5, 3] = -0.0
    case = Case((64, 48), (1.0e-3, 1.5e-3), uvw, freq, wgt, 2.0)
    # the inputs are what the docstring says
    assert (uvw[:, 1] < 0).sum() > 50 and (wgt == 0).sum() > 500
    assert case.dens[case.ref.hx, 0] >= 5000 * wnp.quantise(np.float64(0.1), case.ref)
    _, _, inside = wnp.cells(uvw, freq, case.ref)
    assert ((wgt[20:160] > 0) & inside[20:160]).sum() > 4500 and inside[20:160].all()
    assert 0.02 < case.counts[1] / case.nvis < 0.10 and case.counts[2] == 0
    return case


@pytest.fixture(scope="module")
def exact():
    rng = np.random.default_rng(7)
    nrow = 200
    freq = C * np.array([1.0, 2.0, 3.0])
    # SX = SY = 1 / 16: x = m a, y = m b for u = 16 a, v = 16 b; a, b multiples of 1 / 4
    a = rng.integers(-4 * 33, 4 * 33 + 1, nrow) / 4.0
    b = rng.integers(-4 * 17, 4 * 17 + 1, nrow) / 4.0
    a[:8] = [32.0, -32.0, 31.5, -32.5, 32.5, 10.5, -10.5, 16.0]   # the edge, half cells, m a = 32 at m = 2
    b[:8] = [16.0, -16.0, 15.5, 16.5, 0.0, 0.0, -0.0, 8.0]
    uvw = np.stack([16.0 * a, 16.0 * b, np.zeros(nrow)], 1)
    wgt = rng.integers(1, 9, (nrow, 3)).astype(np.float64) / 8.0
    case = Case((64, 32), (2.0 ** -10, 2.0 ** -9), uvw, freq, wgt, 1.0)
    assert case.ref.SX == 1 / 16 and case.ref.SY == 1 / 16
    return case


def _density(case, uvw, wgt, dens_t, grid=None):
    """cip_weight_density of the rows given onto dens_t; returns (rc, counts)."""
    import torch

    u, f = _t(uvw), _t(case.freq)
    w = None if wgt is None else _t(wgt)
    code = _lib.CIP_NONE if wgt is None else {np.float32: _lib.CIP_F32, np.float64: _lib.CIP_F64}[wgt.dtype.type]
    counts = (ctypes.c_int64 * 3)(-1, -1, -1)
    rc = _lib.lib().cip_weight_density(u.data_ptr(), u.shape[0], f.data_ptr(), f.shape[0],
                                       None if w is None else w.data_ptr(), code,
                                       ctypes.byref(grid or case.grid), None, dens_t.data_ptr(), counts)
    torch.cuda.synchronize()
    return rc, list(counts)


def _zeros(case):
    import torch

    return torch.zeros(case.grid.density_shape, dtype=torch.int64, device="cuda:0")


@pytest.mark.parametrize("name", ["base", "exact"])
def test_density_and_counts_equal_numpy(name, request):
    case = request.getfixturevalue(name)
    dens = _zeros(case)
    rc, counts = _density(case, case.uvw, case.wgt, dens)
    assert rc == _lib.CIP_OK
    assert counts == case.counts.tolist()
    assert case.grid.shift == case.ref.shift and tuple(dens.shape) == case.ref.shape
    assert np.array_equal(dens.cpu().numpy(), case.dens)


def test_density_without_weights_counts_samples(base):
    grid = _lib.weight_grid(*base.npix, *base.pix, 1.0, base.nvis)
    ref = wnp.Grid(*base.npix, *base.pix, 1.0, base.nvis)
    dens = _zeros(base)
    rc, counts = _density(base, base.uvw, None, dens, grid)
    want, want_counts = wnp.density(base.uvw, base.freq, None, ref)
    assert rc == _lib.CIP_OK and counts == want_counts.tolist()
    assert np.array_equal(dens.cpu().numpy(), want)


def test_chunks_in_any_order_and_summed_halves(base):
    import torch

    cuts = [(0, 97), (97, 230), (230, 300)]
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        dens = _zeros(base)
        total = np.zeros(3, dtype=np.int64)
        for k in order:
            a, b = cuts[k]
            rc, counts = _density(base, base.uvw[a:b], base.wgt[a:b], dens)
            assert rc == _lib.CIP_OK
            total += counts
        assert np.array_equal(dens.cpu().numpy(), base.dens), order
        assert total.tolist() == base.counts.tolist()
    # two "ranks", each with half of the rows, summed as an all-reduce would
    halves = []
    for a, b in ((0, 150), (150, 300)):
        dens = _zeros(base)
        assert _density(base, base.uvw[a:b], base.wgt[a:b], dens)[0] == _lib.CIP_OK
        halves.append(dens)
    assert np.array_equal(torch.add(halves[0], halves[1]).cpu().numpy(), base.dens)


@pytest.mark.parametrize("name", ["base", "exact"])
def test_stats(name, request):
    case = request.getfixturevalue(name)
    dens = _t(case.dens)
    out = (ctypes.c_double * 3)()
    assert _lib.lib().cip_weight_stats(dens.data_ptr(), ctypes.byref(case.grid), None, out) == _lib.CIP_OK
    sum_w, sum_d2, n_cells = case.stats
    print(f"{name}: sum_w {out[0]!r} (numpy {sum_w!r}), sum_d2 {out[1]!r} (fsum {sum_d2!r}), cells {out[2]}")
    assert out[0] == sum_w          # an exact integer sum: bit-equal
    assert out[2] == n_cells
    # any summation order of non-negative terms stays within (terms) 2^-52 relative of the exact sum
    assert abs(out[1] - sum_d2) <= case.dens.size * 2.0 ** -52 * sum_d2
    again = (ctypes.c_double * 3)()
    assert _lib.lib().cip_weight_stats(dens.data_ptr(), ctypes.byref(case.grid), None, again) == _lib.CIP_OK
    assert list(again) == list(out)


def _apply(case, wgt, mode, f2, out_dtype, inplace=False):
    import torch

    u, f, dens = _t(case.uvw), _t(case.freq), _t(case.dens)
    w = None if wgt is None else _t(wgt)
    codes = {np.float32: _lib.CIP_F32, np.float64: _lib.CIP_F64}
    out = w if inplace else torch.full(case.wgt.shape, -7.0, dtype=getattr(torch, np.dtype(out_dtype).name),
                                       device="cuda:0")
    rc = _lib.lib().cip_weight_apply(u.data_ptr(), u.shape[0], f.data_ptr(), f.shape[0],
                                     None if w is None else w.data_ptr(),
                                     _lib.CIP_NONE if w is None else codes[wgt.dtype.type], dens.data_ptr(),
                                     ctypes.byref(case.grid), mode, f2, None, out.data_ptr(), codes[out_dtype])
    assert rc == _lib.CIP_OK, _lib.lib().cip_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64),
                                                 b.view(np.uint32 if b.dtype == np.float32 else np.uint64))


@pytest.mark.parametrize("name", ["base", "exact"])
@pytest.mark.parametrize("mode", ["uniform", "briggs"])
def test_apply_equals_numpy_bit_for_bit(name, mode, request):
    case = request.getfixturevalue(name)
    f2 = wnp.briggs_f2(-0.5, case.stats[0], case.stats[1]) if mode == "briggs" else 0.0
    for in_dtype in (np.float32, np.float64):
        wgt = case.wgt.astype(in_dtype)
        for out_dtype in (np.float32, np.float64):
            want = wnp.apply(case.uvw, case.freq, wgt, case.dens, case.ref, MODES[mode], f2, out_dtype)
            got = _apply(case, wgt, MODES[mode], f2, out_dtype)
            assert _same_bits(got, want), (in_dtype, out_dtype)
        want = wnp.apply(case.uvw, case.freq, wgt, case.dens, case.ref, MODES[mode], f2, in_dtype)
        assert _same_bits(_apply(case, wgt, MODES[mode], f2, in_dtype, inplace=True), want), ("in place", in_dtype)
    for out_dtype in (np.float32, np.float64):  # wgt == NULL: unit weights against the same density
        want = wnp.apply(case.uvw, case.freq, None, case.dens, case.ref, MODES[mode], f2, out_dtype)
        assert _same_bits(_apply(case, None, MODES[mode], f2, out_dtype), want), ("no weights", out_dtype)


def _one_shot_reference(case, wgt, mode, robust, info, out_dtype):
    """numpy's weights for the one-shot call (wmax = the largest weight), evaluated with the returned f2."""
    ref = wnp.Grid(*case.npix, *case.pix, float(np.max(wgt)), case.nvis)
    dens, counts = wnp.density(case.uvw, case.freq, wgt, ref)
    sum_w, sum_d2, n_cells = wnp.stats(dens, ref)
    assert info["quantum"] == ref.quantum
    assert (info["n_added"], info["n_outside"], info["n_cells"]) == (counts[0], counts[1], n_cells)
    assert info["sum_w"] == sum_w
    assert abs(info["sum_d2"] - sum_d2) <= dens.size * 2.0 ** -52 * sum_d2
    if mode == "briggs":
        # the returned sums in the header's formula; pow is the one step libm may round differently
        f2 = wnp.briggs_f2(robust, info["sum_w"], info["sum_d2"])
        assert abs(info["f2"] - f2) <= 4 * np.spacing(f2)
    else:
        assert info["f2"] == 0.0
    return wnp.apply(case.uvw, case.freq, wgt, dens, ref, MODES[mode], info["f2"], out_dtype), n_cells


@pytest.mark.parametrize("mode", ["uniform", "briggs"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_shot(base, mode, dtype):
    import torch

    wgt = base.wgt.astype(dtype)
    u, f, w = _t(base.uvw), _t(base.freq), _t(wgt)
    out, info = weighting.device_imaging_weights(u, f, w, *base.npix, *base.pix, weighting=mode, robust=0.5)
    want, n_cells = _one_shot_reference(base, wgt, mode, 0.5, info, dtype)
    assert _same_bits(out.cpu().numpy(), want)
    assert torch.equal(w, _t(wgt))  # the input is not modified
    out2, info2 = weighting.device_imaging_weights(u, f, w, *base.npix, *base.pix, weighting=mode, robust=0.5)
    assert torch.equal(out, out2) and info == info2  # identical calls, identical bits
    if mode == "uniform":
        # every non-empty cell's weights sum to 1
        total = float(out.to(torch.float64).sum())
        print(f"uniform {np.dtype(dtype).name}: sum of weights {total!r}, non-zero cells {n_cells}")
        assert abs(total - n_cells) <= (1e-6 if dtype == np.float32 else 1e-12) * n_cells
    # numpy in, numpy out
    out_np, info_np = weighting.imaging_weights(base.uvw.copy(), base.freq.copy(), wgt, *base.npix, *base.pix, weighting=mode,
                                                robust=0.5)
    assert isinstance(out_np, np.ndarray) and _same_bits(out_np, want) and info_np == info


def test_bad_weights_are_erange(base):
    for bad in (-1.0, math.nan, 2.5):  # negative, NaN, above the grid's wmax = 2
        wgt = base.wgt.copy()
        wgt[123, 20] = bad
        rc, counts = _density(base, base.uvw, wgt, _zeros(base))
        assert rc == _lib.CIP_ERANGE and counts[2] == 1, bad
        assert b"cip_weight_density" in _lib.lib().cip_last_error()
    for bad in (-1.0, math.nan, math.inf):
        wgt = base.wgt.copy()
        wgt[123, 20] = bad
        with pytest.raises(ValueError, match="cip_imaging_weights"):
            weighting.device_imaging_weights(_t(base.uvw), _t(base.freq), _t(wgt), *base.npix, *base.pix)


def test_empty_zero_odd_and_workspace_reuse(base):
    import torch

    f = _t(base.freq)
    # nrow == 0
    out, info = weighting.device_imaging_weights(torch.zeros((0, 3), dtype=torch.float64, device="cuda:0"), f,
                                                 torch.zeros((0, 37), dtype=torch.float32, device="cuda:0"),
                                                 *base.npix, *base.pix)
    assert tuple(out.shape) == (0, 37) and info["n_added"] == 0
    # all-zero weights: all-zero output, no error
    u = _t(base.uvw)
    out, info = weighting.device_imaging_weights(u, f, torch.zeros((300, 37), dtype=torch.float32, device="cuda:0"),
                                                 *base.npix, *base.pix, weighting="uniform")
    assert not out.any() and info["sum_w"] == 0.0 and info["n_cells"] == 0
    # odd npix, after the workspace was released, then two grid shapes in turn through one workspace
    assert _lib.lib().cip_release_workspace() == _lib.CIP_OK
    shapes = [((33, 17), (2.0e-3, 4.0e-3)), (base.npix, base.pix), ((33, 17), (2.0e-3, 4.0e-3)),
              (base.npix, base.pix)]
    w = _t(base.wgt)
    seen = {}
    for npix, pix in shapes:
        out, info = weighting.device_imaging_weights(u, f, w, *npix, *pix, weighting="briggs", robust=0.0)
        case = Case(npix, pix, base.uvw, base.freq, base.wgt, 2.0)
        want, _ = _one_shot_reference(case, base.wgt, "briggs", 0.0, info, np.float32)
        assert _same_bits(out.cpu().numpy(), want), npix
        if npix in seen:
            assert torch.equal(seen[npix], out)
        seen[npix] = out


def test_weight_density_class_matches_one_shot(base):
    import torch

    u, f, w = _t(base.uvw), _t(base.freq), _t(base.wgt)
    one, info = weighting.device_imaging_weights(u, f, w, *base.npix, *base.pix, weighting="briggs", robust=-1.0)
    wd = weighting.WeightDensity(*base.npix, *base.pix, float(base.wgt.max()), base.nvis, "cuda:0")
    for a, b in ((200, 300), (0, 200)):
        wd.add_ms(u[a:b], f, w[a:b])
    with pytest.raises(RuntimeError, match="finish"):
        wd.apply(u, f, w)
    stats = wd.finish("briggs", robust=-1.0)
    assert {k: stats[k] for k in info} == info
    parts = [wd.apply(u[a:b], f, w[a:b]) for a, b in ((0, 120), (120, 300))]
    assert torch.equal(torch.cat(parts), one)
    inplace = w.clone()
    assert wd.apply(u, f, inplace, out=inplace) is inplace and torch.equal(inplace, one)


def test_two_ranks_all_reduce_to_the_same_density(base, monkeypatch):
    """Two ranks (host threads on one GPU, each on its own stream and workspace) hold half of the rows
    each; after `all_reduce` both hold numpy's density, and their weights are the one-shot call's rows."""
    import torch

    from _thread_dist import run_ranks

    wmax = float(base.wgt.max())
    halves = ((0, 150), (150, 300))

    def rank(r):
        a, b = halves[r]
        u, f, w = _t(base.uvw[a:b]), _t(base.freq), _t(base.wgt[a:b])
        wd = weighting.WeightDensity(*base.npix, *base.pix, wmax, base.nvis, "cuda:0")
        wd.add_ms(u, f, w)
        wd.all_reduce()
        stats = wd.finish("briggs", robust=0.0)
        return wd.density.clone(), wd.apply(u, f, w), stats

    results, errors = run_ranks(monkeypatch, 2, rank)
    assert not errors, errors
    assert run_ranks.last.calls == [1, 1]
    ref = wnp.Grid(*base.npix, *base.pix, wmax, base.nvis)
    dens, _ = wnp.density(base.uvw, base.freq, base.wgt, ref)
    for density, _, stats in results:
        assert np.array_equal(density.cpu().numpy(), dens)
        assert {k: v for k, v in stats.items() if not k.startswith("n_")} == \
            {k: v for k, v in results[0][2].items() if not k.startswith("n_")}
    one, info = weighting.device_imaging_weights(_t(base.uvw), _t(base.freq), _t(base.wgt), *base.npix, *base.pix,
                                                 weighting="briggs", robust=0.0)
    assert results[0][2]["f2"] == info["f2"] and results[0][2]["n_cells"] == info["n_cells"]
    assert torch.equal(torch.cat([results[0][1], results[1][1]]), one)


def test_major_cycles_with_uniform_weighting():
    import torch

    from ska_sdp_cip_amd import synthetic as syn
    from ska_sdp_cip_amd.invert import StokesIGridderInput

    ms = syn.make_measurement_set(2_000, 8, n_ant=16, array_radius_m=1000.0, seed=11)
    gi = StokesIGridderInput.from_measurement_set_reader(ms)
    npix = 128
    pix = syn.pixel_size_for_grid(gi.uvw, gi.channel_frequencies, npix)
    u, f = _t(gi.uvw), _t(gi.channel_frequencies)
    vis, w = _t(gi.visibilities), _t(gi.effective_weights().astype(np.float32))
    assert tuple(vis.shape) == (2000, 8)
    kw = dict(n_major=2, niter=50, do_wstacking=False)
    got = deconvolve.device_major_cycles(u, f, vis, w, npix, pix, weighting="uniform", **kw)
    wu, _ = weighting.device_imaging_weights(u, f, w, npix, npix, pix, pix, weighting="uniform")
    assert not torch.equal(wu, w)
    want = deconvolve.device_major_cycles(u, f, vis, wu, npix, pix, weighting="natural", **kw)
    plain = deconvolve.device_major_cycles(u, f, vis, wu, npix, pix, **kw)
    for key in ("model", "residual", "psf"):
        assert torch.equal(got[key], want[key]), key
        assert torch.equal(plain[key], want[key]), key
    assert got["components"] == want["components"] == plain["components"] and sum(got["components"]) > 0
    # and the default is natural weighting: other weights, another image
    natural = deconvolve.device_major_cycles(u, f, vis, w, npix, pix, **kw)
    assert not torch.equal(natural["psf"], got["psf"])
