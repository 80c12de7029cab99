"""
Gain calibration on the GPU (`cip_cal_correlate`, `cip_cal_solve`,
`cip_cal_apply`, `cip_gaincal`, `calibrate.py`) against the numpy statement of
include/cip_cal.h (`_cal_np`): correlations, counts, gains, flags, iteration
counts, the info struct and the applied data are compared bit for bit.

Correlate cases: 8 antennas x 6 dumps (168 rows), 2 intervals, nchan 1, 3, 4, 7
(partial runs), 64 (16 lanes x 4 channels, 16-byte loads) and 130 (a lane takes
more than one run); 2017 x 5 crosses workgroups with an odd row count and
16501 x 130 has more row blocks than the launch has workgroups. Every
case holds 5 % zero weights (some under NaN data), rows with ant1 > ant2, an
autocorrelation, antenna and interval indices out of range, a negative and a
NaN weight, an infinite visibility, a weight above wmax and a sample above
amax.
"""

import numpy as np
import pytest

import _cal_np as cnp
from ska_sdp_cip_amd import _lib, calibrate, synthetic

pytestmark = pytest.mark.gpu

N_ANT, N_INT = 8, 2
AMAX, WMAX = 4.5, 1.5
C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64


def _t(a, dev="cuda:0"):
    import torch

    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the cases' arrays are read-only


def _same(a, b):
    """Equal bits; a NaN matches a NaN in the same place (its sign and payload are not part of the definition)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind in "fc":
        real = a.real.dtype  # complex arrays compare as (re, im) pairs
        a, b = a.view(real).copy(), b.view(real).copy()
        if not np.array_equal(np.isnan(a), np.isnan(b)):
            return False
        a[np.isnan(a)] = b[np.isnan(b)] = 0.0
    view = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]
    return np.array_equal(a.view(view), b.view(view))


def _scale(ref):
    return _lib.cal_scale(ref["n_ant"], ref["n_int"], ref["amax"], ref["wmax"], 1 << 20)


class Rows:
    """One chunk with its numpy correlations and counts (computed once, never modified)."""

    def __init__(self, nchan, vis_dtype=C64, model_dtype=C64, wgt_dtype=F32, n_dumps=6, n_rows=None, seed=3):
        rng = np.random.default_rng(seed + nchan)
        nbl = N_ANT * (N_ANT - 1) // 2
        n_rows = nbl * n_dumps if n_rows is None else n_rows
        n_dumps = -(-n_rows // nbl)
        a1, a2, t = synthetic.baseline_indices(n_rows, N_ANT)
        interval = calibrate.solution_intervals(t, -(-n_dumps // N_INT))
        shape = (n_rows, nchan)
        model = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(model_dtype)
        gains = synthetic.random_gains(N_INT, N_ANT, 0.2, 0.6, rng)
        vis = gains[interval, a1][:, None] * model.astype(C128) * np.conj(gains[interval, a2])[:, None]
        vis = (vis + 0.05 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))).astype(vis_dtype)
        wgt = rng.uniform(0.5, 1.5, shape).astype(wgt_dtype)
        for a in (vis, model):  # keep the random part well inside amax
            a[np.maximum(np.abs(a.real), np.abs(a.imag)) > 4.0] = 1.0
        zero = rng.random(shape) < 0.05
        wgt[zero] = 0.0
        vis[zero & (rng.random(shape) < 0.5)] = np.nan
        c = nchan - 1
        wgt[0, 0], vis[0, 0] = 0.0, np.nan + 0j          # a zero weight under NaN, whatever the draw
        a1[3], a2[3] = a2[3], a1[3]                       # folded rows
        a1[40], a2[40] = a2[40], a1[40]
        a1[n_rows - 1], a2[n_rows - 1] = a2[n_rows - 1], a1[n_rows - 1]
        a2[5] = a1[5]                                     # an autocorrelation
        a2[7] = N_ANT                                     # antenna out of range
        a1[9] = -1
        interval[11] = N_INT                              # interval out of range
        interval[13] = -1
        for r, k in ((23, c), (25, 0), (27, c), (29, 0)):  # finite, whatever the zero-weight draw put there
            vis[r, k] = model[r, k] = 0.5 - 1.5j
        wgt[15, c] = -0.75                                # bad samples
        wgt[17, 0] = np.nan
        wgt[19, c], vis[19, c] = 1.0, np.inf + 0j
        wgt[21, 0], model[21, 0] = 1.0, 1j * np.nan
        wgt[23, c] = 2.0                                  # above wmax
        wgt[25, 0], vis[25, 0] = 1.0, 1.0 - 7.0j          # above amax
        wgt[27, c], model[27, c] = 1.0, -5.0 + 0j
        wgt[29, 0], wgt[31, c] = WMAX, -0.0               # on the bound: added; -0: a zero weight
        self.vis, self.model, self.wgt = vis, model, wgt
        self.cols = (a1, a2, interval)
        self.ref = cnp.scale_init(N_ANT, N_INT, AMAX, WMAX, 1 << 20)
        self.corr, self.counts = cnp.correlate(vis, model, wgt, a1, a2, interval, self.ref)
        for a in (vis, model, wgt, a1, a2, interval, self.corr):
            a.setflags(write=False)
        assert self.counts["n_bad"] == 4 and self.counts["n_zero"] >= 2
        assert self.counts["n_outside"] == 3 + 5 * nchan and self.counts["n_added"] > 0.8 * n_rows * nchan
        assert sum(self.counts.values()) == n_rows * nchan
        assert not self.corr[:, np.tril_indices(N_ANT)[0], np.tril_indices(N_ANT)[1]].any()  # p < q only

    def device(self, sel=slice(None), offset=()):
        """The chunk's tensors; the arrays named in `offset` start one element into their storage."""
        import torch

        out = []
        for name, a in (("vis", self.vis), ("model", self.model), ("wgt", self.wgt)):
            a = np.ascontiguousarray(a[sel])
            if name in offset:
                flat = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:1].copy()).dtype, device="cuda:0")
                flat[1:] = _t(a).reshape(-1)
                out.append(flat[1:].view(a.shape))
                assert out[-1].data_ptr() % 16 != 0 or a.dtype.itemsize == 16
            else:
                out.append(_t(a))
        return (*out, *[_t(np.ascontiguousarray(c[sel])) for c in self.cols])


_CASES = {}


def rows(*key, **kw):
    if (key, tuple(kw.items())) not in _CASES:
        _CASES[(key, tuple(kw.items()))] = Rows(*key, **kw)
    return _CASES[(key, tuple(kw.items()))]


def check_correlate(case, offset=()):
    import torch

    scale = _scale(case.ref)
    assert (scale.shift, scale.quantum) == (case.ref["shift"], case.ref["quantum"])
    corr, counts = calibrate.device_gain_correlate(*case.device(offset=offset), scale)
    assert corr.dtype == torch.int64 and tuple(corr.shape) == case.corr.shape
    assert counts == case.counts
    assert _same(corr.cpu().numpy(), case.corr)
    # two half calls into one array, and the sum of two separately accumulated arrays
    n = len(case.cols[0])
    halves = (slice(0, n // 2 + 1), slice(n // 2 + 1, n))
    one, total = None, {}
    parts = []
    for sel in halves:
        one, c = calibrate.device_gain_correlate(*case.device(sel, offset), scale, one)
        part, c2 = calibrate.device_gain_correlate(*case.device(sel, offset), scale)
        assert c == c2
        parts.append(part)
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    assert total == case.counts
    assert _same(one.cpu().numpy(), case.corr) and _same((parts[0] + parts[1]).cpu().numpy(), case.corr)


# ---- correlate ------------------------------------------------------------------
@pytest.mark.parametrize("nchan", [1, 3, 4, 7, 64, 130])
def test_correlate_channel_counts(gpu_device, nchan):
    check_correlate(rows(nchan))


@pytest.mark.parametrize("wgt_dtype", [F32, F64])
@pytest.mark.parametrize("model_dtype", [C64, C128])
@pytest.mark.parametrize("vis_dtype", [C64, C128])
def test_correlate_every_dtype_combination(gpu_device, vis_dtype, model_dtype, wgt_dtype):
    check_correlate(rows(7, vis_dtype=vis_dtype, model_dtype=model_dtype, wgt_dtype=wgt_dtype))


@pytest.mark.parametrize("vis_dtype, wgt_dtype", [(C64, F32), (C128, F64)])
def test_correlate_vector_loads_of_every_dtype(gpu_device, vis_dtype, wgt_dtype):
    check_correlate(rows(8, vis_dtype=vis_dtype, model_dtype=vis_dtype, wgt_dtype=wgt_dtype))


def test_correlate_odd_row_count_across_workgroups(gpu_device):
    check_correlate(rows(5, n_rows=2017))  # 2 lanes per row: 128 rows per workgroup, 16 workgroups


def test_correlate_more_row_blocks_than_workgroups(gpu_device):
    # 64 lanes per row, 4 rows per row block: 4126 row blocks on the launch's 4096 workgroups, so the first
    # 30 workgroups take a second block
    check_correlate(rows(130, n_rows=16501))


@pytest.mark.parametrize("nchan", [4, 64])
@pytest.mark.parametrize("offset", [("vis", "model", "wgt"), ("vis",), ("wgt",)])
def test_correlate_offset_base_pointer(gpu_device, nchan, offset):
    check_correlate(rows(nchan), offset)  # a slice starting at element 1: no 16-byte loads


def test_gain_correlator_accumulates_chunks(gpu_device):
    case = rows(7)
    gc = calibrate.GainCorrelator(N_ANT, N_INT, AMAX, WMAX, 1 << 20, gpu_device)
    n = len(case.cols[0])
    for sel in (slice(0, 50), slice(50, 51), slice(51, n)):
        gc.add_ms(*case.device(sel))
    assert gc.counts == case.counts and _same(gc.corr.cpu().numpy(), case.corr)
    ref = cnp.solve(case.corr, case.ref, 50, 1e-8, 0)
    got = gc.solve(niter=50, tol=1e-8, refant=0)
    assert _same(got[0].cpu().numpy(), ref[0]) and got[3] == ref[3]


# ---- solve -------------------------------------------------------------------
class Solvable:
    """Noise-free correlations of `n_ant` antennas and `n_int` intervals (one dump each); antenna `dead` has
    no weight in interval `n_int - 1`."""

    def __init__(self, n_ant, n_int, dead=None):
        rng = np.random.default_rng(100 * n_ant + n_int)
        nbl = n_ant * (n_ant - 1) // 2
        a1, a2, t = synthetic.baseline_indices(nbl * n_int, n_ant)
        model = rng.standard_normal((len(a1), 2)) + 1j * rng.standard_normal((len(a1), 2))
        self.truth = synthetic.random_gains(n_int, n_ant, 0.2, 0.6, rng)
        vis = self.truth[t, a1][:, None] * model * np.conj(self.truth[t, a2])[:, None]
        wgt = rng.uniform(0.5, 1.5, vis.shape)
        if dead is not None:
            wgt[(t == n_int - 1) & ((a1 == dead) | (a2 == dead))] = 0.0
        amax, wmax = cnp.sample_max(vis, model, wgt, a1, a2, t, n_ant, n_int)
        self.nsamp = vis.size
        self.ref = cnp.scale_init(n_ant, n_int, amax, wmax, self.nsamp)
        self.corr, _ = cnp.correlate(vis, model, wgt, a1, a2, t, self.ref)
        self.corr.setflags(write=False)
        self.n_ant, self.n_int, self.dead = n_ant, n_int, dead


def solvable(*key):
    if ("solve", key) not in _CASES:
        _CASES[("solve", key)] = Solvable(*key)
    return _CASES[("solve", key)]


def check_solve(case, niter=50, tol=1e-8, refant=0, phase_only=False, gains=None):
    scale = _lib.cal_scale(case.n_ant, case.n_int, case.ref["amax"], case.ref["wmax"], case.nsamp)
    assert (scale.shift, scale.quantum) == (case.ref["shift"], case.ref["quantum"])
    ref = cnp.solve(case.corr, case.ref, niter, tol, refant, phase_only, gains)
    start = None if gains is None else _t(gains)
    got = calibrate.device_gain_solve(_t(case.corr), scale, niter=niter, tol=tol, refant=refant,
                                      phase_only=phase_only, gains=start)
    g, ok, iters, info = got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy(), got[3]
    assert _same(ok, ref[1]) and _same(iters, ref[2])
    assert info == ref[3] and _same(np.float64(info["max_change"]), np.float64(ref[3]["max_change"]))
    assert _same(g, ref[0])
    if start is not None:
        assert _same(start.cpu().numpy(), np.asarray(gains))  # the start gains are not modified
    return g, ok, iters, info


@pytest.mark.parametrize("phase_only", [False, True])
@pytest.mark.parametrize("n_int", [1, 3])
@pytest.mark.parametrize("n_ant", [2, 3, 5, 8, 64, 65])
def test_solve_sizes(gpu_device, n_ant, n_int, phase_only):
    case = solvable(n_ant, n_int)
    g, ok, iters, info = check_solve(case, phase_only=phase_only)
    assert ok.all() and info["n_dead"] == 0
    if n_ant >= 8 and not phase_only:  # enough baselines per antenna to converge within 50 iterations
        assert info["n_converged"] == n_int and np.abs(g - cnp.rotate_to(case.truth)).max() < 1e-6


@pytest.mark.parametrize("phase_only", [False, True])
@pytest.mark.parametrize("refant", [-1, 0, "last"])
@pytest.mark.parametrize("n_ant", [8, 65])
def test_solve_reference_antenna(gpu_device, n_ant, refant, phase_only):
    refant = n_ant - 1 if refant == "last" else refant
    g, _, _, _ = check_solve(solvable(n_ant, 3), refant=refant, phase_only=phase_only)
    if refant >= 0:
        assert np.abs(g[:, refant].imag).max() < 1e-15 and np.all(g[:, refant].real > 0)


@pytest.mark.parametrize("phase_only", [False, True])
@pytest.mark.parametrize("niter, tol", [(0, 1e-8), (1, 1e-8), (2, 1e-8), (50, 1e-3), (50, 0.0), (7, 1e-300)])
def test_solve_iteration_limits(gpu_device, niter, tol, phase_only):
    case = solvable(8, 3)
    g, _, iters, info = check_solve(case, niter=niter, tol=tol, phase_only=phase_only)
    if niter == 0:
        assert _same(g, np.ones((3, 8), dtype=C128)) and info["max_iter_done"] == 0 and not iters.any()
    elif tol == 1e-3:
        assert 2 < iters.max() < 50 and info["n_converged"] == 3  # the tolerance stops the solve mid-way
    elif tol == 1e-300:
        assert np.all(iters == niter) and info["n_converged"] == 0


@pytest.mark.parametrize("phase_only", [False, True])
@pytest.mark.parametrize("n_ant, dead", [(8, 2), (65, 64), (5, 0)])
def test_solve_dead_antenna(gpu_device, n_ant, dead, phase_only):
    case = solvable(n_ant, 3, dead)
    rng = np.random.default_rng(1)
    start = synthetic.random_gains(3, n_ant, 0.3, 1.0, rng)  # a non-unit start: the dead gain keeps these bits
    for refant in (0 if dead else 1, dead):
        for niter in (0, 50):
            g, ok, _, info = check_solve(case, niter=niter, refant=refant, phase_only=phase_only, gains=start)
            assert info["n_dead"] == 1 and not ok[2, dead] and ok.sum() == ok.size - 1
            assert _same(g[2, dead], start[2, dead])
            assert info["ref_missing"] == (1 if refant == dead and niter else 0)


def test_solve_from_a_non_unit_start(gpu_device):
    case = solvable(8, 3)
    start = synthetic.random_gains(3, 8, 0.4, 2.0, np.random.default_rng(9)) * 1.7
    g, _, _, info = check_solve(case, gains=start)
    assert info["n_converged"] == 3 and np.abs(g - cnp.rotate_to(case.truth)).max() < 1e-6


# ---- apply -------------------------------------------------------------------
class Applied:
    def __init__(self, nchan, vis_dtype, wgt_dtype):
        base = rows(nchan, vis_dtype=vis_dtype, wgt_dtype=F32 if wgt_dtype is None else wgt_dtype)
        rng = np.random.default_rng(nchan)
        self.vis, self.wgt, self.cols = base.vis, (None if wgt_dtype is None else base.wgt), base.cols
        self.gains = synthetic.random_gains(N_INT, N_ANT, 0.3, 1.5, rng)
        self.ok = np.ones((N_INT, N_ANT), dtype=np.uint8)
        self.ok[1, 4] = 0  # a dead antenna
        self.ref = {m: cnp.apply(self.vis, self.wgt, *self.cols, self.gains, self.ok, m)
                    for m in ("correct", "corrupt")}


def check_apply(case, mode, inplace):
    vis, wgt = _t(case.vis), None if case.wgt is None else _t(case.wgt)
    cols = [_t(c) for c in case.cols]
    kw = dict(out=vis, wgt_out=wgt) if inplace else {}
    out, wout = calibrate.device_gain_apply(vis, wgt, *cols, _t(case.gains), _t(case.ok), mode=mode, **kw)
    ref_vis, ref_wgt = case.ref[mode]
    assert out.dtype == vis.dtype and _same(out.cpu().numpy(), ref_vis)
    assert (wout is None) == (wgt is None)
    if wgt is not None:
        assert wout.dtype == wgt.dtype and _same(wout.cpu().numpy(), ref_wgt)
    if inplace:
        assert out is vis and wout is wgt
    else:
        assert _same(vis.cpu().numpy(), case.vis)  # the inputs are not modified
    a1, a2, iv = case.cols
    dead = (iv == 1) & ((a1 == 4) | (a2 == 4))
    passed = dead | (iv < 0) | (iv >= N_INT) | (a1 < 0) | (a2 >= N_ANT)
    assert dead.sum() >= 7 and passed.sum() == dead.sum() + 4
    assert _same(out.cpu().numpy()[passed], case.vis[passed])
    if wgt is not None:
        assert not wout.cpu().numpy()[passed].any()


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("mode", ["correct", "corrupt"])
@pytest.mark.parametrize("wgt_dtype", [F32, F64, None])
@pytest.mark.parametrize("vis_dtype", [C64, C128])
def test_apply_every_dtype_pair(gpu_device, vis_dtype, wgt_dtype, mode, inplace):
    check_apply(Applied(7, vis_dtype, wgt_dtype), mode, inplace)


@pytest.mark.parametrize("mode", ["correct", "corrupt"])
@pytest.mark.parametrize("nchan", [1, 3, 4, 64, 130])
def test_apply_channel_counts(gpu_device, nchan, mode):
    check_apply(Applied(nchan, C64, F32), mode, nchan in (4, 130))


@pytest.mark.parametrize("vis_dtype, wgt_dtype", [(C64, F32), (C64, F64), (C128, F32), (C128, F64)])
def test_correct_undoes_corrupt(gpu_device, vis_dtype, wgt_dtype):
    import torch

    rng = np.random.default_rng(5)
    a1, a2, t = synthetic.baseline_indices(28 * 4, N_ANT)
    iv = calibrate.solution_intervals(t, 2)
    v = (rng.standard_normal((len(a1), 6)) + 1j * rng.standard_normal((len(a1), 6))).astype(vis_dtype)
    w = rng.uniform(0.5, 1.5, v.shape).astype(wgt_dtype)
    gains, ok = _t(synthetic.random_gains(2, N_ANT, 0.3, 3.0, rng)), torch.ones((2, N_ANT), dtype=torch.uint8,
                                                                                 device=gpu_device)
    cols = [_t(c) for c in (a1, a2, iv)]
    bad, wbad = calibrate.device_gain_apply(_t(v), _t(w), *cols, gains, ok, mode="corrupt")
    assert _same(wbad.cpu().numpy(), w)
    back, wback = calibrate.device_gain_apply(bad, wbad, *cols, gains, ok, mode="correct")
    # each pass is fp64 arithmetic of a few 2^-53 and one rounding of either component to the output dtype:
    # (0.5 sqrt(2) + 0.5) ulp of |v| for complex64, below 3.5 ulp of |v| for complex128
    eps = np.finfo(v.real.dtype).eps
    err = np.abs(back.cpu().numpy().astype(C128) - v.astype(C128)) / (eps * np.abs(v.astype(C128)))
    print(f"{np.dtype(vis_dtype).name}: correct(corrupt(v)) is within {err.max():.2f} ulp")
    assert err.max() <= 4.0
    h2 = np.abs(gains.cpu().numpy()[iv, a1] * np.conj(gains.cpu().numpy()[iv, a2])) ** 2
    assert np.allclose(wback.cpu().numpy(), w * h2[:, None], rtol=4 * np.finfo(wgt_dtype).eps, atol=0.0)


# ---- the one-shot call ---------------------------------------------------------------
@pytest.mark.parametrize("phase_only", [False, True])
@pytest.mark.parametrize("nchan, dtypes", [(7, (C64, C64, F32)), (64, (C64, C128, F64)), (3, (C128, C64, F32))])
def test_gaincal_equals_the_written_out_sequence(gpu_device, nchan, dtypes, phase_only):
    case = rows(nchan, vis_dtype=dtypes[0], model_dtype=dtypes[1], wgt_dtype=dtypes[2])
    dev = case.device()
    gains, ok, info = calibrate.device_gaincal(*dev, N_ANT, N_INT, niter=30, tol=1e-9, refant=1,
                                               phase_only=phase_only)
    # written out: the bounds (numpy), the scale, the correlate and the solve
    amax, wmax = cnp.sample_max(case.vis, case.model, case.wgt, *case.cols, N_ANT, N_INT)
    assert amax > AMAX and wmax == 2.0  # the one-shot call leaves no sample out for its size
    scale = _lib.cal_scale(N_ANT, N_INT, amax, wmax, case.vis.size)
    assert (info["amax"], info["wmax"], info["shift"], info["quantum"]) == (amax, wmax, scale.shift, scale.quantum)
    corr, counts = calibrate.device_gain_correlate(*dev, scale)
    g2, ok2, iters2, info2 = calibrate.device_gain_solve(corr, scale, niter=30, tol=1e-9, refant=1,
                                                         phase_only=phase_only)
    assert _same(gains.cpu().numpy(), g2.cpu().numpy()) and _same(ok.cpu().numpy(), ok2.cpu().numpy())
    assert _same(info["iters"].cpu().numpy(), iters2.cpu().numpy())
    for key, value in {**info2, **counts}.items():
        assert info[key] == value, key
    assert counts["n_outside"] == 5 * nchan and counts["n_bad"] == 4
    # and the numpy statement of the whole call
    ref = cnp.gaincal(case.vis, case.model, case.wgt, *case.cols, N_ANT, N_INT, niter=30, tol=1e-9, refant=1,
                      phase_only=phase_only)
    assert _same(gains.cpu().numpy(), ref[0]) and ref[5] == counts


def test_gaincal_recovers_noise_free_gains(gpu_device):
    from test_cal_host import noise_free_case

    vis, model, wgt, a1, a2, interval, truth = noise_free_case()
    gains, ok, info = calibrate.gaincal(vis, model, wgt, a1, a2, interval, 8, 2, niter=100, tol=1e-10, refant=0)
    assert isinstance(gains, np.ndarray) and gains.dtype == C128 and ok.all()
    err = np.abs(gains - cnp.rotate_to(truth)).max()
    print(f"gain error {err:.3g} after {info['iters'].tolist()} iterations")
    assert err <= 1e-6 and info["n_converged"] == 2 and info["iters"].max() <= 40
    ref = cnp.gaincal(vis, model, wgt, a1, a2, interval, 8, 2, niter=100, tol=1e-10, refant=0)
    assert _same(gains, ref[0]) and _same(info["iters"], ref[2])
    # gain_apply (numpy in, numpy out) with the solution takes the gains out of the data
    fixed, wfixed = calibrate.gain_apply(vis, wgt, a1, a2, interval, gains, ok)
    assert fixed.dtype == vis.dtype and wfixed.dtype == wgt.dtype
    assert np.abs(fixed - model).max() < 1e-5


def test_gaincal_without_a_sample(gpu_device):
    import torch

    case = rows(3)
    vis, model, wgt, a1, a2, iv = case.device()
    gains, ok, info = calibrate.device_gaincal(vis, model, torch.zeros_like(wgt), a1, a2, iv, N_ANT, N_INT)
    assert not ok.any() and info["n_dead"] == N_ANT * N_INT and info["n_added"] == 0
    assert (info["amax"], info["wmax"]) == (1.0, 1.0) and info["ref_missing"] == N_INT
    assert _same(gains.cpu().numpy(), np.ones((N_INT, N_ANT), dtype=C128))
