"""
Antenna gain self-calibration on the GPU: StEFCal (`cip_gaincal` and the
`cip_cal_*` calls of libcip_hip.so) and the self-calibration loop that joins it
to the major cycles.

The operators are defined exactly in include/cip_cal.h. Gains are scalar, per
antenna and per solution interval, shared by all channels: `V_pq ~ g_p M_pq
conj(g_q)`. The data enter through one streaming pass (`cip_cal_correlate`)
that sums, per interval and baseline, the three terms w V conj(M) (re, im) and
w |M|^2 in 64-bit fixed point: integer adds, so the sums have the same bits
for any chunking, arrival order or number of ranks. The solve
(`cip_cal_solve`) and the apply (`cip_cal_apply`) are bit-identical to their
numpy statements.
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._call import (STREAM, VIS_DTYPES, WGT_DTYPES, call, check_array, require_gpu, target_device, to_device, vis_arg,
                    wgt_arg)
from .deconvolve import device_major_cycles
from .gridder import device_dirty2ms
from .invert import DO_WSTACKING, EPSILON
from .skymodel import device_dft_predict

try:
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None


def solution_intervals(time_index, dumps_per_interval: int):
    """
    The solution interval of every row: `time_index // dumps_per_interval` as
    int32 (numpy in -> numpy out, torch in -> torch out). `time_index` holds the
    rows' non-negative dump numbers (`synthetic.baseline_indices`).
    """
    dumps = int(dumps_per_interval)
    if dumps < 1:
        raise ValueError("dumps_per_interval must be >= 1")
    if torch is not None and torch.is_tensor(time_index):
        if time_index.numel() and int(time_index.min()) < 0:
            raise ValueError("time_index must be >= 0")
        return torch.div(time_index, dumps, rounding_mode="floor").to(torch.int32)
    t = np.asarray(time_index)
    if t.size and t.min() < 0:
        raise ValueError("time_index must be >= 0")
    return (t // dumps).astype(np.int32)


def _check_rows(vis, ant1, ant2, interval, what):
    """vis (nrow, nchan) complex and the three int32 row columns on its device; returns (nrow, nchan)."""
    if vis.dim() != 2:
        raise ValueError(f"{what}: vis must have shape (nrow, nchan)")
    nrow, nchan = int(vis.shape[0]), int(vis.shape[1])
    check_array(vis, VIS_DTYPES, None, vis.device, "vis")
    for name, col in (("ant1", ant1), ("ant2", ant2), ("interval", interval)):
        check_array(col, (torch.int32,), (nrow,), vis.device, name)
    return nrow, nchan


def _check_columns(vis, model, wgt, ant1, ant2, interval, what):
    nrow, nchan = _check_rows(vis, ant1, ant2, interval, what)
    check_array(model, VIS_DTYPES, (nrow, nchan), vis.device, "model")
    check_array(wgt, WGT_DTYPES, (nrow, nchan), vis.device, "wgt")
    return nrow, nchan


def _flags(phase_only: bool) -> int:
    return _lib.CAL_PHASE_ONLY if phase_only else 0


def _gains_io(gains, n_int, n_ant, device):
    """The (n_int, n_ant) complex128 start gains on `device`: a copy of `gains`, ones without."""
    if gains is None:
        return torch.ones((n_int, n_ant), dtype=torch.complex128, device=device)
    check_array(gains, (torch.complex128,), (n_int, n_ant), device, "gains")
    return gains.clone()


def device_gain_correlate(vis, model, wgt, ant1, ant2, interval, scale: "_lib.CalScale", corr=None):
    """
    `cip_cal_correlate` on device tensors: adds the chunk's fixed-point sums to
    `corr` (int64 (n_int, n_ant, n_ant, 3), zeros when None; cells p < q only)
    under the scale `_lib.cal_scale(...)`. Returns (corr, counts) with
    `n_added`, `n_zero`, `n_outside`, `n_bad` of this call.
    """
    require_gpu()
    nrow, nchan = _check_columns(vis, model, wgt, ant1, ant2, interval, "device_gain_correlate")
    if corr is None:
        corr = torch.zeros(scale.corr_shape, dtype=torch.int64, device=vis.device)
    else:
        check_array(corr, (torch.int64,), scale.corr_shape, vis.device, "corr")
    counts = _lib.CalCounts()
    call(vis.device, "cip_cal_correlate", *vis_arg(vis), *vis_arg(model), *wgt_arg(wgt), nrow, nchan, ant1, ant2,
         interval, ctypes.byref(scale), STREAM, corr, ctypes.byref(counts))
    return corr, counts.as_dict()


def device_gain_solve(corr, scale: "_lib.CalScale", *, niter: int = 50, tol: float = 1e-8, refant: int = 0,
                      phase_only: bool = False, gains=None):
    """
    `cip_cal_solve`: StEFCal on the correlations `corr`, from `gains`
    (complex128 (n_int, n_ant), not modified; ones when None). `refant < 0`: no
    rotation to a reference antenna. Returns (gains, ant_ok uint8, iters int64
    (n_int), info) with `n_converged`, `n_dead`, `max_iter_done`,
    `ref_missing`, `max_change`.
    """
    require_gpu()
    dev = corr.device
    check_array(corr, (torch.int64,), scale.corr_shape, dev, "corr")
    n_int, n_ant = int(scale.n_int), int(scale.n_ant)
    out = _gains_io(gains, n_int, n_ant, dev)
    ant_ok = torch.empty((n_int, n_ant), dtype=torch.uint8, device=dev)
    iters = torch.empty(n_int, dtype=torch.int64, device=dev)
    info = _lib.CalSolveInfo()
    call(dev, "cip_cal_solve", corr, ctypes.byref(scale), int(niter), float(tol), int(refant), _flags(phase_only),
         STREAM, out, ant_ok, iters, ctypes.byref(info))
    return out, ant_ok, iters, info.as_dict()


def device_gain_apply(vis, wgt, ant1, ant2, interval, gains, ant_ok, *, mode: str = "correct", out=None,
                      wgt_out=None):
    """
    `cip_cal_apply`: `mode="correct"` divides the gains out of `vis`
    (v / (g_p conj(g_q))) and scales the weights by |g_p conj(g_q)|^2;
    "corrupt" multiplies them in and keeps the weights. `out` / `wgt_out`
    (the inputs' dtypes; may be the inputs themselves) receive the results,
    else new tensors. `wgt=None`: visibilities only. A row with a dead antenna
    or a bad index passes through with weight 0. Stream-ordered. Returns
    (vis_out, wgt_out).
    """
    require_gpu()
    if mode not in _lib.CAL_MODES:
        raise ValueError(f"mode must be one of {sorted(_lib.CAL_MODES)}, got {mode!r}")
    nrow, nchan = _check_rows(vis, ant1, ant2, interval, "device_gain_apply")
    dev = vis.device
    if gains.dim() != 2:
        raise ValueError("gains must be complex128 of shape (n_int, n_ant)")
    n_int, n_ant = int(gains.shape[0]), int(gains.shape[1])
    check_array(gains, (torch.complex128,), None, dev, "gains")
    check_array(ant_ok, (torch.uint8, torch.bool), (n_int, n_ant), dev, "ant_ok")
    if out is None:
        out = torch.empty_like(vis)
    else:
        check_array(out, (vis.dtype,), (nrow, nchan), dev, "out")
    if wgt is None:
        if wgt_out is not None:
            raise ValueError("wgt_out needs wgt")
    else:
        check_array(wgt, WGT_DTYPES, (nrow, nchan), dev, "wgt")
        if wgt_out is None:
            wgt_out = torch.empty_like(wgt)
        else:
            check_array(wgt_out, (wgt.dtype,), (nrow, nchan), dev, "wgt_out")
    call(dev, "cip_cal_apply", *vis_arg(vis), *wgt_arg(wgt), nrow, nchan, ant1, ant2, interval, gains,
         ant_ok.view(torch.uint8), n_int, n_ant, _lib.CAL_MODES[mode], STREAM, out, wgt_out)
    return out, wgt_out


def device_gaincal(vis, model, wgt, ant1, ant2, interval, n_ant: int, n_int: int, *, niter: int = 50,
                   tol: float = 1e-8, refant: int = 0, phase_only: bool = False, gains=None):
    """
    The one-shot call `cip_gaincal`: the bounds of the data, the fixed-point
    scale, the correlate and the solve, with the correlations in the library's
    workspace. Returns (gains complex128 (n_int, n_ant), ant_ok uint8, info);
    `info` holds the solver's fields (`device_gain_solve`), `iters` (int64
    tensor (n_int)), the four counts of the correlate, and `quantum`, `shift`,
    `amax`, `wmax` of the scale.
    """
    require_gpu()
    nrow, nchan = _check_columns(vis, model, wgt, ant1, ant2, interval, "device_gaincal")
    dev = vis.device
    n_ant, n_int = int(n_ant), int(n_int)
    out = _gains_io(gains, n_int, n_ant, dev)
    ant_ok = torch.empty((max(n_int, 0), max(n_ant, 0)), dtype=torch.uint8, device=dev)
    iters = torch.empty(max(n_int, 0), dtype=torch.int64, device=dev)
    scale, counts, info = _lib.CalScale(), _lib.CalCounts(), _lib.CalSolveInfo()
    call(dev, "cip_gaincal", *vis_arg(vis), *vis_arg(model), *wgt_arg(wgt), nrow, nchan, ant1, ant2, interval, n_ant,
         n_int, int(niter), float(tol), int(refant), _flags(phase_only), STREAM, out, ant_ok, iters,
         ctypes.byref(scale), ctypes.byref(counts), ctypes.byref(info))
    return out, ant_ok, {**info.as_dict(), "iters": iters, **counts.as_dict(), "quantum": float(scale.quantum),
                         "shift": int(scale.shift), "amax": float(scale.amax), "wmax": float(scale.wmax)}


class GainCorrelator:
    """
    The gain correlations of one data set, accumulated over chunks and ranks:

        gc = GainCorrelator(n_ant, n_int, amax, wmax, nsamp_max, device)
        for chunk in chunks: gc.add_ms(chunk.vis, chunk.model, chunk.wgt, chunk.ant1, chunk.ant2, chunk.interval)
        gc.all_reduce()                       # multi-GPU: exact integer sum
        gains, ant_ok, iters, info = gc.solve(niter=50, tol=1e-8, refant=0)

    `amax` bounds every |real| and |imaginary| part of vis and model, `wmax`
    every weight and `nsamp_max` the number of samples of the whole data set
    (all chunks, all ranks): together they fix the fixed-point scale, so every
    rank must pass the same values. Samples beyond the bounds are left out and
    counted (`self.counts["n_outside"]`). `self.corr` (int64 (n_int, n_ant,
    n_ant, 3)) is a sum of integers: any chunk order and any number of ranks
    give the same bits.
    """

    def __init__(self, n_ant, n_int, amax, wmax, nsamp_max, device):
        require_gpu()
        self.scale = _lib.cal_scale(n_ant, n_int, amax, wmax, nsamp_max)
        self.device = torch.device(device)
        self.corr = torch.zeros(self.scale.corr_shape, dtype=torch.int64, device=self.device)
        self.counts = {"n_added": 0, "n_zero": 0, "n_outside": 0, "n_bad": 0}

    def add_ms(self, vis, model, wgt, ant1, ant2, interval) -> dict:
        """Adds one chunk; returns that chunk's counts."""
        if vis.device != self.device:
            raise ValueError(f"chunk on {vis.device}, correlations on {self.device}")
        _, counts = device_gain_correlate(vis, model, wgt, ant1, ant2, interval, self.scale, self.corr)
        for key, value in counts.items():
            self.counts[key] += value
        return counts

    def all_reduce(self, group=None) -> None:
        """Sums the correlations of every rank of `group` (torch.distributed, SUM on int64: exact)."""
        import torch.distributed as dist  # pylint: disable=import-outside-toplevel

        dist.all_reduce(self.corr, op=dist.ReduceOp.SUM, group=group)

    def solve(self, *, niter: int = 50, tol: float = 1e-8, refant: int = 0, phase_only: bool = False, gains=None):
        """`device_gain_solve` of the accumulated correlations."""
        return device_gain_solve(self.corr, self.scale, niter=niter, tol=tol, refant=refant, phase_only=phase_only,
                                 gains=gains)


def _stage_rows(vis, wgt, ant1, ant2, interval, dev):
    def cplx(x):
        c64 = x.dtype in (np.complex64, torch.complex64)
        return to_device(x, torch.complex64 if c64 else torch.complex128, dev)

    wgt_d = None
    if wgt is not None:
        wgt_d = to_device(wgt, torch.float32 if wgt.dtype in (np.float32, torch.float32) else torch.float64, dev)
    return cplx, cplx(vis), wgt_d, [to_device(np.asarray(a) if not torch.is_tensor(a) else a, torch.int32, dev)
                                    for a in (ant1, ant2, interval)]


def gaincal(vis, model, wgt, ant1, ant2, interval, n_ant, n_int, *, niter=50, tol=1e-8, refant=0, phase_only=False,
            gains=None, device=None):
    """
    `device_gaincal` for host or device arrays: numpy in -> numpy out, torch in
    -> torch out (on the GPU). The inputs are never modified. Returns (gains,
    ant_ok, info).
    """
    require_gpu()
    dev = target_device(device)
    numpy_in = isinstance(vis, np.ndarray)
    with torch.cuda.device(dev):
        cplx, vis_d, wgt_d, cols = _stage_rows(vis, wgt, ant1, ant2, interval, dev)
        if wgt_d is None:
            wgt_d = torch.ones(vis_d.shape, dtype=torch.float32, device=dev)
        gains_d = None if gains is None else to_device(gains, torch.complex128, dev)
        out, ant_ok, info = device_gaincal(vis_d, cplx(model), wgt_d, *cols, n_ant, n_int, niter=niter, tol=tol,
                                           refant=refant, phase_only=phase_only, gains=gains_d)
        if numpy_in:
            out, ant_ok, info["iters"] = out.cpu().numpy(), ant_ok.cpu().numpy(), info["iters"].cpu().numpy()
    return out, ant_ok, info


def gain_apply(vis, wgt, ant1, ant2, interval, gains, ant_ok=None, *, mode="correct", device=None):
    """
    `device_gain_apply` for host or device arrays: numpy in -> numpy out, torch
    in -> torch out (on the GPU). `ant_ok=None`: every antenna is alive. The
    inputs are never modified. Returns (vis_out, wgt_out).
    """
    require_gpu()
    dev = target_device(device)
    numpy_in = isinstance(vis, np.ndarray)
    with torch.cuda.device(dev):
        _, vis_d, wgt_d, cols = _stage_rows(vis, wgt, ant1, ant2, interval, dev)
        gains_d = to_device(gains, torch.complex128, dev)
        if ant_ok is None:
            ok_d = torch.ones(gains_d.shape, dtype=torch.uint8, device=dev)
        else:
            ok_d = to_device(np.asarray(ant_ok) != 0 if not torch.is_tensor(ant_ok) else ant_ok != 0, torch.uint8, dev)
        out, wgt_out = device_gain_apply(vis_d, wgt_d, *cols, gains_d, ok_d, mode=mode)
        if numpy_in:
            out, wgt_out = out.cpu().numpy(), None if wgt_out is None else wgt_out.cpu().numpy()
    return out, wgt_out


def device_selfcal(uvw, freq, vis, wgt, ant1, ant2, interval, npix: int, pixsize: float, *, n_rounds: int,
                   phase_only: bool = True, refant: int = 0, solver_niter: int = 50, solver_tol: float = 1e-8,
                   initial_sky_model=None, **major_cycle_kwargs):
    """
    Self-calibration on device-resident data: `n_rounds` rounds of

      1. `device_major_cycles` (with `major_cycle_kwargs`: `n_major`, `niter`,
         `gain`, ...) on the currently corrected visibilities and weights,
      2. `device_dirty2ms` of its model into one model column, through the
         loop's tile plan,
      3. `device_gaincal` of the ORIGINAL `vis` against that column (one
         solution per antenna and value of `interval`, from unit gains),
      4. `device_gain_apply` of the original `vis` and `wgt` into the corrected
         buffers,

    and one last `device_major_cycles` on the corrected data, whose dict is
    returned with `gains` (complex128 (n_int, n_ant)), `ant_ok`, and per round
    `round_peaks` (the first major cycle's |peak|), `round_rms` (the rms of the
    residual image) and `solver` (the solver's info). The lists have one entry
    per `device_major_cycles` run but `solver`, which has one per round. Only
    scalars cross PCIe. `n_rounds=0` is exactly `device_major_cycles`. The
    number of antennas and intervals is taken from the largest index.
    Amplitude self-calibration (`phase_only=False`) leaves the flux scale free
    to drift; nothing here normalises it.

    `initial_sky_model` (a `skymodel.SkyModel`, for instance a catalogue of
    the field's bright sources): the loop does not start blind. Before the
    first round, `device_dft_predict` of it (with the w term when
    `do_wstacking`) fills the model column, `device_gaincal` solves the
    ORIGINAL `vis` against it and `device_gain_apply` corrects the data, so
    round 1 images calibrated visibilities. The dict then also holds
    `initial_gains`, `initial_ant_ok` and `initial_solver`. With None the loop
    is what it is without the argument.
    """
    require_gpu()
    n_rounds = int(n_rounds)
    if n_rounds < 0:
        raise ValueError("n_rounds must be >= 0")
    if n_rounds == 0:
        return device_major_cycles(uvw, freq, vis, wgt, npix, pixsize, **major_cycle_kwargs)
    nrow, nchan = _check_rows(vis, ant1, ant2, interval, "device_selfcal")
    dev = vis.device
    n_ant = int(max(int(ant1.max()), int(ant2.max()))) + 1 if nrow else 2
    n_int = int(interval.max()) + 1 if nrow else 1
    predict_kw = dict(epsilon=major_cycle_kwargs.get("epsilon", EPSILON), support=major_cycle_kwargs.get("support"),
                      do_wstacking=major_cycle_kwargs.get("do_wstacking", DO_WSTACKING))
    wgt0 = wgt if wgt is not None else torch.ones((nrow, nchan), dtype=torch.float32, device=dev)
    vis_c, wgt_c = vis, wgt
    model_col = torch.empty((nrow, nchan), dtype=vis.dtype, device=dev)
    buf_vis, buf_wgt = torch.empty_like(vis), torch.empty_like(wgt0)
    gains = ant_ok = None
    peaks, rms, solver = [], [], []

    def record(res):
        peaks.append(res["peaks"][0] if res["peaks"] else 0.0)
        rms.append(float(torch.sqrt(torch.mean(res["residual"] * res["residual"]))))

    def solve_and_apply():
        g, ok, info = device_gaincal(vis, model_col, wgt0, ant1, ant2, interval, n_ant, n_int, niter=solver_niter,
                                     tol=solver_tol, refant=refant, phase_only=phase_only)
        info.pop("iters")
        return g, ok, info, device_gain_apply(vis, wgt0, ant1, ant2, interval, g, ok, mode="correct", out=buf_vis,
                                              wgt_out=buf_wgt)

    initial = {}
    if initial_sky_model is not None:
        device_dft_predict(uvw, freq, initial_sky_model, out=model_col, w_term=bool(predict_kw["do_wstacking"]))
        g0, ok0, info0, (vis_c, wgt_c) = solve_and_apply()
        initial = dict(initial_gains=g0, initial_ant_ok=ok0, initial_solver=info0)
    for _round in range(n_rounds):
        res = device_major_cycles(uvw, freq, vis_c, wgt_c, npix, pixsize, **major_cycle_kwargs)
        record(res)
        device_dirty2ms(uvw, freq, res["model"], None, pixsize, pixsize, out=model_col, reuse_plan=True, **predict_kw)
        gains, ant_ok, info, (vis_c, wgt_c) = solve_and_apply()
        solver.append(info)
    res = device_major_cycles(uvw, freq, vis_c, wgt_c, npix, pixsize, **major_cycle_kwargs)
    record(res)
    res.update(gains=gains, ant_ok=ant_ok, round_peaks=peaks, round_rms=rms, solver=solver, **initial)
    return res
