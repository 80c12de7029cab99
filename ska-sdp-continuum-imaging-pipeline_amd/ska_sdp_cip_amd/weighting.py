"""
Imaging weights on the GPU: uniform and Briggs (robust) weighting
(`cip_imaging_weights` and the `cip_weight_*` calls of libcip_hip.so).

The operator is defined exactly in include/cip.h: the field-of-view cell of
every visibility (Hermitian fold to v >= 0, fp64 without contraction), the
density as 64-bit fixed-point sums of the weights (integer atomic adds, so the
array does not depend on arrival order, chunking or the number of ranks), and

    uniform:  w / D          (0 where D is 0)
    briggs:   w / (1 + D f2),   f2 = (5 10^-robust)^2 / (sum D^2 / sum w)

with D the density of the visibility's cell. Natural weighting is the weights
as they are and needs no library call.
"""

from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np

from . import _lib
from ._call import (STREAM, WGT_DTYPES, call, check_array, check_rows, require_gpu, target_device, to_device,
                    wgt_arg)

try:
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None


def _mode(weighting: str) -> int:
    try:
        return _lib.WEIGHTING_MODES[weighting]
    except KeyError:
        raise ValueError(f"weighting must be one of {sorted(_lib.WEIGHTING_MODES)}, got {weighting!r}") from None


def briggs_f2(robust: float, sum_w: float, sum_d2: float) -> float:
    """f2 of the Briggs formula, as `cip_imaging_weights` computes it on the host."""
    if not sum_w > 0.0:
        return 0.0
    t = 5.0 * math.pow(10.0, -float(robust))
    return (t * t) / (sum_d2 / sum_w)


def _check_columns(uvw, freq, wgt, what):
    """Shapes, dtypes and placement of one chunk; returns (nrow, nchan, wgt pointer, wgt code)."""
    nrow, nchan = check_rows(uvw, freq, what)
    wgt_args = wgt_arg(wgt)
    if wgt is not None:
        check_array(wgt, WGT_DTYPES, (nrow, nchan), uvw.device, "wgt")
    return nrow, nchan, *wgt_args


def _check_out(out, wgt, nrow, nchan, device):
    """The output tensor (allocated in the dtype of `wgt`, float64 without weights)."""
    if out is None:
        return torch.empty((nrow, nchan), dtype=torch.float64 if wgt is None else wgt.dtype, device=device)
    check_array(out, WGT_DTYPES, (nrow, nchan), device, "out")
    if wgt is not None and out.data_ptr() == wgt.data_ptr() and out.dtype != wgt.dtype:
        raise ValueError("in place needs out.dtype == wgt.dtype")
    return out


def device_imaging_weights(
    uvw: "torch.Tensor",
    freq: "torch.Tensor",
    wgt: Optional["torch.Tensor"],
    npix_x: int,
    npix_y: int,
    pixsize_x: float,
    pixsize_y: float,
    *,
    weighting: str = "briggs",
    robust: float = 0.0,
    out: Optional["torch.Tensor"] = None,
):
    """
    Imaging weights of device-resident data for an image of `npix_x` x
    `npix_y` pixels of `pixsize_x`, `pixsize_y` radians. `uvw` (nrow, 3) and
    `freq` (nchan) float64, `wgt` (nrow, nchan) float32 / float64 or None (all
    ones). Returns (wgt_out, info): `wgt_out` has `wgt`'s dtype (`out`'s when
    given; `out` may be `wgt` itself), `info` holds `sum_w`, `sum_d2`, `f2`,
    `quantum`, `n_added`, `n_outside`, `n_cells`.

    `weighting="natural"` returns `wgt` unchanged (and an empty info) without
    a library call; "uniform" and "briggs" (with `robust`) run
    `cip_imaging_weights`. A zero weight and a sample outside the image's uv
    cells get weight 0. A negative or non-finite weight is a ValueError.
    """
    mode = _mode(weighting)
    if mode == _lib.CIP_WEIGHT_NATURAL:
        return wgt, {}
    require_gpu()
    nrow, nchan, wgt_ptr, wgt_code = _check_columns(uvw, freq, wgt, "device_imaging_weights inputs")
    out = _check_out(out, wgt, nrow, nchan, uvw.device)
    info = _lib.WeightInfo()
    call(uvw.device, "cip_imaging_weights", uvw, nrow, freq, nchan, wgt_ptr, wgt_code, int(npix_x), int(npix_y),
         float(pixsize_x), float(pixsize_y), mode, float(robust), STREAM, *wgt_arg(out), ctypes.byref(info))
    return out, info.as_dict()


def imaging_weights(uvw, freq, wgt, npix_x, npix_y, pixsize_x, pixsize_y, *, weighting="briggs", robust=0.0,
                    device=None):
    """
    `device_imaging_weights` for host or device arrays: numpy in -> numpy out,
    torch in -> torch out (on the GPU). The inputs are never modified. Returns
    (wgt_out, info).
    """
    if _mode(weighting) == _lib.CIP_WEIGHT_NATURAL:
        return wgt, {}
    require_gpu()
    dev = target_device(device)
    numpy_in = isinstance(uvw, np.ndarray)
    with torch.cuda.device(dev):
        wgt_d = None
        if wgt is not None:
            f32 = (wgt.dtype == np.float32) if isinstance(wgt, np.ndarray) else (wgt.dtype == torch.float32)
            wgt_d = to_device(wgt, torch.float32 if f32 else torch.float64, dev)
        out, info = device_imaging_weights(to_device(uvw, torch.float64, dev), to_device(freq, torch.float64, dev),
                                           wgt_d, npix_x, npix_y, pixsize_x, pixsize_y, weighting=weighting,
                                           robust=robust)
    return (out.cpu().numpy() if numpy_in else out), info


class WeightDensity:
    """
    The weight density of one image, accumulated over chunks and ranks:

        wd = WeightDensity(npix_x, npix_y, pixsize_x, pixsize_y, wmax, nvis_max, device)
        for chunk in chunks: wd.add_ms(chunk.uvw, chunk.freq, chunk.wgt)
        wd.all_reduce()                       # multi-GPU: exact integer sum
        wd.finish("briggs", robust=-0.5)
        for chunk in chunks: w = wd.apply(chunk.uvw, chunk.freq, chunk.wgt)

    `wmax` bounds every weight and `nvis_max` the number of visibilities of
    the whole data set (all chunks, all ranks): together they fix the
    fixed-point scale, so every rank must pass the same values. The density
    (`self.density`, int64 (2 (npix_x // 2) + 1, npix_y // 2 + 1)) is a sum of
    integers: any chunk order and any number of ranks give the same bits.
    """

    def __init__(self, npix_x, npix_y, pixsize_x, pixsize_y, wmax, nvis_max, device):
        require_gpu()
        self.grid = _lib.weight_grid(npix_x, npix_y, pixsize_x, pixsize_y, wmax, nvis_max)
        self.device = torch.device(device)
        self.density = torch.zeros(self.grid.density_shape, dtype=torch.int64, device=self.device)
        self.counts = {"n_added": 0, "n_outside": 0}
        self.mode = None
        self.f2 = 0.0
        self.stats = None

    def add_ms(self, uvw, freq, wgt) -> dict:
        """Adds one chunk's weights; returns that chunk's counts."""
        nrow, nchan, wgt_ptr, wgt_code = _check_columns(uvw, freq, wgt, "WeightDensity.add_ms inputs")
        if uvw.device != self.device:
            raise ValueError(f"chunk on {uvw.device}, density on {self.device}")
        counts = (ctypes.c_int64 * 3)()
        call(self.device, "cip_weight_density", uvw, nrow, freq, nchan, wgt_ptr, wgt_code, ctypes.byref(self.grid),
             STREAM, self.density, counts)
        self.counts["n_added"] += int(counts[0])
        self.counts["n_outside"] += int(counts[1])
        self.mode = None  # the statistics are stale
        return {"n_added": int(counts[0]), "n_outside": int(counts[1])}

    def all_reduce(self, group=None) -> None:
        """Sums the densities of every rank of `group` (torch.distributed, SUM on int64: exact)."""
        import torch.distributed as dist  # pylint: disable=import-outside-toplevel

        dist.all_reduce(self.density, op=dist.ReduceOp.SUM, group=group)
        self.mode = None

    def finish(self, weighting: str = "briggs", robust: float = 0.0) -> dict:
        """The density's statistics and the Briggs f2; selects what `apply` computes."""
        mode = _mode(weighting)
        if mode == _lib.CIP_WEIGHT_NATURAL:
            raise ValueError("natural weighting needs no density")
        if not math.isfinite(float(robust)):
            raise ValueError("robust must be finite")
        stats = (ctypes.c_double * 3)()
        call(self.device, "cip_weight_stats", self.density, ctypes.byref(self.grid), STREAM, stats)
        self.f2 = briggs_f2(robust, stats[0], stats[1]) if mode == _lib.CIP_WEIGHT_BRIGGS else 0.0
        if not math.isfinite(self.f2):
            raise ValueError("robust gives no finite f2")
        self.mode = mode
        self.stats = {"sum_w": float(stats[0]), "sum_d2": float(stats[1]), "n_cells": int(stats[2]), "f2": self.f2,
                      "quantum": float(self.grid.quantum), **self.counts}
        return dict(self.stats)

    def apply(self, uvw, freq, wgt, out=None):
        """The chunk's imaging weights (stream-ordered; `out` may be `wgt`)."""
        if self.mode is None:
            raise RuntimeError("call finish() after the last add_ms() / all_reduce()")
        nrow, nchan, wgt_ptr, wgt_code = _check_columns(uvw, freq, wgt, "WeightDensity.apply inputs")
        if uvw.device != self.device:
            raise ValueError(f"chunk on {uvw.device}, density on {self.device}")
        out = _check_out(out, wgt, nrow, nchan, self.device)
        call(self.device, "cip_weight_apply", uvw, nrow, freq, nchan, wgt_ptr, wgt_code, self.density,
             ctypes.byref(self.grid), self.mode, self.f2, STREAM, *wgt_arg(out))
        return out
