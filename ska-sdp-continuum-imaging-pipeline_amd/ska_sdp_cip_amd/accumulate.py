"""
Accumulating gridder: visibilities arriving in chunks (row blocks of a
measurement set, or uvw_tiling tile chunk files) are gridded onto ONE set of
resident uv-grid planes in HBM, and the dirty image is made once at the end.

This is the device side of SURVEY.md 8(f) item 2 (tile on-disk format and
chunked host -> HBM streaming, config C5): the reference grids a whole
(row x freq) dask chunk per ducc0 call and sums the per-chunk IMAGES
(invert.py:187-209); here the chunks are summed on the GRID (linearity,
exact up to the per-chunk fixed-point rounding, < 1e-13 of max|wV|), so a
data set of any size costs one FFT.

C ABI: cip_grid_ms (dense rows), cip_grid_tiles (ragged row slices, the Tile
layout of reference uvw_tiling/tile.py:14-124), cip_grid_to_dirty,
cip_grid_layout (include/cip.h).
"""

from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib
from ._call import STREAM, call, check_array, check_tensor, require_gpu, target_device, vis_arg, wgt_arg

try:
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None

SPEED_OF_LIGHT = 299792458.0


def w_range_rows(uvw: np.ndarray, channel_freqs: np.ndarray) -> tuple[float, float]:
    """w range (wavelengths) over all rows x channels (the range the one-shot
    gridder computes on the device: extremes at the extreme frequencies)."""
    w = np.asarray(uvw, dtype=np.float64)[:, 2]
    f = np.asarray(channel_freqs, dtype=np.float64) / SPEED_OF_LIGHT
    if w.size == 0:
        return 0.0, 0.0
    a, b = w * f.min(), w * f.max()
    return float(min(a.min(), b.min())), float(max(a.max(), b.max()))


def w_range_slices(uvw: np.ndarray, chan_start: np.ndarray, chan_stop: np.ndarray,
                   channel_freqs: np.ndarray) -> tuple[float, float]:
    """w range (wavelengths) of row slices, by the one-shot gridder's rule
    (each non-empty slice's w at the extreme channel frequencies), so tiles of
    a measurement set get the planes of the whole set. (inf, -inf) if empty."""
    keep = np.asarray(chan_stop) > np.asarray(chan_start)
    if not keep.any():
        return np.inf, -np.inf
    return w_range_rows(np.asarray(uvw, dtype=np.float64)[keep], channel_freqs)


def merge_w_ranges(ranges) -> tuple[float, float]:
    """Union of (wmin, wmax) ranges."""
    lo, hi = np.inf, -np.inf
    for a, b in ranges:
        lo, hi = min(lo, a), max(hi, b)
    return lo, hi


class GridAccumulator:
    """
    uv-grid planes resident in HBM that chunks of visibilities are added to.

    Parameters are fixed at construction (`cip_choose_params`; in w-stacking
    mode the w range of the WHOLE data set must be given, as the one-shot
    gridder derives it from all visibilities). `add_ms` / `add_tile` accept
    device tensors on the accumulator's device and run on the current stream;
    `dirty()` returns the (unnormalised) dirty image and the weight sum,
    `image()` the normalised image (reference invert.py:149).
    """

    def __init__(self, npix_x: int, npix_y: int, pixsize_x: float, pixsize_y: float, *,
                 epsilon: float = 1e-4, support: Optional[int] = None, do_wstacking: bool = False,
                 w_range: tuple[float, float] = (0.0, 0.0), device=None,
                 single_precision_accumulation: bool = False):
        require_gpu()
        self.npix_x, self.npix_y = int(npix_x), int(npix_y)
        self.pixsize_x, self.pixsize_y = float(pixsize_x), float(pixsize_y)
        wmin, wmax = w_range
        if not wmin <= wmax:  # no visibilities seen: any valid stack
            wmin = wmax = 0.0
        self.params = _lib.choose_params(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, support or 0,
                                         do_wstacking, wmin, wmax)
        self.device = target_device(device)
        p = self.params
        self.planes = torch.zeros((p.nplanes, p.nu * p.nv * 2), dtype=torch.float64, device=self.device)
        self.sum_weights = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.transposed = bool(_lib.lib().cip_grid_layout(p, self.npix_x, self.npix_y))
        self.flags = _lib.CIP_ACC_SINGLE if single_precision_accumulation else 0
        self.num_visibilities = 0
        self._done = False

    def _check(self, *tensors):
        if self._done:
            raise RuntimeError("dirty() consumed the grid planes; make a new GridAccumulator")
        for t in tensors:
            if t is not None:
                check_tensor(t, self.device, "chunks")

    def add_ms(self, uvw, freq, vis, wgt=None) -> None:
        """Add MS rows: uvw (nrow, 3) f64, freq (nchan) f64, vis (nrow, nchan)
        complex64/128, wgt (nrow, nchan) f32/f64 or None."""
        self._check(uvw, freq, vis, wgt)
        nrow, nchan = uvw.shape[0], freq.shape[0]
        if tuple(vis.shape) != (nrow, nchan) or (wgt is not None and tuple(wgt.shape) != (nrow, nchan)):
            raise ValueError("vis / wgt must have shape (nrow, nchan)")
        call(self.device, "cip_grid_ms", uvw, nrow, freq, nchan, *vis_arg(vis), *wgt_arg(wgt), self.params,
             self.pixsize_x, self.pixsize_y, self.npix_x, self.npix_y, self.flags, STREAM, self.planes,
             self.sum_weights)
        self.num_visibilities += nrow * nchan

    def add_ms_stokes_i(self, uvw, freq, vis4, flags4, wgt4) -> None:
        """Add MS rows given as raw linear-feed columns (cip_grid_ms_stokes_i:
        Stokes I and effective weights formed on load, reference
        invert.py:78-116): vis4 (nrow, nchan, 4) complex64, flags4 uint8/bool
        or None, wgt4 float32."""
        self._check(uvw, freq, vis4, flags4, wgt4)
        nrow, nchan = uvw.shape[0], freq.shape[0]
        shape = (nrow, nchan, 4)
        if vis4.dtype != torch.complex64 or wgt4.dtype != torch.float32 or tuple(vis4.shape) != shape or \
                tuple(wgt4.shape) != shape or (flags4 is not None and tuple(flags4.shape) != shape):
            raise ValueError(f"vis4 complex64, wgt4 float32 and flags4 must have shape {shape}")
        if flags4 is not None and flags4.dtype == torch.bool:
            flags4 = flags4.view(torch.uint8)
        call(self.device, "cip_grid_ms_stokes_i", uvw, nrow, freq, nchan, vis4, flags4, wgt4, self.params,
             self.pixsize_x, self.pixsize_y, self.npix_x, self.npix_y, self.flags, STREAM, self.planes,
             self.sum_weights)
        self.num_visibilities += nrow * nchan

    def add_tile(self, slice_uvw, chan_start, chan_stop, freq, vis, wgt=None) -> None:
        """Add one tile chunk (Tile layout): slice_uvw (ns, 3) f64, chan_start /
        chan_stop (ns) int32, freq (nchan) f64, vis (nvis) complex, wgt (nvis)
        f32/f64 or None (unit weights, as the reference's tiles carry none)."""
        self._check(slice_uvw, chan_start, chan_stop, freq, vis, wgt)
        if chan_start.dtype != torch.int32 or chan_stop.dtype != torch.int32:
            raise ValueError("channel ranges must be int32")
        ns = slice_uvw.shape[0]
        nvis = vis.shape[0]
        if wgt is not None and tuple(wgt.shape) != (nvis,):
            raise ValueError("wgt must have the shape of vis")
        vis_ptr, vis_code = vis_arg(vis)
        call(self.device, "cip_grid_tiles", slice_uvw, chan_start, chan_stop, ns, freq, freq.shape[0], vis_ptr, nvis,
             vis_code, *wgt_arg(wgt), self.params, self.pixsize_x, self.pixsize_y, self.npix_x, self.npix_y,
             self.flags, STREAM, self.planes, self.sum_weights)
        self.num_visibilities += nvis

    def dirty(self, out=None):
        """(dirty fp64 (npix_x, npix_y), weight sum (1,)): FFT, w-screens and
        grid correction of the accumulated planes (which this consumes)."""
        self._check()
        if out is None:
            out = torch.empty((self.npix_x, self.npix_y), dtype=torch.float64, device=self.device)
        else:
            check_array(out, (torch.float64,), (self.npix_x, self.npix_y), self.device, "out")
        call(self.device, "cip_grid_to_dirty", self.planes, self.params, self.npix_x, self.npix_y, self.pixsize_x,
             self.pixsize_y, STREAM, out)
        self._done = True
        return out, self.sum_weights

    def image(self):
        """Normalised dirty image (dirty / sum of weights, reference invert.py:149)."""
        d, sw = self.dirty()
        return d / sw
