"""
Strong scaling of ONE dirty image over several GPUs: uv strips with a halo
exchange before the FFT (SURVEY.md 8(e) option 1; the north
star's "UVW tiles shard naturally across the 8 GPUs ... RCCL reduce over xGMI
of overlapping partial-grid halos before the FFT-to-dirty-image step").

The uv grid is stored transposed for the pruned FFT (gT[y][x], y along v).
Rank r owns grid rows [y0_r, y1_r) - contiguous v strips balanced by
visibility count - and grids the visibilities whose footprint origin row lies
in its strip (the UVW tiles of that strip: the data layout the reference's
reorder_by_uvw_tile produces offline, reorder.py:19-111). A footprint reaches
W - 1 rows past the origin, so rank r's partial grid also holds rows
[y1_r, y1_r + W - 1) of its successor (mod nv): that halo goes to rank r + 1
(point-to-point, RCCL over xGMI) and is added there. Then the FFT runs
distributed: pass A (along u) on each rank's own rows, one all-to-all that
hands every rank the pass-A columns of its image rows [i0_r, i1_r) (blocks of
4 kept u frequencies x all v), pass B (along v) + crop + grid correction on
them, and a gather of the image rows onto the destination rank. The weight sum
is all-reduced and divided out in pass B's epilogue. Traffic per rank at C4
(16384^2 grid, 8 ranks): halo 1.8 MB, all-to-all 224 MB, image rows 64 MB -
against a 4 GiB partial-grid reduce for row (weak) sharding.

The per-rank stages are a `StripBackend` (`HipStripBackend` runs them through
libcip_hip.so; tests plug in a CPU restatement). Their order is written once,
in `_invert`: a driver over the ranks present in the process and the planes
of their buffers (2-D is the one-plane case), which moves data between ranks
only through an exchange object - halo ring, weight-sum reduction, live-mask
all-gather, all-to-all, image-row gather. `invert_strips` runs it for one rank
with torch.distributed collectives (`_DistExchange`: RCCL, or gloo on CPU
tensors); `invert_strips_local` for all ranks in one process on one device
with the exchanges in memory (`_LocalExchange`) - the single-GPU check of the
decomposition, running the distributed path's own stages.
"""

from __future__ import annotations

import os
import time
from dataclasses import dataclass
from typing import Optional, Sequence

import ctypes

import numpy as np

from . import _lib
from ._call import STREAM, call, require_gpu, target_device, vis_arg, wgt_arg

SPEED_OF_LIGHT = 299792458.0
COL_BLOCK = 4  # pass-A output block width (cip_fft.hip kColBlock)

try:
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None


@dataclass
class StripLayout:
    """Row strips of the grid and image-row strips of the dirty image.

    y_bounds: world + 1 grid-row bounds (0 .. nv); x_bounds: world + 1 image-
    row bounds (0 .. npix_x, multiples of COL_BLOCK); halo = W - 1 rows.
    """

    nu: int
    nv: int
    npix_x: int
    npix_y: int
    support: int
    y_bounds: list
    x_bounds: list

    @property
    def world(self) -> int:
        return len(self.y_bounds) - 1

    @property
    def halo(self) -> int:
        return self.support - 1

    def rows(self, r: int) -> tuple[int, int]:
        return self.y_bounds[r], self.y_bounds[r + 1]

    def image_rows(self, r: int) -> tuple[int, int]:
        return self.x_bounds[r], self.x_bounds[r + 1]


def origin_rows(v_m, fx, scale_v: float, nv: int, support: int):
    """Footprint origin row of every (row, channel): iy0 = floor(v f/c nv
    pixsize_y + nv/2 - W/2) + 1, wrapped into [0, nv) - the gridder's placement
    arithmetic (cip_common.h place_vis: the same fp64 operations in the same
    order), so the strip a visibility is assigned to is the one its footprint
    starts in. v_m (nrow,), fx (nchan,) tensors -> (nrow, nchan) int64."""
    y = (v_m[:, None] * fx[None, :]) * scale_v + float(nv // 2)
    iy0 = torch.floor(y - float(support // 2)).to(torch.int64) + 1
    return torch.remainder(iy0, nv)


TILE = 32  # the scatter's tile edge (cip_common.h kTile): the dirty-tile mask's unit


def _on_device(t) -> bool:
    """CUDA tensors take the HIP split (cip_strips.hip); CPU tensors (the gloo
    tests' ranks) the torch restatement of the same arithmetic."""
    return t is not None and getattr(t, "is_cuda", False)


def _gridder_params(params):
    """The ctypes cip_gridder_params of `params` (a GridderParams, or any object
    with its fields - the CPU tests' stand-in)."""
    if isinstance(params, _lib.GridderParams):
        return params
    out = _lib.GridderParams()
    for name, _ in _lib.GridderParams._fields_:
        setattr(out, name, type(getattr(out, name))(getattr(params, name, 32 if name == "tile" else 0)))
    return out


def strip_histogram(uvw, freq, params, pixsize_x: float, pixsize_y: float):
    """(visibilities, row slices) per grid row (int64 (nv,) tensors each): by
    footprint-origin row, a slice starting at each row's first channel and
    wherever the origin's 32-cell tile changes along the channels. CUDA
    tensors: one HIP pass (cip_strip_histogram, block-private LDS histograms);
    CPU tensors: the torch restatement below."""
    nu, nv, W = int(params.nu), int(params.nv), int(params.support)
    if _on_device(uvw):
        hist = torch.empty(2 * nv, dtype=torch.int64, device=uvw.device)
        uvw_c, f_c = uvw.contiguous().to(torch.float64), freq.contiguous().to(torch.float64)
        call(uvw.device, "cip_strip_histogram", uvw_c, int(uvw_c.shape[0]), f_c, int(f_c.shape[0]),
             _gridder_params(params), float(pixsize_x), float(pixsize_y), STREAM, hist)
        return hist[:nv], hist[nv:]
    fx = freq / SPEED_OF_LIGHT
    vis = torch.zeros(nv, dtype=torch.int64, device=uvw.device)
    runs = torch.zeros(nv, dtype=torch.int64, device=uvw.device)
    for a, b in _row_chunks(uvw.shape[0]):
        iy = origin_rows(uvw[a:b, 1], fx, float(params.nv) * pixsize_y, nv, W)
        ix = origin_rows(uvw[a:b, 0], fx, float(params.nu) * pixsize_x, nu, W)
        key = torch.div(iy, 32, rounding_mode="floor") * (nu // 32 + 1) + torch.div(ix, 32, rounding_mode="floor")
        start = torch.ones_like(key, dtype=torch.bool)
        start[:, 1:] = key[:, 1:] != key[:, :-1]
        vis += torch.bincount(iy.reshape(-1), minlength=nv)
        runs += torch.bincount(iy[start], minlength=nv)
    return vis, runs


def _row_chunks(nrow: int, chunk: int = 65536):
    for a in range(0, nrow, chunk):
        yield a, min(nrow, a + chunk)


# Per-rank cost model of a strip (measured on MI355X, profiles/
# r04_strong_model_c4_n8.json: the 8 strips of C4 balanced by visibility count
# took 6.7-9.5 ms to grid, linear in their row slices): gridding costs
# ~36.9 ps per visibility + ~112 ps per row slice (the planner's runs and the
# scatter's per-slice loads), pass A ~8.9 ps per grid cell of the strip's rows.
COST_PS_PER_VIS = 36.9
COST_PS_PER_SLICE = 112.0
COST_PS_PER_CELL = 8.9


def row_costs(uvw, freq, params, pixsize_x: float, pixsize_y: float, a2a_ps_per_row: float = 0.0):
    """Modelled cost (ps) of each grid row as a strip member: its visibilities
    (by footprint-origin row; per tap, W^2 taps per visibility, W^3 with
    w-stacking - the C3 reference call's w-stacking strips measured 0.63 ps
    per tap against 0.58 for C4's W = 8), the row slices starting there (a
    slice starts at each row's first channel and wherever the origin's 32-cell
    tile changes along the channels) and its pass-A cells (one pass per w
    plane), plus `a2a_ps_per_row` per row and plane: the row's pass-A output
    crossing the all-to-all (a rank's exchange time grows with its rows)."""
    nu, W = int(params.nu), int(params.support)
    wstack = bool(int(getattr(params, "do_wstacking", 0)))
    taps = W * W * (W if wstack else 1)
    nplanes = int(params.nplanes) if wstack else 1
    vis, runs = strip_histogram(uvw, freq, params, pixsize_x, pixsize_y)
    cost = (COST_PS_PER_VIS * (taps / 64.0) * vis.double() + COST_PS_PER_SLICE * runs.double() +
            (COST_PS_PER_CELL * nu + a2a_ps_per_row) * nplanes)
    return cost.cpu().numpy()


def plan_strips(uvw, freq, params, pixsize_y: float, npix_x: int, npix_y: int, world: int,
                balance: str = "cost", pixsize_x: Optional[float] = None,
                link_gbs: Optional[float] = None) -> StripLayout:
    """Balanced strips: grid-row bounds splitting a per-row histogram (all
    visibilities, so every rank computes the same bounds without
    communication) into `world` near-equal parts, each at least W rows high
    (the halo then only reaches the next strip); image rows split into
    near-equal multiples of COL_BLOCK. balance="cost": the measured per-rank
    cost model (`row_costs`: visibilities, row slices, pass-A rows; needs
    pixsize_x, default pixsize_y) plus, for world > 1 and `link_gbs` (off by
    default), each row's share of the all-to-all: its pass-A output (npix_x
    complex128) leaves on world - 1 links, 16 npix_x / world bytes per link
    at link_gbs - the tall, sparse edge strips of long baselines get fewer
    rows (C4 at 8 ranks: 5.86x modelled at 64 GB/s against 5.93x unpriced,
    profiles/r05g_strong_model_c4_bal64.json - the grid imbalance costs more
    than the exchange gains); "vis":
    visibility count only. uvw (nrow, 3), freq (nchan) tensors."""
    nv, W = int(params.nv), int(params.support)
    if world < 1:
        raise ValueError("world must be >= 1")
    nb = npix_x // COL_BLOCK
    if npix_x % COL_BLOCK != 0 or nb < world:
        raise ValueError(f"npix_x must be a multiple of {COL_BLOCK} with at least one block of "
                         f"{COL_BLOCK} image rows per rank")
    if nv < W * world:
        raise ValueError("grid too small for this many strips")
    if balance == "cost":
        a2a = 16.0 * npix_x / world / (link_gbs * 1e9) * 1e12 if (world > 1 and link_gbs) else 0.0
        hist = row_costs(uvw, freq, params, pixsize_y if pixsize_x is None else pixsize_x, pixsize_y,
                         a2a_ps_per_row=a2a)
    elif balance == "vis":
        hist = strip_histogram(uvw, freq, params, pixsize_y if pixsize_x is None else pixsize_x,
                               pixsize_y)[0].cpu().numpy()
    else:
        raise ValueError("balance must be 'cost' or 'vis'")
    cum = np.cumsum(hist)
    total = float(cum[-1]) if cum.size else 0.0
    bounds = [0]
    for r in range(1, world):
        target = total * r / world
        y = int(np.searchsorted(cum, target, side="left")) + 1
        y = max(y, bounds[-1] + W)
        y = min(y, nv - W * (world - r))
        bounds.append(y)
    bounds.append(nv)
    return StripLayout(int(params.nu), nv, int(npix_x), int(npix_y), W, bounds,
                       [COL_BLOCK * (r * nb // world) for r in range(world + 1)])


@dataclass
class StripData:
    """One strip's visibilities in the Tile layout (reference
    uvw_tiling/tile.py:14-124): row slices with uvw and channel ranges,
    visibilities / weights concatenated in slice order."""

    slice_uvw: "torch.Tensor"   # (ns, 3) f64
    chan_start: "torch.Tensor"  # (ns,) int32
    chan_stop: "torch.Tensor"   # (ns,) int32
    vis: "torch.Tensor"         # (nvis,) complex
    wgt: Optional["torch.Tensor"]  # (nvis,) f32/f64 or None
    rows: "torch.Tensor"        # (ns,) int64: the MS row of each slice

    @property
    def nvis(self) -> int:
        return int(self.vis.shape[0])


def _split_device(uvw, freq, params, pixsize_y: float, y0: int, y1: int, vis=None, wgt=None):
    """cip_strip_split: (slice_uvw, c0, c1 (int32), rows (int64), vis, wgt)
    of the strip [y0, y1) - one count pass + scans, then one emit pass that
    writes the slices and gathers the strip's visibilities (when given)."""
    dev = uvw.device
    uvw_c, f_c = uvw.contiguous().to(torch.float64), freq.contiguous().to(torch.float64)
    nrow, nchan = int(uvw_c.shape[0]), int(f_c.shape[0])
    if vis is not None:
        vis = vis.reshape(nrow, nchan).contiguous()
        wgt = None if wgt is None else wgt.reshape(nrow, nchan).contiguous()
    counts = (ctypes.c_int64 * 2)()
    args = (uvw_c, nrow, f_c, nchan, *vis_arg(vis), *wgt_arg(wgt), _gridder_params(params), float(pixsize_y), int(y0),
            int(y1), STREAM, counts)
    call(dev, "cip_strip_split", *args, None, None, None, None, None, None)
    ns, nvis = int(counts[0]), int(counts[1])
    suvw = torch.empty((ns, 3), dtype=torch.float64, device=dev)
    c0 = torch.empty(ns, dtype=torch.int32, device=dev)
    c1 = torch.empty(ns, dtype=torch.int32, device=dev)
    rows = torch.empty(ns, dtype=torch.int64, device=dev)
    vout = torch.empty(nvis, dtype=vis.dtype, device=dev) if vis is not None else None
    wout = torch.empty(nvis, dtype=wgt.dtype, device=dev) if wgt is not None else None
    if ns:  # an empty strip needs no emit pass
        call(dev, "cip_strip_split", *args, suvw, c0, c1, rows, vout, wout)
    return suvw, c0, c1, rows, vout, wout


def split_strip(uvw, freq, vis, wgt, params, pixsize_y: float, y0: int, y1: int) -> "StripData":
    """Rank-local strip data from dense (nrow, nchan) columns: the row slices
    whose footprint-origin rows lie in [y0, y1) and their visibilities /
    weights, in the Tile layout (the reference's reorder_by_uvw_tile output,
    reorder.py:19-111, cut by strip). CUDA tensors: cip_strip_split (one
    count pass, one emit + gather pass); CPU tensors: strip_slices +
    gather_strip (the same slices and order)."""
    if _on_device(uvw):
        suvw, c0, c1, rows, v, w = _split_device(uvw, freq, params, pixsize_y, y0, y1, vis, wgt)
        return StripData(suvw, c0, c1, v, w, rows)
    rows, c0, c1 = strip_slices(uvw, freq, params, pixsize_y, y0, y1)
    return gather_strip(uvw, vis, wgt, rows, c0, c1)


def strip_slices(uvw, freq, params, pixsize_y: float, y0: int, y1: int):
    """(rows, c0, c1) int64 tensors: the maximal channel runs of each row whose
    origin row lies in [y0, y1) (one run per row unless a row's v track wraps
    or leaves and re-enters the strip). CUDA tensors: cip_strip_split."""
    if _on_device(uvw):
        _, c0, c1, rows, _, _ = _split_device(uvw, freq, params, pixsize_y, y0, y1)
        return rows, c0.to(torch.int64), c1.to(torch.int64)
    nv, W = int(params.nv), int(params.support)
    fx = freq / SPEED_OF_LIGHT
    scale_v = float(params.nv) * pixsize_y
    rows_l, c0_l, c1_l = [], [], []
    for a, b in _row_chunks(uvw.shape[0]):
        iy = origin_rows(uvw[a:b, 1], fx, scale_v, nv, W)
        m = (iy >= y0) & (iy < y1)
        pad = torch.zeros((m.shape[0], 1), dtype=torch.bool, device=m.device)
        mp = torch.cat([pad, m, pad], dim=1)
        starts = torch.nonzero(mp[:, 1:] & ~mp[:, :-1])  # (row, channel) of each run start
        stops = torch.nonzero(~mp[:, 1:] & mp[:, :-1])   # (row, channel) one past each run's end
        rows_l.append(starts[:, 0] + a)
        c0_l.append(starts[:, 1])
        c1_l.append(stops[:, 1])
    if not rows_l:
        e = torch.zeros(0, dtype=torch.int64, device=uvw.device)
        return e, e, e
    return torch.cat(rows_l), torch.cat(c0_l), torch.cat(c1_l)


def gather_strip(uvw, vis, wgt, rows, c0, c1) -> StripData:
    """The strip's Tile-layout data from dense (nrow, nchan) columns."""
    nchan = vis.shape[1]
    lengths = (c1 - c0)
    starts = rows * nchan + c0
    idx = torch.repeat_interleave(starts, lengths)
    if idx.numel():
        first = torch.repeat_interleave(torch.cumsum(lengths, 0) - lengths, lengths)
        idx = idx + (torch.arange(idx.numel(), device=idx.device) - first)
    return StripData(uvw[rows].contiguous(), c0.to(torch.int32), c1.to(torch.int32),
                     vis.reshape(-1)[idx].contiguous(), None if wgt is None else wgt.reshape(-1)[idx].contiguous(),
                     rows)


def strip_buffer_rows(layout: StripLayout, r: int) -> tuple[int, int]:
    """(row0, nrows) of rank r's grid buffer: its strip rows [y0, y1) plus the
    W - 1 halo rows after them (buffer row k = grid row (y0 + k) mod nv). One
    strip holding the whole grid: (0, nv), its halo wraps onto its own rows."""
    y0, y1 = layout.rows(r)
    if layout.world == 1:
        return 0, layout.nv
    return y0, y1 - y0 + layout.halo


class StripBackend:
    """One rank's stages of the strip invert: everything the driver (`_invert`)
    asks of a backend. The stages below must be implemented; the attributes and
    the two optional stages after them have defaults. A backend also carries
    `npix_y` (the image rows' length)."""

    nplanes = 1     # w planes in the buffer (1: the 2-D gridder)
    single = False  # the packed class: pass-A blocks cross the all-to-all as complex64
    device = None   # the torch device of the buffers (None: the host)
    ranks = None    # invert_strips_local's per-rank backends, kept between calls

    def spawn(self) -> "StripBackend":
        """A backend of the same configuration (another rank's, for the single-process emulation)."""
        raise NotImplementedError

    def bind(self, layout: StripLayout, rank: int) -> "StripBackend":
        """Hold rank `rank`'s strip + halo rows of `layout` (`strip_buffer_rows`)."""
        raise NotImplementedError

    def grid_strip(self, data: "StripData", freq):
        """Grid the strip -> (buffer (nrows, nu, 2) f64, (nplanes, nrows, nu, 2) with w-stacking; weight sum (1,))."""
        raise NotImplementedError

    def mark_clean(self) -> None:
        """Pass A has consumed every strip row and the halo rows were zeroed."""
        raise NotImplementedError

    def pass_rows(self, grid, y0: int, y1: int, plane: int = 0):
        """Pass A over rows [y0, y1) of one plane's buffer -> H (npix_x / 4, y1 - y0, 4, 2); zeroes the rows."""
        raise NotImplementedError

    def pass_cols(self, H, i0: int, i1: int, norm=None):
        """Pass B + crop + grid correction (/ norm) of image rows [i0, i1) from H ((i1 - i0) / 4, nv, 4, 2)."""
        raise NotImplementedError

    def pass_cols_wplane(self, H, i0: int, i1: int, plane: int, first: bool, acc):
        """Pass B of one w plane with its w screen, added into acc (overwritten when `first`)."""
        raise NotImplementedError

    def finish_rows(self, acc, i0: int, i1: int, norm=None):
        """The final w and grid corrections of image rows [i0, i1) (acc, in place), / norm."""
        raise NotImplementedError

    def live_rows(self, h: int, plane: int = 0):
        """Bool over buffer rows [0, h) of `plane`: the rows that may hold a
        non-zero cell, when the backend knows them before pass A; None: it
        does not (the driver then scans pass A's output)."""
        return None

    def pass_rows_packed(self, grid, y0: int, y1: int, live, count: int, plane: int = 0):
        """Pass A keeping only the live rows (`live`: bool over [y0, y1) with
        `count` Trues) -> (npix_x / 4, count, 4, 2), the sparse all-to-all's
        send buffer. Default: packed after a dense pass A."""
        return _pack_live(self.pass_rows(grid, y0, y1, plane), live, count)

    def planes(self, buf):
        """The buffer of `grid_strip` as (nplanes, nrows, nu, 2): a view (2-D is the one-plane case)."""
        return buf[None] if self.nplanes == 1 else buf

    def wire(self, H):
        """Pass-A blocks as they cross the all-to-all: complex64 for the packed
        class (its own precision; half the bytes), complex128 otherwise."""
        return H.to(torch.float32) if self.single else H


_ADOPTED: dict = {}


def _adopt(backend) -> StripBackend:
    """`backend` as a StripBackend. The drivers used to take any object with
    the stages (and whichever optional members it chose to define); such an
    object keeps working: its class is given StripBackend as a last base, so
    what it defines stands and what it leaves out falls to the defaults."""
    if not isinstance(backend, StripBackend):
        cls = type(backend)
        if cls not in _ADOPTED:
            _ADOPTED[cls] = type(cls.__name__, (cls, StripBackend), {})
        backend.__class__ = _ADOPTED[cls]
    return backend


class HipStripBackend(StripBackend):
    """Per-rank stages on the current GPU through libcip_hip.so:
    cip_grid_tiles_strip (accumulating gridder) onto a buffer holding only the
    rank's strip + halo rows (`bind`: 1/N of the grid plus W - 1 rows instead
    of a full-size grid per rank), cip_strip_rows (pass A), cip_strip_cols
    (pass B + crop + correction). The buffer is kept between calls and left
    clean (pass A zeroes the rows it reads; the halo rows are zeroed after
    they are sent); an invert that fails in between leaves it marked dirty and
    the next `grid_strip` zeroes it first instead of trusting CIP_GRID_ZEROED.
    Unbound (rows=None) the buffer is the whole transposed grid.
    w-stacking parameters (nplanes > 1): the buffer holds the strip's rows of
    every w plane, (nplanes, nrows, nu, 2); pass A runs per plane, pass B per
    plane with the w screen into the rank's image rows (`pass_cols_wplane`),
    then `finish_rows` applies the final w and grid corrections.
    `single_precision_accumulation`: the packed class (complex64 visibilities;
    the reference call's float class), gridded into the same fp64 planes."""

    def __init__(self, params, pixsize_x: float, pixsize_y: float, npix_x: int, npix_y: int, device=None,
                 rows: Optional[tuple] = None, single_precision_accumulation: bool = False):
        require_gpu()
        self.params = params
        self.px, self.py = float(pixsize_x), float(pixsize_y)
        self.npix_x, self.npix_y = int(npix_x), int(npix_y)
        self.device = target_device(device)
        if not _lib.lib().cip_grid_layout(params, self.npix_x, self.npix_y):
            raise ValueError("strips need a grid in the pruned-FFT layout (power-of-two grids)")
        self.nplanes = int(params.nplanes) if int(params.do_wstacking) else 1
        self.single = bool(single_precision_accumulation)
        # the gridded strip's dirty-tile bits, written by every grid_strip call
        # (cip_grid_tiles_strip_mask: the call's own planner mask + the halo
        # tile rows); CIP_STRIP_MASK=0 runs pass A over every cell
        self.masked = os.environ.get("CIP_STRIP_MASK", "1") != "0"
        self._bits = None
        self._bits_valid = False
        self.rows = None
        self.grid = None
        self.dirty = False
        self._alloc((0, int(params.nv)) if rows is None else rows)

    def _alloc(self, rows):
        row0, nrows = int(rows[0]), int(rows[1])
        if not (0 <= row0 < int(self.params.nv) and 1 <= nrows <= int(self.params.nv)):
            raise ValueError("strip rows outside the grid")
        if self.rows != (row0, nrows):
            self.grid = None  # free the old buffer first
            shape = (nrows, int(self.params.nu), 2) if self.nplanes == 1 else (self.nplanes, nrows,
                                                                                 int(self.params.nu), 2)
            self.grid = torch.zeros(shape, dtype=torch.float64, device=self.device)
            self.rows = (row0, nrows)
            self.dirty = False

    def spawn(self) -> "HipStripBackend":
        return HipStripBackend(self.params, self.px, self.py, self.npix_x, self.npix_y, device=self.device,
                               rows=self.rows, single_precision_accumulation=self.single)

    def bind(self, layout: StripLayout, rank: int) -> "HipStripBackend":
        self._alloc(strip_buffer_rows(layout, rank))
        return self

    def grid_strip(self, data: StripData, freq):
        """Grid the strip's visibilities; returns (strip buffer (nrows, nu, 2) f64 - (nplanes, nrows, nu, 2)
        with w-stacking -, weight sum (1,) f64)."""
        if self.dirty:  # a previous invert did not finish: the buffer may hold partial sums
            self.grid.zero_()
        self.dirty = True
        self._bits_valid = False
        sumw = torch.zeros(1, dtype=torch.float64, device=self.device)
        ns = int(data.slice_uvw.shape[0])
        nu, nv = int(self.params.nu), int(self.params.nv)
        mask = self.masked and nu % 1024 == 0
        if mask:
            shape = (self.nplanes, nv // TILE, nu // TILE // 32)
            if self._bits is None or tuple(self._bits.shape) != shape:
                self._bits = torch.empty(shape, dtype=torch.int32, device=self.device)
        if ns or mask:
            # an empty strip still writes its mask (the halo rows it receives)
            vis_ptr, vis_code = vis_arg(data.vis)
            call(self.device, "cip_grid_tiles_strip_mask" if mask else "cip_grid_tiles_strip",
                 data.slice_uvw, data.chan_start, data.chan_stop, ns, freq, int(freq.shape[0]), vis_ptr, data.nvis,
                 vis_code, *wgt_arg(data.wgt), self.params, self.px, self.py, self.npix_x, self.npix_y,
                 self.rows[0], self.rows[1], _lib.CIP_GRID_ZEROED | (_lib.CIP_ACC_SINGLE if self.single else 0),
                 STREAM, self.grid, sumw, *((self._bits,) if mask else ()))
        self._bits_valid = mask
        return self.grid, sumw

    def mark_clean(self) -> None:
        self.dirty = False

    def pass_rows(self, grid, y0: int, y1: int, plane: int = 0):
        """Pass A over buffer rows [y0, y1) of w plane `plane` -> H (npix_x / 4, y1 - y0, 4, 2); zeroes the
        rows (only the dirty tiles' cells are read when the gridded strip's mask is known)."""
        H = torch.empty((self.npix_x // COL_BLOCK, y1 - y0, COL_BLOCK, 2), dtype=torch.float64, device=self.device)
        if self._bits_valid and self.dirty:
            call(self.device, "cip_strip_rows_masked", grid, self.params, self.npix_x, self.npix_y, int(y0), int(y1),
                 int(self.rows[0]), self._bits[plane], STREAM, H)
        else:
            call(self.device, "cip_strip_rows", grid, self.params, self.npix_x, self.npix_y, int(y0), int(y1),
                 STREAM, H)
        return H

    def pass_rows_packed(self, grid, y0: int, y1: int, live, count: int, plane: int = 0):
        """Pass A over buffer rows [y0, y1) keeping only the live rows (`live`:
        bool over them, as live_rows gives; `count` Trues) -> H (npix_x / 4,
        count, 4, 2): the sparse all-to-all's send buffer, written by pass A
        itself (cip_strip_rows_packed) instead of packed after it."""
        if not (self._bits_valid and self.dirty):
            return super().pass_rows_packed(grid, y0, y1, live, count, plane)
        slot = torch.cumsum(live.to(torch.int64), 0).sub_(1)
        slot = torch.where(live, slot, torch.full_like(slot, -1))
        H = torch.empty((self.npix_x // COL_BLOCK, count, COL_BLOCK, 2), dtype=torch.float64, device=self.device)
        call(self.device, "cip_strip_rows_packed", grid, self.params, self.npix_x, self.npix_y, int(y0), int(y1),
             int(self.rows[0]), self._bits[plane], slot, int(count), STREAM, H)
        return H

    def live_rows(self, h: int, plane: int = 0):
        """Buffer rows [0, h) of `plane` that may hold a non-zero cell (their
        tile row has a dirty tile in the gridded strip's mask), or None when
        no mask is known: pass A of every other row is exactly zero."""
        if not self._bits_valid:
            return None
        words = self._bits[plane]  # (nty, ntx / 32) int32
        tile_live = (words != 0).any(dim=1)
        rows = torch.remainder(torch.arange(self.rows[0], self.rows[0] + h, device=words.device), int(self.params.nv))
        return tile_live[rows // TILE]

    def pass_cols(self, H, i0: int, i1: int, norm=None):
        """Pass B for image rows [i0, i1) from H ((i1 - i0) / 4, nv, 4, 2)."""
        out = torch.empty((i1 - i0, self.npix_y), dtype=torch.float64, device=self.device)
        call(self.device, "cip_strip_cols", H, self.params, self.npix_x, self.npix_y, int(i0), int(i1), norm, STREAM,
             out)
        return out

    def pass_cols_wplane(self, H, i0: int, i1: int, plane: int, first: bool, acc):
        """Pass B of w plane `plane` for image rows [i0, i1) with its w screen, into acc ((i1 - i0), npix_y)
        f64 (overwritten when `first`)."""
        call(self.device, "cip_strip_cols_wplane", H, self.params, self.npix_x, self.npix_y, self.px, self.py,
             int(i0), int(i1), int(plane), int(bool(first)), STREAM, acc)
        return acc

    def finish_rows(self, acc, i0: int, i1: int, norm=None):
        call(self.device, "cip_strip_wfinal", acc, self.params, self.npix_x, self.npix_y, self.px, self.py, int(i0),
             int(i1), norm, STREAM)
        return acc


def _dist():
    """torch.distributed, imported on first use (its entry points are looked up per call)."""
    import torch.distributed as dist  # pylint: disable=import-outside-toplevel

    return dist


def _heights(layout: StripLayout) -> list:
    """Every rank's strip height (grid rows)."""
    return [layout.rows(r)[1] - layout.rows(r)[0] for r in range(layout.world)]


def _pack_live(H, live, count: int):
    """This rank's live pass-A rows, compacted: (nb, h, 4, 2) -> (nb, count,
    4, 2) (`live`: bool (h); count = its number of Trues). On the GPU one
    copy kernel (cip_strip_pack_rows); CPU tensors (the gloo tests' backend)
    take the torch form."""
    nb, h = int(H.shape[0]), int(H.shape[1])
    if H.device.type != "cuda":
        return H.index_select(1, torch.nonzero(live).reshape(-1))
    H = H.contiguous()
    slot = torch.cumsum(live.to(torch.int64), 0).sub_(1)
    slot = torch.where(live, slot, torch.full_like(slot, -1))
    out = torch.empty((nb, count) + tuple(H.shape[2:]), dtype=H.dtype, device=H.device)
    call(H.device, "cip_strip_pack_rows", H, nb, h, 2 * H.element_size(), slot, count, STREAM, out)
    return out


_ROW_MAPS: dict = {}


def _unpack_rows(recv, nb: int, layout: StripLayout, masks, dtype, stacked=None):
    """A receiver's pass-B input (nb, nv, 4, 2) from the flat received buffer:
    rank r's piece (nb, its live row count, 4, 2) holds its live rows
    (masks[r], bool over its strip rows; None: every row), in order; rows no
    rank sent are zero. One copy kernel (cip_strip_unpack_rows); its row map - the record
    of each grid row's block 0 and its source's row count - in a handful of
    vectorised ops (`stacked`: the ranks' masks as one (world, >= max rows)
    tensor, when the caller has it)."""
    dev = recv.device
    nv, world = layout.nv, layout.world
    hs = _heights(layout)
    if stacked is None:
        stacked = torch.zeros((world, max(hs)), dtype=torch.uint8, device=dev)
        for r, m in enumerate(masks):
            stacked[r, :hs[r]] = 1 if m is None else m.to(torch.uint8)
    M = stacked[:, :max(hs)].to(torch.int64)
    key = (tuple(layout.y_bounds), str(dev))
    maps = _ROW_MAPS.get(key)
    if maps is None:  # grid row -> (its rank, its row in the rank's strip), per layout
        rr = torch.repeat_interleave(torch.arange(world, device=dev), torch.tensor(hs, device=dev))
        y0s = torch.tensor([layout.rows(r)[0] for r in range(world)], device=dev)
        maps = (rr, torch.arange(nv, device=dev) - y0s[rr])
        if len(_ROW_MAPS) > 16:
            _ROW_MAPS.clear()
        _ROW_MAPS[key] = maps
    rr, jj = maps
    cnt = M.sum(dim=1)  # = counts, on the device (no host copies)
    base = (torch.cumsum(cnt, 0) - cnt) * nb
    rec = torch.where(M[rr, jj] != 0, torch.cumsum(M, dim=1).sub_(1)[rr, jj] + base[rr],
                      torch.full((nv,), -1, dtype=torch.int64, device=dev))
    stride = cnt[rr]
    H = torch.empty((nb, nv, COL_BLOCK, 2), dtype=dtype, device=dev)
    call(dev, "cip_strip_unpack_rows", recv, nb, nv, 2 * H.element_size(), rec, stride, STREAM, H)
    return H


def _assemble_H(recv, nb: int, layout: StripLayout, counts, masks):
    """_unpack_rows in torch index form, for CPU tensors (the gloo tests'
    backend): rank r's piece of `recv` is (nb, counts[r], 4, 2)."""
    sparse = any(m is not None for m in masks)
    H = (torch.zeros if sparse else torch.empty)((nb, layout.nv, COL_BLOCK, 2), dtype=recv.dtype, device=recv.device)
    for r, piece in enumerate(torch.split(recv, [nb * c * COL_BLOCK * 2 for c in counts])):
        y0, y1 = layout.rows(r)
        if masks[r] is None:
            H[:, y0:y1] = piece.reshape(nb, y1 - y0, COL_BLOCK, 2)
        elif counts[r]:
            H[:, y0 + torch.nonzero(masks[r]).reshape(-1)] = piece.reshape(nb, counts[r], COL_BLOCK, 2)
    return H


def _stack_masks(lives: Sequence, layout: StripLayout, allgather=None):
    """The ranks' live-row masks (`lives`, bool over each one's strip rows;
    with `allgather` this rank's only, the others' fetched by it) -> (stacked
    (world, max rows) uint8, counts, masks (bool per rank)); the counts are the
    all-to-all's split sizes (the one host wait)."""
    hs = _heights(layout)
    padded = []
    for live in lives:
        padded.append(torch.zeros(max(hs), dtype=torch.uint8, device=live.device))
        padded[-1][:live.shape[0]] = live.to(torch.uint8)
    if allgather is not None:
        padded = allgather(padded[0])
    stacked = torch.stack(padded)
    counts = [int(c) for c in stacked.sum(dim=1).tolist()]
    return stacked, counts, [padded[r][:hs[r]].to(torch.bool) for r in range(layout.world)]


class PendingGather:
    """A strip invert whose image-row gather is in flight
    (`invert_strips(..., gather_async=True)`): the collective runs on the
    communicator's stream while the caller goes on - e.g. with the next
    invert's gridding, which touches none of its buffers. `wait()` returns
    the image on `dst` (None elsewhere)."""

    def __init__(self, work, gathered, layout: StripLayout, rank: int, dst: int, image=None):
        self._work, self._gathered, self._layout = work, gathered, layout
        self._rank, self._dst, self._image = rank, dst, image
        self._done = work is None and gathered is None

    def wait(self):
        if not self._done:
            if self._work is not None:  # None: the gather was a blocking one
                self._work.wait()
            self._done = True
            if self._rank == self._dst:
                lay = self._layout
                self._image = torch.cat([g[:lay.image_rows(r)[1] - lay.image_rows(r)[0]]
                                         for r, g in enumerate(self._gathered)])
            self._gathered = None
        return self._image


class _DistExchange:
    """The strip invert's exchanges as torch.distributed collectives (RCCL, or
    gloo on CPU tensors): this process holds one rank, `mine` = [rank]. Every
    operation takes and returns one entry per rank in `mine`."""

    def __init__(self, layout: StripLayout, group, dst: int, gather_async: bool):
        dist = _dist()
        alone = not dist.is_available() or not dist.is_initialized()
        self.world = 1 if alone else dist.get_world_size(group)
        self.rank = 0 if alone else dist.get_rank(group)
        self.mine = [self.rank]
        self.layout, self.group, self.dst, self.gather_async = layout, group, dst, gather_async
        # diagnostic stage names: the live-row scan of pass A's output counts as
        # "rows", packing and unpacking as this rank's "alltoall"; the gather is
        # timed only where the rank waits for it
        self.stage_names = {"scan": "rows", "pack": "alltoall", "assemble": "alltoall",
                            "gather": "gather" if self.world > 1 and not gather_async else None}

    def halo(self, tails):
        """Send the halo rows to rank + 1 -> [those of rank - 1]."""
        dist = _dist()
        send = tails[0].contiguous()
        recv = torch.empty_like(send)
        ops = [dist.P2POp(dist.isend, send, (self.rank + 1) % self.world, self.group),
               dist.P2POp(dist.irecv, recv, (self.rank - 1) % self.world, self.group)]
        for w in dist.batch_isend_irecv(ops):
            w.wait()
        return [recv]

    def sum_weights(self, sums):
        _dist().all_reduce(sums[0], group=self.group)
        return sums[0]

    def live_masks(self, lives):
        def allgather(mine):
            allm = [torch.empty_like(mine) for _ in range(self.world)]
            _dist().all_gather(allm, mine, group=self.group)
            return allm

        return _stack_masks(lives, self.layout, allgather)

    def alltoall(self, i: int, sends, counts):
        """Rank s receives blocks [i0_s / 4, i1_s / 4) of every rank's sent rows -> the flat receive buffer."""
        nbs = [(b - a) // COL_BLOCK for a, b in zip(self.layout.x_bounds, self.layout.x_bounds[1:])]
        splits_in = [nb * counts[self.rank] * COL_BLOCK * 2 for nb in nbs]
        splits_out = [nbs[self.rank] * c * COL_BLOCK * 2 for c in counts]
        recv = torch.empty(sum(splits_out), dtype=sends[i].dtype, device=sends[i].device)
        _dist().all_to_all_single(recv, sends[i].reshape(-1), splits_out, splits_in, group=self.group)
        return recv

    def sent_bytes(self, i: int, send) -> int:
        """The bytes handed to the all-to-all."""
        return send.numel() * send.element_size()

    def gather(self, rows_imgs):
        """This rank's image rows -> the whole image on `dst` (None elsewhere); gather_async: a PendingGather."""
        rows_img, layout, rank, dst = rows_imgs[0], self.layout, self.rank, self.dst
        if self.world == 1:
            return PendingGather(None, None, layout, rank, dst, rows_img) if self.gather_async else rows_img
        # strips padded to the largest: gather needs equal sizes
        hmax = max(b - a for a, b in zip(layout.x_bounds, layout.x_bounds[1:]))
        if rows_img.shape[0] < hmax:
            rows_img = torch.cat([rows_img, rows_img.new_zeros((hmax - rows_img.shape[0], rows_img.shape[1]))])
        gathered = [torch.empty_like(rows_img) for _ in range(self.world)] if rank == dst else None
        work = _dist().gather(rows_img, gathered, dst=dst, group=self.group, async_op=self.gather_async)
        pending = PendingGather(work, gathered, layout, rank, dst)
        return pending if self.gather_async else pending.wait()


class _LocalExchange:
    """The same exchanges in memory: every rank is in this process (one
    device), `mine` = all of them; the network's part is untimed."""

    def __init__(self, layout: StripLayout):
        self.layout, self.world = layout, layout.world
        self.mine = list(range(self.world))
        self.stage_names = {"scan": None, "gather": None}

    def halo(self, tails):
        sent = [t.clone() for t in tails]
        return [sent[(r - 1) % self.world] for r in self.mine]

    def sum_weights(self, sums):
        sumw = sums[0].clone()
        for sw in sums[1:]:
            sumw = sumw + sw
        return sumw

    def live_masks(self, lives):
        return _stack_masks(lives, self.layout)

    def alltoall(self, i: int, sends, counts):  # pylint: disable=unused-argument
        i0, i1 = self.layout.image_rows(i)
        return torch.cat([snd[i0 // COL_BLOCK:i1 // COL_BLOCK].reshape(-1) for snd in sends])

    def sent_bytes(self, i: int, send) -> int:
        """The bytes bound for the other N - 1 ranks."""
        i0, i1 = self.layout.image_rows(i)
        return (send.numel() - send[i0 // COL_BLOCK:i1 // COL_BLOCK].numel()) * send.element_size()

    def gather(self, rows_imgs):
        return torch.cat(rows_imgs, dim=0)


class _Clock:
    """The diagnostic stage times: `clock(i, name, fn)` runs fn() and, with
    `stages` (one dict per rank in the process), adds its synchronised seconds
    to stages[i][name]. `laps` (the distributed driver): a stage lasts from the
    end of the one before it, so whatever runs between two of them - the
    collectives - counts with the later. Without `stages` it only calls fn."""

    def __init__(self, stages, device, laps: bool, names: dict):
        self.stages, self.laps, self.names = stages, laps, names
        self.device = device if device is not None and torch.device(device).type == "cuda" else None
        self.last = time.perf_counter()

    def _now(self) -> float:
        if self.device is not None:
            torch.cuda.synchronize(self.device)
        return time.perf_counter()

    def __call__(self, i: int, name: str, fn):
        if self.stages is None:
            return fn()
        t0 = self.last if self.laps else self._now()
        out = fn()
        self.last = self._now()
        self.add(i, self.names.get(name, name), self.last - t0)
        return out

    def add(self, i: int, name, amount) -> None:
        if self.stages is not None and name is not None:
            self.stages[i][name] = self.stages[i].get(name, 0) + amount

    def idle(self, i: int, name: str) -> None:
        """A stage with nothing to do (one strip): laps still report it."""
        if self.laps:
            self(i, name, lambda: None)


def _pass_a(ranks, grids, plane: int, last: bool, ex, clock: _Clock, sparse: bool):
    """Pass A of one plane on every rank in the process -> (sends, counts,
    masks, stacked): sends[i] is rank ex.mine[i]'s all-to-all send buffer
    (npix_x / 4, counts[r], 4, 2) on the wire. A sparse exchange sends only
    the rows that can be non-zero (masks[r]; a row whose grid row was empty
    transforms to exact zeros): a backend that knows them before pass A has it
    write the packed buffer; otherwise pass A runs dense, its output is
    scanned and packed. Dense: every row (masks None). One strip: pass A's
    output as it is. The `last` plane's pass A leaves the buffer clean."""
    hs = _heights(ex.layout)

    def run(i, fn):
        H = clock(i, "rows", fn)
        if last:
            ranks[i].mark_clean()
        return H

    sparse = sparse and ex.world > 1
    known = [ranks[i].live_rows(hs[r], plane) if sparse else None for i, r in enumerate(ex.mine)]
    Hs = [run(i, lambda: ranks[i].pass_rows(grids[i], 0, hs[r], plane=plane)) if known[i] is None else None
          for i, r in enumerate(ex.mine)]
    if ex.world == 1:
        return Hs, None, None, None
    if not sparse:
        return [ranks[i].wire(H) for i, H in enumerate(Hs)], hs, [None] * ex.world, None
    lives = [lv if H is None else clock(i, "scan", lambda: (H != 0).reshape(H.shape[0], H.shape[1], -1).any(dim=2)
                                        .any(dim=0)) for i, (H, lv) in enumerate(zip(Hs, known))]
    stacked, counts, masks = ex.live_masks([lv.to(torch.bool) for lv in lives])
    sends = []
    for i, r in enumerate(ex.mine):
        if Hs[i] is None:
            sends.append(run(i, lambda: ranks[i].wire(
                ranks[i].pass_rows_packed(grids[i], 0, hs[r], masks[r], counts[r], plane=plane))))
        else:
            H = ranks[i].wire(Hs[i])
            sends.append(clock(i, "pack", lambda: _pack_live(H, masks[r], counts[r])))
    return sends, counts, masks, stacked


def _invert(datas, freq, layout: StripLayout, ranks, ex, clock: _Clock, sparse: bool):
    """The strip invert of the ranks in this process: ranks[i] is the bound
    backend of rank ex.mine[i], datas[i] its strip, `ex` the exchange between
    all ranks. 2-D is the one-plane case of w-stacking; only pass B differs
    (pass_cols with the norm; pass_cols_wplane per plane, then finish_rows)."""
    world, mine = ex.world, ex.mine
    local = range(len(mine))
    hs = _heights(layout)
    grids, sums = [None] * len(mine), [None] * len(mine)
    for i in local:
        buf, sums[i] = clock(i, "grid", lambda: ranks[i].grid_strip(datas[i], freq))
        grids[i] = ranks[i].planes(buf)
    nplanes = int(grids[0].shape[0])
    sumw = sums[0]
    if world > 1:
        # halo: buffer rows [h, h + W - 1) = the grid rows past the strip ->
        # the next rank, added to its first rows (every plane's at once)
        tails = [grids[i][:, hs[r]:hs[r] + layout.halo] for i, r in enumerate(mine)]
        heads = ex.halo(tails)
        sumw = ex.sum_weights(sums)
        for tail in tails:
            tail.zero_()
        for i in local:
            clock(i, "halo", lambda: grids[i][:, :layout.halo].add_(heads[i]))
    else:
        clock.idle(0, "halo")
    rows = [layout.image_rows(r) for r in mine]
    outs = [None if nplanes == 1 else torch.empty((i1 - i0, ranks[i].npix_y), dtype=torch.float64,
                                                  device=grids[i].device) for i, (i0, i1) in enumerate(rows)]
    for p in range(nplanes):
        sends, counts, masks, stacked = _pass_a(ranks, [g[p] for g in grids], p, p == nplanes - 1, ex, clock, sparse)
        for i, (i0, i1) in enumerate(rows):
            if world > 1:
                clock.add(i, "a2a_send_bytes", ex.sent_bytes(i, sends[i]))
                recv, nb = ex.alltoall(i, sends, counts), (i1 - i0) // COL_BLOCK
                Hm = clock(i, "assemble", lambda: (
                    _unpack_rows(recv, nb, layout, masks, recv.dtype, stacked) if recv.is_cuda else
                    _assemble_H(recv, nb, layout, counts, masks)).to(torch.float64))
            else:
                Hm = sends[i]
                clock.idle(i, "alltoall")
            if nplanes == 1:
                outs[i] = clock(i, "cols", lambda: ranks[i].pass_cols(Hm, i0, i1, norm=sumw))
            else:
                clock(i, "cols", lambda: ranks[i].pass_cols_wplane(Hm, i0, i1, p, p == 0, outs[i]))
    if nplanes > 1:
        for i, (i0, i1) in enumerate(rows):
            clock(i, "final", lambda: ranks[i].finish_rows(outs[i], i0, i1, norm=sumw))
    return clock(0, "gather", lambda: ex.gather(outs))


def invert_strips(data: StripData, freq, layout: StripLayout, backend: StripBackend, *, dst: int = 0, group=None,
                  stages: Optional[dict] = None, sparse: bool = True, gather_async: bool = False):
    """This rank's share of the strip-distributed invert (torch.distributed
    initialised, one rank per strip). Returns the normalised dirty image
    (npix_x, npix_y) on `dst`, None elsewhere. Collectives: one point-to-point
    halo exchange with the ring neighbours, one all-to-all of the pass-A
    blocks, a scalar all-reduce of the weight sum, a gather of image rows.
    The backend is bound to this rank's strip + halo rows (`strip_buffer_rows`).
    `sparse` (default): the all-to-all carries only the rows of the pass-A
    output that can be non-zero (after an all-gather of the live-row masks).
    `gather_async`: return a `PendingGather` at once (the image-row gather in
    flight on the communicator's stream, e.g. beside the next invert's
    gridding); `.wait()` gives the image.
    `stages` (a dict, diagnostic): each stage is synchronised and its seconds
    added under its name (grid, halo, rows, alltoall, cols, final, gather), and
    the all-to-all's bytes sent by this rank under a2a_send_bytes."""
    backend = _adopt(backend)
    ex = _DistExchange(layout, group, dst, gather_async)
    clock = _Clock(None if stages is None else [stages], backend.device, True, ex.stage_names)
    if ex.world != layout.world:
        raise ValueError("the layout was planned for another number of ranks")
    backend.bind(layout, ex.rank)
    return _invert([data], freq, layout, [backend], ex, clock, sparse)


def invert_strips_local(datas: Sequence[StripData], freq, layout: StripLayout, backend: StripBackend,
                        stages: Optional[list] = None, sparse: bool = True):
    """All ranks' stages in ONE process on one device, the exchanges done in
    memory (the single-GPU check of the decomposition and its kernels, and the
    per-rank cost breakdown of the N-GPU split): the distributed invert's own
    driver over every rank. Rank r's stages run on its own strip + halo buffer
    (`backend.spawn()` per rank, kept as `backend.ranks`). `stages` (a list,
    diagnostic): filled with one dict per rank of synchronised seconds (grid,
    halo, rows, pack, assemble, cols, final) and the bytes the rank would send
    to the others in the all-to-all (a2a_send_bytes). Returns the normalised
    dirty image (npix_x, npix_y)."""
    world, backend = layout.world, _adopt(backend)
    if len(datas) != world:
        raise ValueError("one StripData per strip")
    if stages is not None:
        stages[:] = [{} for _ in range(world)]
    if not backend.ranks or len(backend.ranks) != world:
        backend.ranks = [backend] + [_adopt(backend.spawn()) for _ in range(world - 1)]
    for r in range(world):
        backend.ranks[r].bind(layout, r)
    ex = _LocalExchange(layout)
    clock = _Clock(stages, backend.device, False, ex.stage_names)
    return _invert(datas, freq, layout, backend.ranks, ex, clock, sparse)

