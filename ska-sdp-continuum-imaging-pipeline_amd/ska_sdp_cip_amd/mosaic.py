"""
Facet mosaicking: facet images, each on the tangent plane at its own centre
(`continuum.continuum_invert`), resampled onto one wide-field plane at the
phase centre (`cip_mosaic_add`, `cip_mosaic_finish`), on the GPU.

The operator is defined exactly in include/cip_mosaic.h. The facet frames are
rotated against the output plane, so an output pixel is mapped into the facet
(q = Q^T s) and the facet is interpolated there with 2 half x 2 half taps of a
sinc windowed by the gridder's exponential of a semicircle, normalised to sum
1. Overlapping facets are blended with the weight w (1 inside, a linear ramp of
`feather` pixels towards the trimmed edge): the mosaic is sum(w val) / sum(w).
With `nscale` the values are multiplied by n' / n, which turns the 1 / n' of
w-stacked facet images into the 1 / n of the mosaic's own plane.

`facet_layout` (host-only) places the facets so that their valid regions cover
the plane; `MosaicAccumulator` follows `accumulate.GridAccumulator`: `add`
facets in any number of calls, `reduce` over ranks, `finish` once.
"""

from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._call import STREAM, call, check_array, require_gpu, target_device

try:
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None

MAX_HALF = _lib.MOSAIC_MAX_HALF


def mosaic_beta(half: int, nu_max: float) -> float:
    """The window parameter for images band-limited to `nu_max` cycles per
    facet pixel (0 <= nu_max < 0.5): pi half (1 - 2 nu_max). Host-only."""
    out = ctypes.c_double(0.0)
    _lib.check(_lib.lib().cip_mosaic_beta(int(half), float(nu_max), ctypes.byref(out)))
    return float(out.value)


def mosaic_taps(half: int, beta: float, frac: float) -> np.ndarray:
    """The 2 half normalised taps of one axis at the fractional position `frac`
    in [0, 1), for the pixels floor(x) - half + 1 .. floor(x) + half, as the
    kernel forms them (`cip_mosaic_taps`). Host-only."""
    half = int(half)
    out = np.zeros(2 * max(half, 1), dtype=np.float64)
    _lib.check(_lib.lib().cip_mosaic_taps(half, float(beta), float(frac),
                                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return out


def _pair(v, default, what):
    """A scalar or an (x, y) pair of positive finite floats."""
    if v is None:
        v = default
    x, y = (v, v) if np.isscalar(v) else v
    x, y = float(x), float(y)
    if not (math.isfinite(x) and math.isfinite(y) and x > 0.0 and y > 0.0):
        raise ValueError(f"{what} must be finite and > 0, got {v}")
    return x, y


def _check_plane(nx, ny, px, py, what):
    """Dimensions >= 1 and every corner of the plane inside the unit disc."""
    if int(nx) != nx or int(ny) != ny or nx < 1 or ny < 1:
        raise ValueError(f"{what}: image dimensions must be integers >= 1, got {nx} x {ny}")
    lc = max(nx // 2, nx - 1 - nx // 2) * px
    mc = max(ny // 2, ny - 1 - ny // 2) * py
    if not lc * lc + mc * mc < 1.0:
        raise ValueError(f"{what}: an output corner has l^2 + m^2 >= 1")


def _check_window(half, trim, what):
    if int(half) != half or not 2 <= half <= MAX_HALF:
        raise ValueError(f"{what}: half must be an integer in 2 .. {MAX_HALF}, got {half}")
    if int(trim) != trim or trim < 0:
        raise ValueError(f"{what}: trim must be an integer >= 0, got {trim}")


def _margins(l, m, centre, fn, fp, half, trim):  # noqa: E741
    """(dx, dy, q2) of include/cip_mosaic.h for the directions (l, m) (arrays)
    in the facet at `centre`: dx, dy >= 0 and q2 > 0 mean a valid pixel."""
    l0, m0 = centre
    n0 = math.sqrt((1.0 - l0 * l0) - m0 * m0)
    c = 1.0 / (1.0 + n0)
    a01 = -((c * l0) * m0)
    n = np.sqrt((1.0 - l * l) - m * m)
    x = ((1.0 - (c * l0) * l0) * l + a01 * m - l0 * n) / fp[0] + fn[0] // 2
    y = (a01 * l + (1.0 - (c * m0) * m0) * m - m0 * n) / fp[1] + fn[1] // 2
    lo = trim + half - 1
    return (np.minimum(x - lo, fn[0] - 1 - trim - half - x), np.minimum(y - lo, fn[1] - 1 - trim - half - y),
            (l0 * l + m0 * m) + n0 * n)


def facet_layout(nx: int, ny: int, px: float, facet_pixels: int, *, half: int = 6, trim: int = 0,
                 py: Optional[float] = None, facet_pixel_size=None) -> list:
    """
    Centres (l0, m0), row-major in (x, y), of a regular grid of facets of
    `facet_pixels`^2 pixels whose valid regions (include/cip_mosaic.h,
    for this `half` and `trim`) cover every pixel of the (nx, ny) output plane
    with pixel sizes (px, py = px). `facet_pixel_size`: the facets' pixel size,
    a scalar or a pair (default: the plane's). Host-only.

    The plane is cut into ncx x ncy cells of pixels, equal to a pixel, with a
    facet centred on each cell; the counts start at what the valid span of a
    facet allows and grow until every pixel on every cell's perimeter is valid
    in its facet. A facet's valid region is the
    one-to-one image of a rectangle, so it has no holes, and its edges bend over
    the scale of the facet, not of a pixel: a cell whose perimeter pixels are
    valid is valid throughout.
    """
    px, py = _pair((px, px if py is None else py), None, "pixel sizes")
    _check_plane(nx, ny, px, py, "facet_layout")
    _check_window(half, trim, "facet_layout")
    fp = _pair(facet_pixel_size, (px, py), "facet pixel sizes")
    if int(facet_pixels) != facet_pixels or facet_pixels < 2 * (trim + half):
        raise ValueError(f"facet_layout: facets of {facet_pixels} pixels hold no valid pixel at half {half}, trim {trim}")
    nx, ny, fn = int(nx), int(ny), (int(facet_pixels), int(facet_pixels))
    span = facet_pixels - 2 * (trim + half)  # hi - lo, in facet pixels
    ncx = max(1, math.ceil(nx * px / ((span + 1) * fp[0])))
    ncy = max(1, math.ceil(ny * py / ((span + 1) * fp[1])))
    while True:
        ex, ey = np.linspace(0, nx, ncx + 1).round().astype(int), np.linspace(0, ny, ncy + 1).round().astype(int)
        centres, bad_x, bad_y = [], False, False
        for a in range(ncx):
            for b in range(ncy):
                ia, ib, ja, jb = ex[a], ex[a + 1] - 1, ey[b], ey[b + 1] - 1
                centre = (float(((ia + ib) / 2.0 - nx // 2) * px), float(((ja + jb) / 2.0 - ny // 2) * py))
                centres.append(centre)
                i = np.concatenate([np.arange(ia, ib + 1), np.arange(ia, ib + 1), np.full(jb - ja + 1, ia),
                                    np.full(jb - ja + 1, ib)])
                j = np.concatenate([np.full(ib - ia + 1, ja), np.full(ib - ia + 1, jb), np.arange(ja, jb + 1),
                                    np.arange(ja, jb + 1)])
                dx, dy, q2 = _margins((i - nx // 2) * px, (j - ny // 2) * py, centre, fn, fp, half, trim)
                bad_x |= bool((dx < 0).any())
                bad_y |= bool((dy < 0).any() or (q2 <= 0).any())
        if not (bad_x or bad_y):
            return centres
        ncx, ncy = ncx + bad_x, ncy + bad_y
        if ncx > nx or ncy > ny:
            raise ValueError("facet_layout: these facets cannot cover the plane")


class MosaicAccumulator:
    """
    The numerator (nplane, nx, ny) and the weight sum (nx, ny) of a mosaic,
    resident in HBM, that facets are added to.

    The plane and the interpolation are fixed at construction: `half` taps
    either side and either `nu_max` (the band limit of the facet images in
    cycles per facet pixel; beta = `mosaic_beta(half, nu_max)`) or `beta`
    itself; `trim` facet edge pixels are ignored, `feather` pixels blend
    overlapping facets, `nscale` multiplies by n' / n (w-stacked facets).
    `add` runs on the current stream and returns at once; `reduce` sums over
    the ranks of an initialised torch.distributed group; `finish` divides,
    writes `fill` where no facet reached and returns (images, n_uncovered).
    """

    def __init__(self, nx: int, ny: int, px: float, py: float, nplane: int = 1, *, half: int = 6,
                 nu_max: Optional[float] = None, beta: Optional[float] = None, trim: int = 0, feather: float = 0.0,
                 nscale: bool = False, device=None):
        self.px, self.py = _pair((px, py), None, "pixel sizes")
        _check_plane(nx, ny, self.px, self.py, "MosaicAccumulator")
        _check_window(half, trim, "MosaicAccumulator")
        if int(nplane) != nplane or nplane < 1:
            raise ValueError(f"MosaicAccumulator: nplane must be an integer >= 1, got {nplane}")
        if (nu_max is None) == (beta is None):
            raise ValueError("MosaicAccumulator: give exactly one of nu_max and beta")
        self.beta = mosaic_beta(half, nu_max) if beta is None else float(beta)
        if not (math.isfinite(self.beta) and self.beta >= 0.0):
            raise ValueError(f"MosaicAccumulator: beta must be finite and >= 0, got {beta}")
        self.feather = float(feather)
        if not (math.isfinite(self.feather) and self.feather >= 0.0):
            raise ValueError(f"MosaicAccumulator: feather must be finite and >= 0, got {feather}")
        self.nx, self.ny, self.nplane, self.half, self.trim = int(nx), int(ny), int(nplane), int(half), int(trim)
        self.flags = _lib.MOSAIC_NSCALE if nscale else 0
        require_gpu()
        self.device = target_device(device)
        self.num = torch.zeros((self.nplane, self.nx, self.ny), dtype=torch.float64, device=self.device)
        self.wsum = torch.zeros((self.nx, self.ny), dtype=torch.float64, device=self.device)
        self.num_facets = 0
        self._done = False

    def _check(self):
        if self._done:
            raise RuntimeError("finish() consumed the numerator; make a new MosaicAccumulator")

    def add(self, facet_images, l0: float, m0: float, facet_pixel_size=None) -> None:
        """Add one facet: `facet_images` (nplane, fnx, fny) float64 on the
        accumulator's device ((fnx, fny) when nplane is 1), on the tangent
        plane at (l0, m0) with pixel size `facet_pixel_size` (a scalar or a
        pair; default: the plane's)."""
        self._check()
        if facet_images.dim() == 2:
            facet_images = facet_images.unsqueeze(0)
        if facet_images.dim() != 3 or facet_images.shape[0] != self.nplane:
            raise ValueError(f"facet_images must be ({self.nplane}, fnx, fny), got {tuple(facet_images.shape)}")
        check_array(facet_images, (torch.float64,), None, self.device, "facet_images")
        fpx, fpy = _pair(facet_pixel_size, (self.px, self.py), "facet pixel sizes")
        g = _lib.MosaicGeom(self.nx, self.ny, self.px, self.py, int(facet_images.shape[1]),
                            int(facet_images.shape[2]), fpx, fpy, self.half, self.flags, self.beta, self.trim,
                            self.feather)
        call(self.device, "cip_mosaic_add", ctypes.byref(g), facet_images, self.nplane, float(l0), float(m0), STREAM,
             self.num, self.wsum)
        self.num_facets += 1

    def reduce(self) -> None:
        """Sum the numerator and the weight sum over the ranks of the default
        torch.distributed group (nothing without an initialised group)."""
        self._check()
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.num)
            dist.all_reduce(self.wsum)

    def finish(self, fill: float = float("nan")):
        """(images (nplane, nx, ny), n_uncovered): the numerator over the
        weight sum, in place, `fill` on the n_uncovered pixels no facet reached."""
        self._check()
        missed = ctypes.c_int64(0)
        call(self.device, "cip_mosaic_finish", self.num, self.wsum, self.nplane, self.nx, self.ny, float(fill),
             STREAM, ctypes.byref(missed))
        self._done = True
        return self.num, int(missed.value)


def device_mosaic(facet_images: Sequence, centres: Sequence, nx: int, ny: int, px: float, py: Optional[float] = None,
                  *, facet_pixel_size=None, fill: float = float("nan"), **kwargs):
    """
    The mosaic of `facet_images` (one device tensor (nplane, fnx, fny) or
    (fnx, fny) per facet, or one stacked tensor) at `centres` ((l0, m0) each)
    on the (nx, ny) plane of pixel sizes (px, py = px). The keywords are
    `MosaicAccumulator`'s. Returns (images, n_uncovered); the images are
    (nx, ny) for 2-D facets, else (nplane, nx, ny).
    """
    if len(facet_images) != len(centres) or len(centres) == 0:
        raise ValueError("device_mosaic: need one centre per facet image and at least one facet")
    first = facet_images[0]
    acc = MosaicAccumulator(nx, ny, px, px if py is None else py, 1 if first.dim() == 2 else int(first.shape[0]),
                            device=first.device if torch is not None and torch.is_tensor(first) else None, **kwargs)
    for img, (l0, m0) in zip(facet_images, centres):
        acc.add(img, l0, m0, facet_pixel_size)
    out, missed = acc.finish(fill)
    return (out[0] if first.dim() == 2 else out), missed


__all__ = ["MAX_HALF", "MosaicAccumulator", "device_mosaic", "facet_layout", "mosaic_beta", "mosaic_taps"]
