"""
The numpy statement of facet mosaicking (include/cip_mosaic.h), vectorised
over the output plane: the geometry q = Q^T s, the normalised windowed-sinc
taps, the validity weight, `add` (num += w val, wsum += w) and `finish`. The
GPU tests compare cip_mosaic_add / cip_mosaic_finish against it; the
arithmetic is written in the header's order, one rounded fp64 operation at a
time, so the two differ by the rounding of sqrt / exp / sin and by fused
multiply-adds in the tap sums only.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

NSCALE = 1  # CIP_MOSAIC_NSCALE


@dataclass
class Geom:
    """Mirror of cip_mosaic_geom."""

    nx: int
    ny: int
    px: float
    py: float
    fnx: int
    fny: int
    fpx: float
    fpy: float
    half: int = 6
    beta: float = 0.0
    trim: int = 0
    feather: float = 0.0
    flags: int = 0


def beta_rule(half: int, nu_max: float) -> float:
    """beta = pi half (1 - 2 nu_max): the window's spectral half-width
    beta / (2 pi half) fills the guard band 0.5 - nu_max."""
    return np.pi * half * (1.0 - 2.0 * nu_max)


def rotation_t(l0: float, m0: float) -> np.ndarray:
    """Q^T in closed form (rows q0, q1, q2 of the header); Q is
    oracle.facet_rotation(l0, m0)."""
    n0 = np.sqrt((1.0 - l0 * l0) - m0 * m0)
    c = 1.0 / (1.0 + n0)
    a01 = -((c * l0) * m0)
    return np.array([[1.0 - (c * l0) * l0, a01, -l0],
                     [a01, 1.0 - (c * m0) * m0, -m0],
                     [l0, m0, n0]])


def coords(g: Geom, l0: float, m0: float):
    """(x, y, q2, n): continuous facet pixel coordinates, the facet-plane n and
    the output-plane n of every output pixel, each (nx, ny)."""
    qt = rotation_t(l0, m0)
    l = ((np.arange(g.nx) - g.nx // 2) * g.px)[:, None]  # noqa: E741
    m = ((np.arange(g.ny) - g.ny // 2) * g.py)[None, :]
    n = np.sqrt((1.0 - l * l) - m * m)
    q0 = (qt[0, 0] * l + qt[0, 1] * m) - l0 * n
    q1 = (qt[1, 0] * l + qt[1, 1] * m) - m0 * n
    q2 = (l0 * l + m0 * m) + qt[2, 2] * n
    return q0 / g.fpx + (g.fnx // 2), q1 / g.fpy + (g.fny // 2), q2, n


def sinpi_frac(f):
    """sin(pi f) for 0 <= f < 1, folded onto [0, 1/2] (1 - f is exact there),
    so it is exactly 0 at f = 0 and has a relative error of an ulp."""
    f = np.asarray(f, dtype=np.float64)
    return np.sin(np.pi * np.where(f > 0.5, 1.0 - f, f))


def order(half: int) -> list:
    """The order in which the 2 half terms of a tap sum are added: from the
    outermost pair inwards (q = 0, 2 half - 1, 1, 2 half - 2, ...)."""
    return [q for pair in zip(range(half), range(2 * half - 1, half - 1, -1)) for q in pair]


def taps(half: int, beta: float, frac) -> np.ndarray:
    """The 2 half normalised taps h(frac - k), k = -half + 1 .. half, on the
    last axis."""
    frac = np.asarray(frac, dtype=np.float64)
    s = sinpi_frac(frac)
    h = np.empty(frac.shape + (2 * half,))
    for q, k in enumerate(range(-half + 1, half + 1)):
        t = frac - k
        u = t / half
        e = np.exp(beta * (np.sqrt(np.maximum(0.0, 1.0 - u * u)) - 1.0))
        sgn = -1.0 if k % 2 else 1.0
        with np.errstate(invalid="ignore", divide="ignore"):
            v = ((sgn * s) * e) / (np.pi * t)
        v = np.where(t == 0.0, 1.0, v)
        v = np.where(np.abs(t) >= half, 0.0, v)
        h[..., q] = v
    total = np.zeros(frac.shape)
    for q in order(half):
        total = total + h[..., q]
    return h / total[..., None]


def bounds(g: Geom):
    """(lo_x, hi_x, lo_y, hi_y) of the valid facet coordinates."""
    return (g.trim + g.half - 1, g.fnx - 1 - g.trim - g.half, g.trim + g.half - 1, g.fny - 1 - g.trim - g.half)


def margins(g: Geom, x, y):
    """(dx, dy): the distance of (x, y) inside the valid rectangle (< 0 outside)."""
    lo_x, hi_x, lo_y, hi_y = bounds(g)
    return np.minimum(x - lo_x, hi_x - x), np.minimum(y - lo_y, hi_y - y)


def weight(g: Geom, x, y, q2):
    dx, dy = margins(g, x, y)
    w = np.minimum(1.0, (dx + 1.0) / (g.feather + 1.0)) * np.minimum(1.0, (dy + 1.0) / (g.feather + 1.0))
    return np.where((dx >= 0) & (dy >= 0) & (q2 > 0), w, 0.0)


def add(g: Geom, facet, l0: float, m0: float, num, wsum) -> None:
    """num (nplane, nx, ny) += w val, wsum (nx, ny) += w, in place."""
    facet = np.asarray(facet, dtype=np.float64).reshape(-1, g.fnx, g.fny)
    x, y, q2, n = coords(g, l0, m0)
    w = weight(g, x, y, q2)
    on = w > 0
    if not on.any():
        return
    xs, ys = x[on], y[on]
    ix, iy = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    tx, ty = taps(g.half, g.beta, xs - ix), taps(g.half, g.beta, ys - iy)
    scale = (q2[on] / n[on]) if g.flags & NSCALE else None
    offs = np.arange(-g.half + 1, g.half + 1)
    for p in range(facet.shape[0]):
        val = np.zeros(xs.shape)
        for a in order(g.half):
            row = np.zeros(xs.shape)
            for b in order(g.half):
                row = row + ty[:, b] * facet[p, ix + offs[a], iy + offs[b]]
            val = val + tx[:, a] * row
        if scale is not None:
            val = val * scale
        num[p][on] += w[on] * val
    wsum[on] += w[on]


def finish(num, wsum, fill=np.nan):
    """(image(s), n_uncovered): num / wsum where wsum > 0, `fill` elsewhere."""
    on = wsum > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(on, num / wsum, fill)
    return out, int((~on).sum())


def mosaic(g: Geom, facets, centres, fill=np.nan):
    """One-shot: facets (nfacet, nplane, fnx, fny) at `centres` onto the plane."""
    facets = [np.asarray(f, dtype=np.float64).reshape(-1, g.fnx, g.fny) for f in facets]
    num = np.zeros((facets[0].shape[0], g.nx, g.ny))
    wsum = np.zeros((g.nx, g.ny))
    for f, (l0, m0) in zip(facets, centres):
        add(g, f, l0, m0, num, wsum)
    return finish(num, wsum, fill)
