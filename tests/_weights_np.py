"""
The numpy statement of the imaging-weights operator of include/cip.h
(`cip_weight_*`, `cip_imaging_weights`): the yardstick of the weights tests.

Every step is the header's, in its order: the field-of-view cell of a
visibility in fp64 (numpy never contracts a product and a sum), the Hermitian
fold to v >= 0, the fixed-point weight q(w) = rint(ldexp(w, shift)), the
density by `np.add.at` on int64, the statistics with `math.fsum`, and the two
weighting formulas.
"""

import math

import numpy as np

C = 299792458.0
UNIFORM, BRIGGS = 1, 2


def ceil_log2(v):
    """The least integer e with v <= 2^e (v > 0)."""
    m, e = math.frexp(v)
    return e - 1 if m == 0.5 else e


def grid_shift(wmax, nvis_max):
    """shift = 62 - B - E of cip_weight_grid_init."""
    b = 0
    while (1 << b) < nvis_max:
        b += 1
    return 62 - b - ceil_log2(float(wmax))


class Grid:
    """cip_weight_grid."""

    def __init__(self, npix_x, npix_y, pixsize_x, pixsize_y, wmax, nvis_max):
        self.npix_x, self.npix_y = int(npix_x), int(npix_y)
        self.hx, self.hy = self.npix_x // 2, self.npix_y // 2
        self.SX = float(self.npix_x) * float(pixsize_x)
        self.SY = float(self.npix_y) * float(pixsize_y)
        self.wmax = float(wmax)
        self.shift = grid_shift(wmax, nvis_max)
        self.quantum = math.ldexp(1.0, -self.shift)
        self.shape = (2 * self.hx + 1, self.hy + 1)


def cells(uvw, freq, grid):
    """(iu, iv, inside) per (row, channel); iu, iv are int64 and 0 where outside."""
    uvw = np.asarray(uvw, dtype=np.float64)
    wi = np.asarray(freq, dtype=np.float64) / C
    su = uvw[:, 0] * grid.SX
    sv = uvw[:, 1] * grid.SY
    with np.errstate(invalid="ignore", over="ignore"):
        x = wi[None, :] * su[:, None]
        y = wi[None, :] * sv[:, None]
        fold = (y < 0) | ((y == 0) & (x < 0))
        x = np.where(fold, -x, x)
        y = np.where(fold, -y, y)
        fx = np.floor(x + 0.5)
        fy = np.floor(y + 0.5)
        inside = np.isfinite(x) & np.isfinite(y) & (np.abs(fx) <= grid.hx) & (fy <= grid.hy)
    iu = np.where(inside, fx, 0.0).astype(np.int64)
    iv = np.where(inside, fy, 0.0).astype(np.int64)
    return iu, iv, inside


def _weights64(wgt, nrow, nchan):
    if wgt is None:
        return np.ones((nrow, nchan), dtype=np.float64)
    return np.asarray(wgt).astype(np.float64)


def quantise(w64, grid):
    """q(w): round-half-even of w 2^shift."""
    return np.rint(np.ldexp(w64, grid.shift)).astype(np.int64)


def density(uvw, freq, wgt, grid, density_io=None):
    """Adds onto density_io (int64, grid.shape; None: zeros). Returns (density, counts[3])."""
    nrow, nchan = np.asarray(uvw).shape[0], np.asarray(freq).shape[0]
    w = _weights64(wgt, nrow, nchan)
    iu, iv, inside = cells(uvw, freq, grid)
    with np.errstate(invalid="ignore"):
        bad = (w < 0) | np.isnan(w) | (w > grid.wmax)
        pos = (w > 0) & ~bad
    add = pos & inside
    dens = np.zeros(grid.shape, dtype=np.int64) if density_io is None else density_io
    np.add.at(dens, (iu[add] + grid.hx, iv[add]), quantise(w[add], grid))
    counts = np.array([add.sum(), (pos & ~inside).sum(), bad.sum()], dtype=np.int64)
    return dens, counts


def stats(dens, grid):
    """(sum_w, sum_d2, n_cells): the integer sum is exact, sum_d2 is the fsum of the rounded squares."""
    sum_w = float(int(dens.sum(dtype=np.int64))) * grid.quantum
    d = dens.astype(np.float64) * grid.quantum
    return sum_w, math.fsum((d * d).ravel().tolist()), int(np.count_nonzero(dens))


def briggs_f2(robust, sum_w, sum_d2):
    t = 5.0 * math.pow(10.0, -robust)
    return (t * t) / (sum_d2 / sum_w)


def apply(uvw, freq, wgt, dens, grid, mode, f2, out_dtype):
    """The imaging weights, rounded once to out_dtype."""
    nrow, nchan = np.asarray(uvw).shape[0], np.asarray(freq).shape[0]
    w = _weights64(wgt, nrow, nchan)
    iu, iv, inside = cells(uvw, freq, grid)
    d = dens[iu + grid.hx, iv].astype(np.float64) * grid.quantum
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == UNIFORM:
            res = np.where(d > 0, w / d, 0.0)
        else:
            res = w / (1.0 + d * f2)
    res = np.where(inside & (w != 0), res, 0.0)
    return res.astype(out_dtype)
