"""
The numpy statement of include/cip_noise.h (no scipy): `select`, `noise` and
`auto_mask`. Tests compare the library with these for equality, not closeness.
"""
from collections import deque

import numpy as np

MAD_TO_SIGMA = 1.482602218505602


def samples(image, region=None):
    """The finite pixels inside `region` (None: all), flat."""
    x = np.asarray(image, dtype=np.float64).ravel()
    keep = np.isfinite(x)
    if region is not None:
        keep &= np.asarray(region).ravel() != 0
    return x[keep]


def select(image, rank, region=None):
    """(np.sort(samples)[rank], count); the value is None when rank >= count."""
    v = samples(image, region)
    return (np.sort(v)[rank] if 0 <= rank < v.size else None), int(v.size)


def noise(image, region=None):
    """count, the lower median, the same rank among |x - median| (one rounded
    subtraction each; an overflow to +inf sorts last) and MAD_TO_SIGMA * mad."""
    v = samples(image, region)
    if v.size == 0:
        return dict(count=0, median=np.nan, mad=np.nan, sigma=np.nan)
    rank = (v.size - 1) // 2
    median = np.sort(v)[rank]
    with np.errstate(over="ignore"):
        mad = np.sort(np.abs(v - median))[rank]
        sigma = np.float64(MAD_TO_SIGMA) * mad
    return dict(count=int(v.size), median=float(median), mad=float(mad), sigma=float(sigma))


def auto_mask(image, seed, grow=None, region=None, base=None, positive=False, connectivity=8):
    """(mask uint8, dict(n_seed, n_island, n_out)): "in" spreads from the seeds
    to neighbouring candidates until none is left."""
    x = np.asarray(image, dtype=np.float64)
    grow = seed if grow is None else grow
    a = x if positive else np.abs(x)
    with np.errstate(invalid="ignore"):
        lo = a >= grow  # NaN: False
        hi = lo & (a >= seed)
    if region is not None:
        allowed = np.asarray(region) != 0
        lo, hi = lo & allowed, hi & allowed
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    inside = hi.copy()
    nx, ny = x.shape
    queue = deque(zip(*np.nonzero(hi)))
    while queue:  # breadth first from every seed at once
        i, j = queue.popleft()
        for di, dj in steps:
            p, q = i + di, j + dj
            if 0 <= p < nx and 0 <= q < ny and lo[p, q] and not inside[p, q]:
                inside[p, q] = True
                queue.append((p, q))
    mask = inside.copy()
    if base is not None:
        mask |= np.asarray(base) != 0
    return mask.astype(np.uint8), dict(n_seed=int(hi.sum()), n_island=int(inside.sum()), n_out=int(mask.sum()))


def serpentine(n):
    """A one-pixel-wide path of ones that fills an (n, n) image of zeros:
    every other row whole, joined by one pixel at alternating ends."""
    img = np.zeros((n, n))
    img[0::2, :] = 1.0
    for k, i in enumerate(range(1, n, 2)):
        img[i, n - 1 if k % 2 == 0 else 0] = 1.0
    return img
