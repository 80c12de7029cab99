"""
The numpy statement of the joint multi-term minor cycle as include/cip_mfs.h
defines it (`cip_mfs_clean`): the reference the GPU tests compare against bit
for bit. Elementwise numpy never fuses a product into a sum, so every `*`, `+`
and `-` below is one rounded fp64 operation, in the header's order.
"""

import numpy as np

NITER, THRESHOLD, EMPTY = 0, 1, 2


def _row(hinv, q, r):
    """hinv[q][0] r_0, then + hinv[q][t] r_t for t = 1 .. T - 1 in order."""
    s = hinv[q, 0] * r[0]
    for t in range(1, r.shape[0]):
        s = s + hinv[q, t] * r[t]
    return s


def mfs_clean(res, psf, hinv, gain=0.1, threshold=0.0, niter=1000, mask=None, model=None, psf_centre=None):
    """res (T, nx, ny), psf (2T - 1, px, py), hinv (T, T) -> (model, residual, info);
    the inputs are not modified."""
    res = np.array(res, dtype=np.float64)
    psf = np.asarray(psf, dtype=np.float64)
    hinv = np.asarray(hinv, dtype=np.float64)
    nterms, nx, ny = res.shape
    assert psf.shape[0] == 2 * nterms - 1 and hinv.shape == (nterms, nterms)
    px, py = psf.shape[1:]
    cx, cy = (px // 2, py // 2) if psf_centre is None else psf_centre
    model = np.zeros_like(res) if model is None else np.array(model, dtype=np.float64)
    allowed = np.ones((nx, ny), dtype=bool) if mask is None else np.asarray(mask) != 0
    gain = np.float64(gain)
    comp_index, comp_flux = [], []
    k = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            s = _row(hinv, 0, res)
            score = np.where(allowed & ~np.isnan(s), np.abs(s), -1.0)
            flat = int(np.argmax(score))  # the first maximum: the lowest flat index
            i, j = divmod(flat, ny)
            if score[i, j] < 0:
                reason, peak, flat = EMPTY, 0.0, -1
                break
            peak = s[i, j]
            if abs(peak) <= threshold:
                reason = THRESHOLD
                break
            if k == niter:
                reason = NITER
                break
            f = np.array([gain * _row(hinv, q, res[:, i, j]) for q in range(nterms)], dtype=np.float64)
            model[:, i, j] += f
            comp_index.append(flat)
            comp_flux.append(f)
            # image window [i0, i1) x [j0, j1) whose PSF index (i' - i + cx, j' - j + cy) is inside the PSF
            i0, i1 = max(0, i - cx), min(nx, i - cx + px)
            j0, j1 = max(0, j - cy), min(ny, j - cy + py)
            for t in range(nterms):
                for q in range(nterms):
                    res[t, i0:i1, j0:j1] -= f[q] * psf[t + q, i0 - i + cx:i1 - i + cx, j0 - j + cy:j1 - j + cy]
            k += 1
    info = {"niter_done": k, "stop_reason": reason, "peak": float(peak), "peak_index": flat,
            "comp_index": np.array(comp_index, dtype=np.int64),
            "comp_flux": np.array(comp_flux, dtype=np.float64).reshape(k, nterms)}
    return model, res, info
