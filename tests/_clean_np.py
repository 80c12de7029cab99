"""
The numpy statement of Hogbom CLEAN as include/cip.h defines it
(`cip_hogbom_clean`): the reference the GPU tests compare against bit for bit.
"""

import numpy as np

NITER, THRESHOLD, EMPTY = 0, 1, 2


def hogbom_clean(res, psf, gain=0.1, threshold=0.0, niter=1000, mask=None, model=None, psf_centre=None):
    """-> (model, residual, info); the inputs are not modified."""
    res = np.array(res, dtype=np.float64)
    nx, ny = res.shape
    px, py = psf.shape
    cx, cy = (px // 2, py // 2) if psf_centre is None else psf_centre
    model = np.zeros_like(res) if model is None else np.array(model, dtype=np.float64)
    allowed = np.ones(res.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    gain = np.float64(gain)
    comp_index, comp_flux = [], []
    k = 0
    while True:
        score = np.where(allowed & ~np.isnan(res), np.abs(res), -1.0)
        flat = int(np.argmax(score))  # the first maximum: the lowest flat index
        i, j = divmod(flat, ny)
        if score[i, j] < 0:
            reason, peak, flat = EMPTY, 0.0, -1
            break
        peak = res[i, j]
        if abs(peak) <= threshold:
            reason = THRESHOLD
            break
        if k == niter:
            reason = NITER
            break
        f = gain * peak
        model[i, j] += f
        comp_index.append(flat)
        comp_flux.append(f)
        # image window [i0, i1) x [j0, j1) whose PSF index (i' - i + cx, j' - j + cy) is inside the PSF
        i0, i1 = max(0, i - cx), min(nx, i - cx + px)
        j0, j1 = max(0, j - cy), min(ny, j - cy + py)
        res[i0:i1, j0:j1] -= f * psf[i0 - i + cx:i1 - i + cx, j0 - j + cy:j1 - j + cy]
        k += 1
    info = {"niter_done": k, "stop_reason": reason, "peak": float(peak), "peak_index": flat,
            "comp_index": np.array(comp_index, dtype=np.int64), "comp_flux": np.array(comp_flux, dtype=np.float64)}
    return model, res, info
