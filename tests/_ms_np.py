"""
The numpy statement of multiscale CLEAN as include/cip_ms.h defines it: the
scale taps, the separable convolution (`cip_ms_convolve`), the minor cycle
(`cip_ms_clean`) and the model image. The reference the GPU tests compare
against bit for bit. Elementwise numpy never fuses a product into a sum, so
every `*`, `+`, `-` and `/` below is one rounded fp64 operation, in the header's
order.
"""

import numpy as np

NITER, THRESHOLD, EMPTY = 0, 1, 2


def tri(s, q, nscales):
    """The plane of the packed cross-PSF stack that holds the pair (s, q), s <= q."""
    return s * nscales - s * (s - 1) // 2 + (q - s)


def scale_radius(width, tol=1e-8):
    """ceil(sqrt(log(1 / tol) / c)) with c = (4 log 2) / width^2; 0 for width 0."""
    if width == 0:
        return 0
    c = (4.0 * np.log(2.0)) / (np.float64(width) * np.float64(width))
    return int(np.ceil(np.sqrt(np.log(1.0 / tol) / c)))


def scale_taps(width, radius=None, tol=1e-8):
    """The 2 R + 1 taps of the scale of FWHM `width` pixels: unit sum, [1.0] for width 0."""
    if width == 0:
        return np.ones(1)
    radius = scale_radius(width, tol) if radius is None else radius
    c = (4.0 * np.log(2.0)) / (np.float64(width) * np.float64(width))
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    e = np.exp(-((d * d) * c))
    total = np.float64(0.0)
    for v in e:  # ascending d, one add at a time (np.sum adds pairwise)
        total = total + v
    return e / total


def _pass(img, taps, axis):
    """One 1-D pass along `axis`: +0.0, then + taps[d + R] * img[.. + d] for d = -R .. R
    ascending over the terms inside the image."""
    img = np.moveaxis(img, axis, -1)
    n = img.shape[-1]
    radius = taps.size // 2
    out = np.zeros_like(img)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(-radius, radius + 1):
            lo, hi = max(0, -d), min(n, n - d)  # outputs j with 0 <= j + d < n
            if lo < hi:
                out[..., lo:hi] = out[..., lo:hi] + taps[d + radius] * img[..., lo + d:hi + d]
    return np.moveaxis(out, -1, axis)


def convolve(img, taps):
    """`cip_ms_convolve`: the pass along axis 1, then the pass along axis 0."""
    img = np.asarray(img, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    return np.ascontiguousarray(_pass(_pass(img, taps, 1), taps, 0))


def smooth(img, width, tol=1e-8):
    """`multiscale.device_ms_convolve`: a copy for width 0, else `convolve` with the scale's taps."""
    return np.array(img, dtype=np.float64) if width == 0 else convolve(img, scale_taps(width, tol=tol))


def scale_residuals(res, widths):
    return np.stack([smooth(res, w) for w in widths])


def cross_psfs(psf, widths):
    """Packed (S (S + 1) / 2, px, py): scale s first, then scale q, for s <= q."""
    n = len(widths)
    return np.stack([smooth(smooth(psf, widths[s]), widths[q]) for s in range(n) for q in range(s, n)])


def scale_weights(cross, widths, scale_bias=0.6, centre=None):
    n = len(widths)
    cx, cy = (cross.shape[1] // 2, cross.shape[2] // 2) if centre is None else centre
    flux_scale = 1.0 / np.array([cross[tri(s, s, n), cx, cy] for s in range(n)], dtype=np.float64)
    wmax = float(widths[-1])
    bias = np.array([1.0 if wmax == 0.0 else 1.0 - scale_bias * float(w) / wmax for w in widths])
    return bias * flux_scale, flux_scale


def ms_model(models, widths):
    """sum_s scale_s (*) models[s], added in ascending s."""
    total = smooth(models[0], widths[0])
    for s in range(1, len(widths)):
        total = total + smooth(models[s], widths[s])
    return total


def ms_clean(res, psf, select_weight, flux_scale, gain=0.1, threshold=0.0, niter=1000, mask=None, model=None,
             psf_centre=None):
    """res (S, nx, ny), psf (S (S + 1) / 2, px, py), select_weight and flux_scale (S,)
    -> (model, residual, info); the inputs are not modified."""
    res = np.array(res, dtype=np.float64)
    psf = np.asarray(psf, dtype=np.float64)
    select_weight = np.asarray(select_weight, dtype=np.float64)
    flux_scale = np.asarray(flux_scale, dtype=np.float64)
    nscales, nx, ny = res.shape
    assert psf.shape[0] == nscales * (nscales + 1) // 2 and select_weight.shape == flux_scale.shape == (nscales,)
    px, py = psf.shape[1:]
    cx, cy = (px // 2, py // 2) if psf_centre is None else psf_centre
    model = np.zeros_like(res) if model is None else np.array(model, dtype=np.float64)
    allowed = np.ones((nx, ny), dtype=bool) if mask is None else np.asarray(mask) != 0
    gain = np.float64(gain)
    comp_index, comp_scale, comp_flux = [], [], []
    k = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            v = select_weight[:, None, None] * res
            score = np.where(allowed[None] & ~np.isnan(v), np.abs(v), -1.0)
            key = int(np.argmax(score))  # the first maximum: the lowest key s nx ny + flat
            sel, flat = divmod(key, nx * ny)
            i, j = divmod(flat, ny)
            if score[sel, i, j] < 0:
                reason, peak, flat, sel = EMPTY, 0.0, -1, -1
                break
            peak = v[sel, i, j]
            if abs(peak) <= threshold:
                reason = THRESHOLD
                break
            if k == niter:
                reason = NITER
                break
            f = gain * (flux_scale[sel] * res[sel, i, j])
            model[sel, i, j] += f
            comp_index.append(flat)
            comp_scale.append(sel)
            comp_flux.append(f)
            # image window [i0, i1) x [j0, j1) whose PSF index (i' - i + cx, j' - j + cy) is inside the PSF
            i0, i1 = max(0, i - cx), min(nx, i - cx + px)
            j0, j1 = max(0, j - cy), min(ny, j - cy + py)
            for s in range(nscales):
                plane = psf[tri(min(s, sel), max(s, sel), nscales)]
                res[s, i0:i1, j0:j1] -= f * plane[i0 - i + cx:i1 - i + cx, j0 - j + cy:j1 - j + cy]
            k += 1
    info = {"niter_done": k, "stop_reason": reason, "peak": float(peak), "peak_index": flat, "peak_scale": sel,
            "comp_index": np.array(comp_index, dtype=np.int64), "comp_scale": np.array(comp_scale, dtype=np.int64),
            "comp_flux": np.array(comp_flux, dtype=np.float64)}
    return model, res, info
