"""
The numpy statement of include/cip_dft.h (sky-model predict): every sample, in
fp64, in loops over row chunks and components. The reference of
test_dft_host.py, test_gpu_dft_predict.py and test_gpu_selfcal_skymodel.py.

    model[r, c] = sum_k S_k(c) G_k(r, c) exp(-2 pi i fx_c p_k(r)),  fx_c = freq_c / c0

As in the header, the phase fx p (cycles) is reduced to its fraction before the
sine and cosine (exact in fp64), and a component with a non-finite field, a
negative FWHM or (with the w term) 1 - l^2 - m^2 <= 0 contributes nothing.
"""
import numpy as np

C0 = 299792458.0
ENVELOPE = np.pi ** 2 / (4.0 * np.log(2.0))
MAX_TERMS = 3
FLAG_ADD, FLAG_SUBTRACT, FLAG_WTERM, FLAG_FAST = 1, 2, 4, 8


def coefficients(lm, flux, shape=None, w_term=True):
    """Per component: (l, m, nm1, sin pa, cos pa, ea, eb) and the flux with the left-out components zeroed."""
    lm = np.asarray(lm, dtype=np.float64).reshape(-1, 2)
    flux = np.array(flux, dtype=np.float64)
    flux = flux.reshape(len(lm), -1) if len(lm) else np.zeros((0, flux.shape[-1] if flux.ndim == 2 else 1))
    l, m = lm[:, 0].copy(), lm[:, 1].copy()  # noqa: E741
    ok = np.isfinite(l) & np.isfinite(m) & np.isfinite(flux).all(axis=1)
    nm1 = np.zeros(len(lm))
    with np.errstate(invalid="ignore"):
        if w_term:
            e = l * l + m * m
            n2 = 1.0 - e
            ok &= n2 > 0.0
            nm1 = -e / (np.sqrt(np.where(ok, n2, 1.0)) + 1.0)
        sp, cp, ea, eb = np.zeros(len(lm)), np.ones(len(lm)), np.zeros(len(lm)), np.zeros(len(lm))
        if shape is not None:
            shape = np.asarray(shape, dtype=np.float64).reshape(len(lm), 3)
            ok &= np.isfinite(shape).all(axis=1) & (shape[:, 0] >= 0.0) & (shape[:, 1] >= 0.0)
            ext = ok & ((shape[:, 0] != 0.0) | (shape[:, 1] != 0.0))
            pa = np.where(ext, shape[:, 2], 0.0)
            sp, cp = np.where(ext, np.sin(pa), 0.0), np.where(ext, np.cos(pa), 1.0)
            ea = np.where(ext, ENVELOPE * (shape[:, 0] * shape[:, 0]), 0.0)
            eb = np.where(ext, ENVELOPE * (shape[:, 1] * shape[:, 1]), 0.0)
    zero = lambda a: np.where(ok, a, 0.0)  # noqa: E731
    return dict(l=zero(l), m=zero(m), nm1=zero(nm1), sp=zero(sp), cp=np.where(ok, cp, 1.0), ea=zero(ea), eb=zero(eb),
                flux=np.where(ok[:, None], flux, 0.0), ok=ok)


def spectra(flux, freq, ref_freq):
    """S (ncomp, nchan): sum_t flux[k, t] x_c^t, x_c = (freq_c - ref_freq) / ref_freq."""
    flux = np.asarray(flux, dtype=np.float64)
    nterms = flux.shape[1]
    if not 1 <= nterms <= MAX_TERMS:
        raise ValueError("nterms")
    if nterms == 1:
        return np.repeat(flux[:, :1], len(freq), axis=1)
    x = (np.asarray(freq, dtype=np.float64) - ref_freq) / ref_freq
    return sum(flux[:, t:t + 1] * x[None, :] ** t for t in range(nterms))


def predict(uvw, freq, lm, flux, shape=None, ref_freq=0.0, w_term=True, row_chunk=4096):
    """
    The model column, complex128 (nrow, nchan), and the two figures of the
    fp64-class bound: phi, the largest |phase| in cycles, and sigma = max_c
    sum_k |S_k(c)|.
    """
    uvw = np.asarray(uvw, dtype=np.float64)
    freq = np.asarray(freq, dtype=np.float64)
    co = coefficients(lm, flux, shape, w_term)
    s = spectra(co["flux"], freq, ref_freq)
    fx = freq / C0
    out = np.zeros((len(uvw), len(freq)), dtype=np.complex128)
    phi = 0.0
    for a in range(0, len(uvw), row_chunk):
        u, v, w = (uvw[a:a + row_chunk, i] for i in range(3))
        acc = out[a:a + row_chunk]
        for k in range(len(s)):
            p = u * co["l"][k] + v * co["m"][k] - w * co["nm1"][k]
            ph = p[:, None] * fx[None, :]
            phi = max(phi, float(np.abs(ph).max(initial=0.0)))
            fr = ph - np.rint(ph)
            term = s[k][None, :] * np.exp(-2j * np.pi * fr)
            if shape is not None:
                pa = u * co["sp"][k] + v * co["cp"][k]
                pb = u * co["cp"][k] - v * co["sp"][k]
                q = co["ea"][k] * (pa * pa) + co["eb"][k] * (pb * pb)
                term = term * np.exp(-(fx * fx)[None, :] * q[:, None])
            acc += term
    sigma = float(np.abs(s).sum(axis=0).max(initial=0.0)) if len(s) else 0.0
    return out, phi, sigma


def apply(model, vis_io, wgt, mode):
    """The flags' rule: the column cip_dft_predict leaves in vis_io (same dtype), `mode` in set / add / subtract."""
    w = np.ones(model.shape) if wgt is None else np.asarray(wgt, dtype=np.float64)
    wm = w * model
    old = np.asarray(vis_io).astype(np.complex128)
    with np.errstate(invalid="ignore"):
        new = {"set": wm, "add": old + wm, "subtract": old - wm}[mode]
    out = new.astype(vis_io.dtype)
    zero = w == 0.0
    out[zero] = 0.0 if mode == "set" else np.asarray(vis_io)[zero]
    return out


def fp64_bound(phi, sigma):
    """|gpu - reference| per sample in the fp64 class: sigma (32 pi phi 2^-52 + 1e-13)."""
    return sigma * (32.0 * np.pi * phi * 2.0 ** -52 + 1e-13)
