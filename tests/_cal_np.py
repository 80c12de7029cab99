"""
The numpy statement of include/cip_cal.h (gain self-calibration): every
operation is one rounded fp64 numpy operation on real arrays, sums over the
antenna index run in Python loops in the header's order, so the device results
can be compared bit for bit. Not a test module.
"""
import math

import numpy as np

MAX_ANT = 1024


def scale_init(n_ant, n_int, amax, wmax, nsamp_max):
    """cip_cal_scale_init: a dict with the struct's fields."""
    if not (2 <= n_ant <= MAX_ANT) or n_int < 1 or nsamp_max < 1:
        raise ValueError("shape")
    if not (np.isfinite(amax) and amax > 0 and np.isfinite(wmax) and wmax > 0):
        raise ValueError("bounds")
    x = ((2.0 * float(wmax)) * float(amax)) * float(amax)
    b = 0
    while (1 << b) < nsamp_max:
        b += 1
    e = math.frexp(x)[1]  # x = m 2^e, 0.5 <= m < 1: the least e with x < 2^e
    shift = 61 - b - e
    return dict(n_ant=int(n_ant), n_int=int(n_int), amax=float(amax), wmax=float(wmax), shift=shift,
                quantum=math.ldexp(1.0, -shift))


def _parts(x):
    x = np.asarray(x)
    return x.real.astype(np.float64), x.imag.astype(np.float64)


def _classify(vis, model, wgt, ant1, ant2, interval, n_ant, n_int):
    """(row_ok (nrow), zero, bad, candidate (nrow, nchan) masks, the five fp64 planes)."""
    vr, vi = _parts(vis)
    mr, mi = _parts(model)
    w = np.asarray(wgt).astype(np.float64)
    p, q, s = (np.asarray(a).astype(np.int64) for a in (ant1, ant2, interval))
    row_ok = (p != q) & (p >= 0) & (p < n_ant) & (q >= 0) & (q < n_ant) & (s >= 0) & (s < n_int)
    rows = row_ok[:, None]
    zero = rows & (w == 0.0)
    finite = np.isfinite(w) & np.isfinite(vr) & np.isfinite(vi) & np.isfinite(mr) & np.isfinite(mi)
    bad = rows & ~zero & (~(w > 0.0) | ~finite)
    cand = rows & ~zero & ~bad
    return row_ok, zero, bad, cand, (vr, vi, mr, mi, w)


def correlate(vis, model, wgt, ant1, ant2, interval, scale, corr=None):
    """cip_cal_correlate: (corr int64 (n_int, n_ant, n_ant, 3), counts dict); `corr` is accumulated into a copy."""
    n_ant, n_int = scale["n_ant"], scale["n_int"]
    corr = np.zeros((n_int, n_ant, n_ant, 3), dtype=np.int64) if corr is None else corr.copy()
    row_ok, zero, bad, cand, (vr, vi, mr, mi, w) = _classify(vis, model, wgt, ant1, ant2, interval, n_ant, n_int)
    nchan = w.shape[1]
    with np.errstate(all="ignore"):
        big = np.maximum(np.maximum(np.abs(vr), np.abs(vi)), np.maximum(np.abs(mr), np.abs(mi)))
        outside = cand & ((w > scale["wmax"]) | (big > scale["amax"]))
        add = cand & ~outside
        z = lambda a: np.where(add, a, 0.0)  # noqa: E731 - skipped samples contribute exact zeros
        vr, vi, mr, mi, w = z(vr), z(vi), z(mr), z(mi), z(w)
        cr = vr * mr + vi * mi
        ci = vi * mr - vr * mi
        m2 = mr * mr + mi * mi
        terms = [np.rint(np.ldexp(w * t, scale["shift"])).astype(np.int64) for t in (cr, ci, m2)]
    p, q, s = (np.asarray(a).astype(np.int64) for a in (ant1, ant2, interval))
    fold = p > q
    lo, hi = np.minimum(p, q), np.maximum(p, q)
    sums = [t.sum(axis=1) for t in terms]
    sums[1] = np.where(fold, -sums[1], sums[1])
    ok = np.nonzero(row_ok)[0]
    for k in range(3):
        np.add.at(corr, (s[ok], lo[ok], hi[ok], k), sums[k][ok])
    counts = dict(n_added=int(add.sum()), n_zero=int(zero.sum()),
                  n_outside=int(outside.sum()) + int((~row_ok).sum()) * nchan, n_bad=int(bad.sum()))
    return corr, counts


def sample_max(vis, model, wgt, ant1, ant2, interval, n_ant, n_int):
    """Step 1 of cip_gaincal: (amax, wmax) of the samples that will be added, 1.0 when there are none."""
    _, _, _, cand, (vr, vi, mr, mi, w) = _classify(vis, model, wgt, ant1, ant2, interval, n_ant, n_int)
    if not cand.any():
        return 1.0, 1.0
    big = np.maximum(np.maximum(np.abs(vr), np.abs(vi)), np.maximum(np.abs(mr), np.abs(mi)))
    amax, wmax = float(big[cand].max()), float(w[cand].max())
    return (amax if amax > 0.0 else 1.0), (wmax if wmax > 0.0 else 1.0)


def solve(corr, scale, niter, tol, refant=-1, phase_only=False, gains=None):
    """cip_cal_solve: (gains complex128 (n_int, n_ant), ant_ok uint8, iters int64 (n_int), info dict)."""
    n, n_int = scale["n_ant"], scale["n_int"]
    if niter < 0 or not (np.isfinite(tol) and tol >= 0) or refant >= n:
        raise ValueError("arguments")
    gains = np.ones((n_int, n), dtype=np.complex128) if gains is None else np.array(gains, dtype=np.complex128)
    d = corr.astype(np.float64) * scale["quantum"]
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    ant_ok = np.ones((n_int, n), dtype=np.uint8)
    iters = np.zeros(n_int, dtype=np.int64)
    info = dict(n_converged=0, n_dead=0, max_iter_done=0, ref_missing=0, max_change=0.0)
    tol2 = float(tol) * float(tol)
    with np.errstate(all="ignore"):
        for s in range(n_int):
            # A_pq = D0 + i D1 (p < q), its conjugate (p > q), 0 on the diagonal; B_pq = D2 in both orders
            ar = np.where(upper, d[s, :, :, 0], np.where(upper.T, d[s, :, :, 0].T, 0.0))
            ai = np.where(upper, d[s, :, :, 1], np.where(upper.T, -d[s, :, :, 1].T, 0.0))
            bb = np.where(upper, d[s, :, :, 2], np.where(upper.T, d[s, :, :, 2].T, 0.0))
            gr, gi = gains[s].real.copy(), gains[s].imag.copy()
            gr_in, gi_in = gr.copy(), gi.copy()
            dead = np.zeros(n, dtype=bool)

            def denominator(gr, gi):
                m2 = gr * gr + gi * gi
                den = np.zeros(n)
                for q in range(n):
                    den = den + bb[:, q] * m2[q]
                return den

            if niter == 0:
                dead = denominator(gr, gi) == 0.0
            d2 = n2 = 0.0
            converged = False
            for k in range(1, niter + 1):
                nr, ni = np.zeros(n), np.zeros(n)
                for q in range(n):
                    nr = nr + (ar[:, q] * gr[q] - ai[:, q] * gi[q])
                    ni = ni + (ar[:, q] * gi[q] + ai[:, q] * gr[q])
                den = denominator(gr, gi)
                if k == 1:
                    dead = den == 0.0
                xr, xi = nr / den, ni / den
                if phase_only:
                    av = np.sqrt(xr * xr + xi * xi)
                    xr, xi = xr / av, xi / av
                if k % 2 == 0:
                    xr, xi = 0.5 * (xr + gr), 0.5 * (xi + gi)
                xr, xi = np.where(dead, gr, xr), np.where(dead, gi, xi)
                d2 = n2 = 0.0
                for p in range(n):
                    dr, di = xr[p] - gr[p], xi[p] - gi[p]
                    d2 = d2 + (dr * dr + di * di)
                    n2 = n2 + (xr[p] * xr[p] + xi[p] * xi[p])
                gr, gi = xr, xi
                iters[s] = k
                if d2 <= tol2 * n2:
                    converged = True
                    break
            ant_ok[s] = ~dead
            info["n_dead"] += int(dead.sum())
            if niter == 0:
                continue
            info["n_converged"] += int(converged)
            info["max_iter_done"] = max(info["max_iter_done"], int(iters[s]))
            if n2 > 0.0:
                change = math.sqrt(d2 / n2)
                if change > info["max_change"]:
                    info["max_change"] = change
            if refant >= 0:
                if dead[refant]:
                    info["ref_missing"] += 1
                else:
                    av = np.sqrt(gr[refant] * gr[refant] + gi[refant] * gi[refant])
                    ur, ui = gr[refant] / av, -(gi[refant] / av)
                    gr, gi = gr * ur - gi * ui, gr * ui + gi * ur
            gains[s].real = np.where(dead, gr_in, gr)
            gains[s].imag = np.where(dead, gi_in, gi)
    return gains, ant_ok, iters, info


def apply(vis, wgt, ant1, ant2, interval, gains, ant_ok, mode="correct"):
    """cip_cal_apply: (vis_out, wgt_out) in the input dtypes (wgt_out None without wgt)."""
    n_int, n_ant = gains.shape
    p, q, s = (np.asarray(a).astype(np.int64) for a in (ant1, ant2, interval))
    ok = (p >= 0) & (p < n_ant) & (q >= 0) & (q < n_ant) & (s >= 0) & (s < n_int)
    pc, qc, sc = np.where(ok, p, 0), np.where(ok, q, 0), np.where(ok, s, 0)
    ok &= (ant_ok[sc, pc] != 0) & (ant_ok[sc, qc] != 0)
    gp, gq = gains[sc, pc], gains[sc, qc]
    with np.errstate(all="ignore"):
        hr = (gp.real * gq.real + gp.imag * gq.imag)[:, None]
        hi = (gp.imag * gq.real - gp.real * gq.imag)[:, None]
        n2 = hr * hr + hi * hi
        vr, vi = _parts(vis)
        if mode == "correct":
            xr, xi = (vr * hr + vi * hi) / n2, (vi * hr - vr * hi) / n2
        else:
            xr, xi = hr * vr - hi * vi, hr * vi + hi * vr
        out = np.empty(vr.shape, dtype=np.asarray(vis).dtype)
        out.real = np.where(ok[:, None], xr, vr)
        out.imag = np.where(ok[:, None], xi, vi)
        wgt_out = None
        if wgt is not None:
            w = np.asarray(wgt).astype(np.float64)
            wo = w * n2 if mode == "correct" else w
            wgt_out = np.where(ok[:, None], wo, 0.0).astype(np.asarray(wgt).dtype)
    return out, wgt_out


def gaincal(vis, model, wgt, ant1, ant2, interval, n_ant, n_int, niter=50, tol=1e-8, refant=0, phase_only=False,
            gains=None):
    """cip_gaincal: the written-out sequence -> (gains, ant_ok, iters, info, scale, counts)."""
    amax, wmax = sample_max(vis, model, wgt, ant1, ant2, interval, n_ant, n_int)
    scale = scale_init(n_ant, n_int, amax, wmax, max(np.asarray(vis).size, 1))
    corr, counts = correlate(vis, model, wgt, ant1, ant2, interval, scale)
    return (*solve(corr, scale, niter, tol, refant, phase_only, gains), scale, counts)


def rotate_to(gains, refant=0):
    """`gains` (n_int, n_ant) with the phase of antenna `refant` removed per interval (for comparisons)."""
    ref = gains[:, refant]
    return gains * (np.conj(ref) / np.abs(ref))[:, None]
