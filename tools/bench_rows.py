#!/usr/bin/env python3
"""
Secondary measurements of the SURVEY.md 8(f) rows built beside the hot path
(bench.py keeps the contract's one JSON line for the headline metric):

  --mode stream     invert_measurement_set_streamed: raw (rows, chans, 4)
                    columns in HOST memory, staged through pinned buffers to
                    HBM on a copy stream while the previous chunk grids
                    (PCIe-inclusive; row 2, config C5's host->HBM streaming)
  --mode continuum  continuum_invert: Stokes I, Q, U, V dirty images + PSF on
                    a mosaic of facets (row 4, config C5's products) from
                    device-resident raw columns
  --mode degrid     device_dirty2ms (predict, the invert's transpose) on
                    resident synthetic data: 2-D support 8 fp64, or --refcall
                    (epsilon 1e-4, w-stacking); also the same call through an
                    invert's tile plan (reuse_plan) and the invert's own time
                    on the same inputs
  --mode clean      device_hogbom_clean (the minor cycle) on a seeded image of
                    point sources convolved with a PSF cut from a real
                    device_ms2dirty(psf=True) call: microseconds per iteration
                    and the GB/s that implies at 24 B per window pixel, beside
                    the obvious torch loop on the same device (argmax(abs) ->
                    .item() -> sliced sub_) in the same run
  --mode mfs_clean  device_mfs_clean (the joint minor cycle of multi-term MFS,
                    --nterms Taylor terms) on seeded point sources with linear
                    spectra convolved with the PSF stack of a real
                    device_mfs_invert call, once with the full PSF and once
                    with a --patch^2 cut: microseconds per iteration and the
                    GB/s that implies at 8 (4T - 1) B per window pixel, beside
                    device_hogbom_clean on term 0 at the same shapes and a
                    torch loop that restates the operator, all in the same
                    run; also written to profiles/mfs_clean_c3.json
  --mode ms_clean   device_ms_clean (the multiscale minor cycle, scales --widths)
                    on the scene of --mode clean smoothed with every scale,
                    once with a --patch^2 cut of the PSF and once with the full
                    PSF: microseconds per iteration and the GB/s that implies
                    at 24 S B per window pixel, beside device_hogbom_clean at
                    the same shapes in the same run; and device_ms_convolve on
                    the full image at radius 32 and 128: ms and GB/s at 32 B
                    per pixel; also written to profiles/ms_clean_c3.json
  --mode weights    uniform imaging weights (weighting.py) on bench.py's C3
                    inputs and geometry: density / statistics / apply and the
                    one-shot call, best of --repeat; the synchronous
                    device_ms2dirty step of the same inputs in the same run;
                    a torch restatement on the same device (cell index,
                    bincount with weights, gather, divide) and whether its
                    weights agree; the mean run of equal cells a lane merges
                    into one atomic add
  --mode restore    device_restore on an 8192^2 image with the beam fitted to a
                    PSF from device_ms2dirty(psf=True) on bench.py's C3 inputs:
                    a sparse model (10 000 seeded non-zeros) and a dense 512^2
                    patch, best of --repeat around a synchronised call, beside
                    torch conv2d in fp64 with the same taps plus the add and a
                    torch fft2 convolution on the same device in the same run;
                    also written to profiles/restore_c3.json
  --mode gaincal    gain calibration (calibrate.py) on bench.py's C3 inputs as
                    the model column, the data being that column with seeded
                    gains multiplied in, 64 antennas, intervals of 16 dumps:
                    correlate / solve (50 iterations) / apply and the one-shot
                    call, best of --repeat; a torch restatement of the
                    correlate (fp64 terms, index_add_) and a read-only torch
                    stream of the same 20 B per sample in the same run; the
                    same for the samples laid out as rows of 64 channels; also
                    written to profiles/gaincal_c3.json
  --mode dft        device_dft_predict (skymodel.py, the sky-model predict) on
                    bench.py's C3 rows (390,625 x 256): 64 and 1024 seeded
                    components, points and Gaussians, the fp64 and the fast
                    class, complex64 output with weights, best of --repeat
                    around a synchronised call: ms and (visibility, component)
                    pairs per second, beside a torch restatement of the same
                    sum in fp64 on the same device in the same run (64
                    components: best of --repeat; 1024: one run); also written
                    to profiles/dft_predict_c3.json
  --mode noise      device_image_noise and device_auto_mask (noise.py) on the
                    scene of --mode clean at --noise-npix^2 (8192) with seeded
                    Gaussian pixel noise: ms per call, interleaved in the same
                    run with what torch offers for the same numbers
                    (kthvalue of the flattened image, then of |x - median|),
                    both lists of times and their spread; the full reads of
                    the image the two selects make (replayed in numpy from the
                    digit widths and the compaction capacity), the GB/s that
                    implies beside a device copy of the same image; the mask
                    at (5 sigma, 3 sigma) and its rounds; and one major
                    cycle's predict + re-invert on bench.py's C3 inputs, with
                    the noise and the mask at C3's image size beside it; also
                    written to profiles/noise_c3.json
  --mode mosaic     the facet mosaic (mosaic.py, cip_mosaic_add) at C5's size:
                    --facets-xy (8 4) facets of --mosaic-facet^2 (4096) pixels
                    with --mosaic-planes (4) planes at C5's pixel size onto the
                    largest plane for which `facet_layout` places that grid,
                    half-width --mosaic-half (6): ms per `add` (best and
                    median over the facets of the best of --repeat mosaics),
                    ms for the whole mosaic (the adds and `finish`), with the
                    tile windows staged in LDS and with direct loads
                    (CIP_MOSAIC_LDS), the two alternating in the same run;
                    the traffic floor (each facet read once, the footprint's
                    num and wsum read and written once) and the GB/s and the
                    fraction of a device copy's rate that implies; the fp64
                    fused multiply-adds of the tap sums per second; the same
                    adds with one plane, which splits an add into the part per
                    plane and the geometry and taps; also written to
                    profiles/mosaic_c5.json

Each prints one JSON line (synthetic data: real uvw tracks, random values).
"""

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "ska-sdp-continuum-imaging-pipeline_amd"))

import numpy as np  # noqa: E402


def degrid(args):
    """ms per device_dirty2ms call on resident inputs, its profile phases, the
    call through an invert's plan, and that invert's time."""
    import torch

    from ska_sdp_cip_amd import _lib, gridder, synthetic as syn

    dev = torch.device("cuda", 0)
    uvw_h = syn.uvw_tracks(args.rows, 64, array_radius_m=4000.0)
    freq_h = syn.channel_frequencies(args.nchan)
    px = syn.pixel_size_for_grid(uvw_h, freq_h, args.npix, support=8)
    uvw, freq = torch.from_numpy(uvw_h).to(dev), torch.from_numpy(freq_h).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(20241008)
    shape = (args.rows, args.nchan)
    vis = torch.randn(shape, dtype=torch.complex64, device=dev, generator=g)
    wgt = torch.rand(shape, dtype=torch.float32, device=dev, generator=g) + 0.5
    image = torch.randn((args.npix, args.npix), dtype=torch.float64, device=dev, generator=g)
    out = torch.empty(shape, dtype=torch.complex64, device=dev)
    call = dict(epsilon=1e-4, do_wstacking=True) if args.refcall else dict(support=8, do_wstacking=False)
    nvis = args.rows * args.nchan

    def timed(fn):
        fn()  # warm-up: workspace, FFT plan, correction tables
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.repeat):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.repeat

    predict = lambda **kw: gridder.device_dirty2ms(uvw, freq, image, wgt, px, px, out=out, **call, **kw)  # noqa: E731
    invert = lambda: gridder.device_ms2dirty(uvw, freq, vis, wgt, args.npix, args.npix, px, px, **call)  # noqa: E731
    dt = timed(predict)
    _lib.profile_enable(True)
    _, params = predict()
    prof = _lib.profile_last()
    _lib.profile_enable(False)
    dt_invert = timed(invert)
    invert()  # the plan the reusing predict runs through
    dt_reuse = timed(lambda: predict(reuse_plan=True))
    mode = "epsilon 1e-4, w-stacking" if args.refcall else "2-D, support 8"
    return {"data": "synthetic (real uvw tracks, random fp64 image, float32 weights, complex64 output)",
            "rows": args.rows, "channels": args.nchan, "npix": args.npix, "visibilities": nvis,
            "metric": f"Gvis/s predicted (device_dirty2ms, {mode}, fp64)", "value": round(nvis / dt / 1e9, 3),
            "unit": "Gvis/s", "ms_per_call": round(dt * 1e3, 3), "support": params.support,
            "nplanes": params.nplanes, "grid": [params.nu, params.nv],
            "phases_ms": {k: round(v, 3) for k, v in prof.items() if k.endswith("_ms")},
            "degrid_launches": prof["scatter_launches"], "chunks": prof["chunks"],
            "reuse_plan_ms_per_call": round(dt_reuse * 1e3, 3),
            "reuse_plan_gvis_per_s": round(nvis / dt_reuse / 1e9, 3),
            "invert_ms_per_call": round(dt_invert * 1e3, 3), "invert_gvis_per_s": round(nvis / dt_invert / 1e9, 3)}


def clean(args):
    """us per CLEAN iteration of device_hogbom_clean and of the torch loop."""
    import torch

    from ska_sdp_cip_amd import _lib, deconvolve, gridder, synthetic as syn

    dev = torch.device("cuda", 0)
    npix, pn = args.npix, args.psf_npix
    full = max(npix, pn)
    uvw_h = syn.uvw_tracks(args.rows, 64, array_radius_m=4000.0)
    freq_h = syn.channel_frequencies(args.nchan)
    px = syn.pixel_size_for_grid(uvw_h, freq_h, full, support=8)
    uvw, freq = torch.from_numpy(uvw_h).to(dev), torch.from_numpy(freq_h).to(dev)
    psf_full, _ = gridder.device_ms2dirty(uvw, freq, None, None, full, full, px, px, support=8, psf=True,
                                          normalise=True)
    o = full // 2 - pn // 2  # the cut keeps the peak at (pn // 2, pn // 2)
    psf = psf_full[o:o + pn, o:o + pn].contiguous()
    del psf_full
    _lib.lib().cip_release_workspace()  # the invert's grid is not needed any more
    c = pn // 2

    def window(i, j):
        i0, i1, j0, j1 = max(0, i - c), min(npix, i - c + pn), max(0, j - c), min(npix, j - c + pn)
        return i0, i1, j0, j1

    rng = np.random.default_rng(20241019)
    image = torch.zeros((npix, npix), dtype=torch.float64, device=dev)
    for i, j, flux in zip(rng.integers(0, npix, args.sources), rng.integers(0, npix, args.sources),
                          rng.lognormal(0.0, 1.0, args.sources)):
        i0, i1, j0, j1 = window(int(i), int(j))
        image[i0:i1, j0:j1] += float(flux) * psf[i0 - i + c:i1 - i + c, j0 - j + c:j1 - j + c]
    gain, niter = args.gain, args.niter

    def hip_run():
        res = image.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model, res, info = deconvolve.device_hogbom_clean(res, psf, gain=gain, niter=niter, inplace=True,
                                                          return_components=True, batch=args.batch)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, model, res, info

    def torch_run():
        res = image.clone()
        model = torch.zeros_like(res)
        flat_res, flat_model = res.view(-1), model.view(-1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(niter):
            flat = int(torch.argmax(torch.abs(res)).item())
            f = gain * flat_res[flat]
            flat_model[flat] += f
            i, j = divmod(flat, npix)
            i0, i1, j0, j1 = window(i, j)
            res[i0:i1, j0:j1].sub_(f * psf[i0 - i + c:i1 - i + c, j0 - j + c:j1 - j + c])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, model, res

    hip_run()  # warm-up: workspace, kernels
    dt, model, res, info = min((hip_run() for _ in range(args.repeat)), key=lambda r: r[0])
    n = info["niter_done"]
    pixels = 0
    for flat in info["comp_index"].cpu().tolist():
        i0, i1, j0, j1 = window(*divmod(flat, npix))
        pixels += (i1 - i0) * (j1 - j0)
    dt_torch, model_t, res_t = torch_run()
    us, us_torch = dt / n * 1e6, dt_torch / niter * 1e6
    return {"data": "synthetic (lognormal point sources convolved with a PSF cut from device_ms2dirty(psf=True))",
            "npix": npix, "psf_npix": pn, "sources": args.sources, "niter": n, "gain": gain,
            "stop": info["stop"], "metric": "us per CLEAN iteration (device_hogbom_clean, fp64)",
            "value": round(us, 2), "unit": "us/iteration", "window_pixels_mean": round(pixels / n),
            "GBs_at_24B_per_window_pixel": round(24.0 * pixels / dt / 1e9, 1),
            "batch": args.batch or _lib.CIP_CLEAN_DEFAULT_BATCH,
            "torch_loop_us_per_iteration": round(us_torch, 2), "speedup_over_torch_loop": round(us_torch / us, 2),
            "bit_identical_to_torch_loop": bool(torch.equal(res, res_t) and torch.equal(model, model_t))}


def mfs_clean(args):
    """us per iteration of device_mfs_clean, of device_hogbom_clean at the same shapes and of a torch loop."""
    import torch

    from ska_sdp_cip_amd import _lib, deconvolve, mfs, synthetic as syn

    dev = torch.device("cuda", 0)
    npix, nterms, gain, niter = args.npix, args.nterms, args.gain, args.niter
    uvw_h = syn.uvw_tracks(args.rows, 64, array_radius_m=4000.0)
    freq_h = syn.channel_frequencies(args.nchan)
    px = syn.pixel_size_for_grid(uvw_h, freq_h, npix, support=8)
    uvw, freq = torch.from_numpy(uvw_h).to(dev), torch.from_numpy(freq_h).to(dev)
    ones = torch.ones((args.rows, args.nchan), dtype=torch.complex64, device=dev)
    _, psf_full = mfs.device_mfs_invert(uvw, freq, ones, None, npix, px, nterms=nterms, support=8)
    del ones
    _lib.lib().cip_release_workspace()  # the invert's grid is not needed any more
    hessian, hinv = mfs.mfs_hessian(psf_full)
    hinv_d = torch.from_numpy(hinv).to(dev)
    rng = np.random.default_rng(20241019)
    where = (rng.integers(0, npix, args.sources), rng.integers(0, npix, args.sources))
    fluxes = rng.lognormal(0.0, 1.0, args.sources)
    slopes = rng.normal(-0.7, 0.3, args.sources) * fluxes

    def case(pn):
        o = npix // 2 - pn // 2  # the cut keeps the peak at (pn // 2, pn // 2)
        psf = psf_full if pn == npix else psf_full[:, o:o + pn, o:o + pn].contiguous()
        c = pn // 2

        def window(i, j):
            return max(0, i - c), min(npix, i - c + pn), max(0, j - c), min(npix, j - c + pn)

        image = torch.zeros((nterms, npix, npix), dtype=torch.float64, device=dev)
        for i, j, i0, i1 in zip(*where, fluxes, slopes):
            a0, a1, b0, b1 = window(int(i), int(j))
            cut = (slice(a0 - i + c, a1 - i + c), slice(b0 - j + c, b1 - j + c))
            for t in range(nterms):
                image[t, a0:a1, b0:b1] += float(i0) * psf[t][cut]
                if nterms > 1:
                    image[t, a0:a1, b0:b1] += float(i1) * psf[t + 1][cut]

        def hip_run(n):
            res = image.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model, res, info = mfs.device_mfs_clean(res, psf, hinv, gain=gain, niter=n, inplace=True,
                                                    return_components=True, batch=args.batch)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, model, res, info

        def hogbom_run():
            res = image[0].clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, info = deconvolve.device_hogbom_clean(res, psf[0], gain=gain, niter=niter, inplace=True,
                                                        batch=args.batch)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, info

        def torch_run(n):
            res = image.clone()
            model = torch.zeros_like(res)
            flat_res, flat_model = res.view(nterms, -1), model.view(nterms, -1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                s = hinv_d[0, 0] * res[0]
                for t in range(1, nterms):
                    s = s + hinv_d[0, t] * res[t]
                flat = int(torch.argmax(torch.abs(s)).item())
                r = flat_res[:, flat].clone()
                f = []
                for q in range(nterms):
                    cq = hinv_d[q, 0] * r[0]
                    for t in range(1, nterms):
                        cq = cq + hinv_d[q, t] * r[t]
                    f.append(gain * cq)
                    flat_model[q, flat] += f[q]
                a0, a1, b0, b1 = window(*divmod(flat, npix))
                i, j = divmod(flat, npix)
                cut = (slice(a0 - i + c, a1 - i + c), slice(b0 - j + c, b1 - j + c))
                for t in range(nterms):
                    for q in range(nterms):
                        res[t, a0:a1, b0:b1].sub_(f[q] * psf[t + q][cut])
            torch.cuda.synchronize()
            return time.perf_counter() - t0, model, res

        hip_run(min(niter, 8))  # warm-up: workspace, kernels
        dt, _, _, info = min((hip_run(niter) for _ in range(args.repeat)), key=lambda r: r[0])
        n = info["niter_done"]
        pixels = 0
        for flat in info["comp_index"].cpu().tolist():
            a0, a1, b0, b1 = window(*divmod(flat, npix))
            pixels += (a1 - a0) * (b1 - b0)
        hogbom_run()
        dt_h, info_h = min((hogbom_run() for _ in range(args.repeat)), key=lambda r: r[0])
        nt = min(niter, args.torch_niter)
        _, model, res, _ = hip_run(nt)
        torch_run(2)
        dt_t, model_t, res_t = torch_run(nt)
        us, us_h, us_t = dt / n * 1e6, dt_h / info_h["niter_done"] * 1e6, dt_t / nt * 1e6
        per_pixel = 8 * (4 * nterms - 1)
        return {"psf_npix": pn, "niter": n, "stop": info["stop"], "us_per_iteration": round(us, 2),
                "window_pixels_mean": round(pixels / n), "bytes_per_window_pixel": per_pixel,
                "GBs_at_model_bytes": round(per_pixel * pixels / dt / 1e9, 1),
                "hogbom_us_per_iteration": round(us_h, 2), "hogbom_niter": info_h["niter_done"],
                "ratio_to_hogbom": round(us / us_h, 2), "byte_model_ratio": round((4 * nterms - 1) / 3, 2),
                "torch_loop_us_per_iteration": round(us_t, 2), "torch_loop_niter": nt,
                "speedup_over_torch_loop": round(us_t / us, 2),
                "bit_identical_to_torch_loop": bool(torch.equal(res, res_t) and torch.equal(model, model_t))}

    result = {"data": "synthetic (lognormal point sources with linear spectra convolved with the PSF stack of "
                      "device_mfs_invert on real uvw tracks)",
              "npix": npix, "nterms": nterms, "sources": args.sources, "gain": gain, "rows": args.rows,
              "channels": args.nchan, "hessian": hessian.tolist(), "batch": args.batch or _lib.CIP_CLEAN_DEFAULT_BATCH,
              "repeat": args.repeat, "metric": "us per iteration (device_mfs_clean, full PSF, fp64)",
              "unit": "us/iteration"}
    result["full_psf"] = case(npix)
    result["patch"] = case(min(args.patch, npix))
    result["value"] = result["full_psf"]["us_per_iteration"]
    if npix == 8192 and nterms == 2:  # the row DESIGN.md 15 quotes
        (ROOT / "profiles" / "mfs_clean_c3.json").write_text(json.dumps(result, indent=1) + "\n")
    return result


def ms_clean(args):
    """us per iteration of device_ms_clean and of device_hogbom_clean at the same shapes; GB/s of device_ms_convolve."""
    import torch

    from ska_sdp_cip_amd import _lib, deconvolve, gridder, multiscale, synthetic as syn

    dev = torch.device("cuda", 0)
    npix, gain, widths = args.npix, args.gain, [float(w) for w in args.widths]
    nscales = len(widths)
    uvw_h = syn.uvw_tracks(args.rows, 64, array_radius_m=4000.0)
    freq_h = syn.channel_frequencies(args.nchan)
    px = syn.pixel_size_for_grid(uvw_h, freq_h, npix, support=8)
    uvw, freq = torch.from_numpy(uvw_h).to(dev), torch.from_numpy(freq_h).to(dev)
    psf_full, _ = gridder.device_ms2dirty(uvw, freq, None, None, npix, npix, px, px, support=8, psf=True,
                                          normalise=True)
    _lib.lib().cip_release_workspace()  # the invert's grid is not needed any more
    rng = np.random.default_rng(20241019)
    where = (rng.integers(0, npix, args.sources), rng.integers(0, npix, args.sources))
    fluxes = rng.lognormal(0.0, 1.0, args.sources)

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def case(pn, niter):
        o = npix // 2 - pn // 2  # the cut keeps the peak at (pn // 2, pn // 2)
        psf = psf_full if pn == npix else psf_full[o:o + pn, o:o + pn].contiguous()
        c = pn // 2

        def window(i, j):
            return max(0, i - c), min(npix, i - c + pn), max(0, j - c), min(npix, j - c + pn)

        image = torch.zeros((npix, npix), dtype=torch.float64, device=dev)
        for i, j, flux in zip(*where, fluxes):
            a0, a1, b0, b1 = window(int(i), int(j))
            image[a0:a1, b0:b1] += float(flux) * psf[a0 - i + c:a1 - i + c, b0 - j + c:b1 - j + c]
        cross = multiscale.device_cross_psfs(psf, widths)
        select_weight, flux_scale = multiscale.scale_weights(cross, widths)
        scaled = multiscale.device_scale_residuals(image, widths)

        def ms_run(n):
            res = scaled.clone()
            dt, (_, _, info) = sync_time(lambda: multiscale.device_ms_clean(
                res, cross, select_weight, flux_scale, gain=gain, niter=n, inplace=True, return_components=True,
                batch=args.batch))
            return dt, info

        def hogbom_run(n):
            res = image.clone()
            dt, (_, _, info) = sync_time(lambda: deconvolve.device_hogbom_clean(res, psf, gain=gain, niter=n,
                                                                                inplace=True, batch=args.batch))
            return dt, info

        ms_run(min(niter, 8))  # warm-up: workspace, kernels
        dt, info = min((ms_run(niter) for _ in range(args.repeat)), key=lambda r: r[0])
        n = info["niter_done"]
        pixels = 0
        for flat in info["comp_index"].cpu().tolist():
            a0, a1, b0, b1 = window(*divmod(flat, npix))
            pixels += (a1 - a0) * (b1 - b0)
        hogbom_run(min(niter, 8))
        dt_h, info_h = min((hogbom_run(niter) for _ in range(args.repeat)), key=lambda r: r[0])
        us, us_h = dt / n * 1e6, dt_h / info_h["niter_done"] * 1e6
        return {"psf_npix": pn, "niter": n, "stop": info["stop"], "us_per_iteration": round(us, 2),
                "components_per_scale": torch.bincount(info["comp_scale"], minlength=nscales).cpu().tolist(),
                "window_pixels_mean": round(pixels / n), "bytes_per_window_pixel": 24 * nscales,
                "GBs_at_model_bytes": round(24.0 * nscales * pixels / dt / 1e9, 1),
                "hogbom_us_per_iteration": round(us_h, 2), "hogbom_niter": info_h["niter_done"],
                "ratio_to_hogbom": round(us / us_h, 2), "byte_model_ratio": float(nscales),
                "select_weight": select_weight.tolist(), "flux_scale": flux_scale.tolist()}

    def convolve(radius, width):
        taps = multiscale.scale_taps(width, radius)
        out = torch.empty_like(psf_full)
        run = lambda: multiscale.device_ms_convolve(psf_full, None, taps=taps, out=out)  # noqa: E731
        run()
        dt = min(sync_time(run)[0] for _ in range(max(args.repeat, 3)))
        # the input read, the workspace image written and read, the output written
        return {"radius": radius, "width": width, "ms": round(dt * 1e3, 3),
                "GBs_at_32B_per_pixel": round(32.0 * npix * npix / dt / 1e9, 1),
                "Gtaps_per_s": round(2.0 * (2 * radius + 1) * npix * npix / dt / 1e9, 1)}

    result = {"data": "synthetic (lognormal point sources convolved with a PSF from device_ms2dirty(psf=True) on real "
                      "uvw tracks, then smoothed with every scale)",
              "npix": npix, "widths": widths, "sources": args.sources, "gain": gain, "rows": args.rows,
              "channels": args.nchan, "batch": args.batch or _lib.CIP_CLEAN_DEFAULT_BATCH, "repeat": args.repeat,
              "metric": "us per iteration (device_ms_clean, full PSF, fp64)", "unit": "us/iteration"}
    result["convolve"] = [convolve(32, 12.0), convolve(128, 49.0)]
    result["patch"] = case(min(args.patch, npix), args.niter)
    result["full_psf"] = case(npix, min(args.niter, args.full_niter))
    result["value"] = result["full_psf"]["us_per_iteration"]
    if npix == 8192 and nscales == 4:  # the row DESIGN.md 18 quotes
        (ROOT / "profiles" / "ms_clean_c3.json").write_text(json.dumps(result, indent=1) + "\n")
    return result


def weights(args):
    """ms of the imaging-weights calls, of the invert and of a torch restatement, all on C3's inputs."""
    import torch

    sys.path.insert(0, str(ROOT))
    import bench  # the flagship workload's own inputs

    from ska_sdp_cip_amd import gridder, weighting

    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[args.config]
    uvw, freq, vis, wgt, px, _, _ = bench.make_inputs(cfg, 0, 1, dev)
    npix, nrow, nchan = cfg["npix"], cfg["rows"], cfg["nchan"]
    nvis = nrow * nchan

    def best(fn):
        fn()  # warm-up: workspace buffers
        times = []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return min(times) * 1e3

    wd = weighting.WeightDensity(npix, npix, px, px, float(wgt.max()), nvis, dev)
    out = torch.empty_like(wgt)

    def density():
        wd.density.zero_()
        wd.add_ms(uvw, freq, wgt)

    ms_density = best(density)
    ms_stats = best(lambda: wd.finish("uniform"))
    ms_apply = best(lambda: wd.apply(uvw, freq, wgt, out=out))
    info = {}

    def one_shot():
        info.update(weighting.device_imaging_weights(uvw, freq, wgt, npix, npix, px, px, weighting="uniform",
                                                     out=out)[1])

    ms_total = best(one_shot)
    ms_invert = best(lambda: gridder.device_ms2dirty(uvw, freq, vis, wgt, npix, npix, px, px, support=8,
                                                     do_wstacking=False))
    hx = hy = npix // 2
    sx = float(npix) * px
    keep = {}

    def torch_cells():
        wi = freq / 299792458.0
        x = wi[None, :] * (uvw[:, 0] * sx)[:, None]
        y = wi[None, :] * (uvw[:, 1] * sx)[:, None]
        sign = torch.where((y < 0) | ((y == 0) & (x < 0)), -1.0, 1.0)
        fx, fy = torch.floor(sign * x + 0.5), torch.floor(sign * y + 0.5)
        inside = (fx.abs() <= hx) & (fy <= hy)
        return torch.where(inside, (fx + hx) * (hy + 1) + fy, -1.0).to(torch.int64), inside

    def torch_run():
        cell, inside = torch_cells()
        flat = cell.clamp_(min=0).view(-1)
        w64 = torch.where(inside, wgt.to(torch.float64), 0.0).view(-1)
        dens = torch.bincount(flat, weights=w64, minlength=(2 * hx + 1) * (hy + 1))
        d = dens[flat]
        keep["w"] = torch.where(d > 0, w64 / d, 0.0).to(torch.float32).view(nrow, nchan)

    ms_torch = best(torch_run)
    rel = ((keep["w"].double() - out.double()).abs() / out.double().clamp(min=1e-300)).max().item()
    # the atomics the density kernel issues: a lane merges equal cells of consecutive samples it adds
    # within its 16 channels (zero weights and outside samples are skipped, not run breaks)
    cell, inside = torch_cells()
    added = inside & (wgt > 0)
    key = torch.where(added, cell, -2)
    atomics = 0
    for c0 in range(0, nchan, 16):
        seg, on = key[:, c0:c0 + 16], added[:, c0:c0 + 16]
        last = torch.full((nrow,), -2, dtype=torch.int64, device=dev)
        for k in range(seg.shape[1]):
            atomics += int((on[:, k] & (seg[:, k] != last)).sum())
            last = torch.where(on[:, k], seg[:, k], last)
    n_added = int(added.sum())
    return {"data": f"bench.py {args.config} inputs and geometry (synthetic uvw tracks, float32 weights, 5% zero)",
            "rows": nrow, "channels": nchan, "npix": npix, "visibilities": nvis,
            "metric": "ms per imaging-weights step (uniform, float32 in and out), best of repeats",
            "value": round(ms_total, 3), "unit": "ms", "repeat": args.repeat,
            "density_ms": round(ms_density, 3), "stats_ms": round(ms_stats, 3), "apply_ms": round(ms_apply, 3),
            "one_shot_total_ms": round(ms_total, 3), "ms2dirty_sync_ms": round(ms_invert, 3),
            "torch_restatement_ms": round(ms_torch, 3),
            "torch_restatement": "fp64 cell index, torch.bincount(weights=fp64), gather, divide, to float32",
            "speedup_over_torch": round(ms_torch / ms_total, 2),
            "torch_max_rel_diff": rel, "torch_weights_agree": bool(rel < 1e-5),
            "n_added": n_added, "n_outside": info["n_outside"], "n_cells": info["n_cells"],
            "density_atomics": atomics, "mean_merged_run": round(n_added / max(atomics, 1), 2),
            "density_GBs_at_4B_per_vis": round(4.0 * nvis / ms_density / 1e6, 1),
            "apply_GBs_at_8B_per_vis": round(8.0 * nvis / ms_apply / 1e6, 1)}


def gaincal(args):
    """ms of the gain-calibration calls, of a torch restatement of the correlate and of a read-only stream of the
    same bytes, all on C3's inputs."""
    import torch

    sys.path.insert(0, str(ROOT))
    import bench  # the flagship workload's own inputs

    from ska_sdp_cip_amd import calibrate
    from ska_sdp_cip_amd import synthetic as syn

    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[args.config]
    result = _gaincal_case(args, cfg, bench, calibrate, syn, dev)
    if cfg["nchan"] != 64:  # the same samples as rows of 64 channels: 16 lanes per row, four rows per wave
        torch.cuda.empty_cache()
        narrow = dict(cfg, rows=cfg["rows"] * cfg["nchan"] // 64, nchan=64)
        result["rows_of_64_channels"] = _gaincal_case(args, narrow, bench, calibrate, syn, dev)
    if args.config == "c3":  # the rows DESIGN.md 16 quotes
        (ROOT / "profiles" / "gaincal_c3.json").write_text(json.dumps(result, indent=1) + "\n")
    return result


def _gaincal_case(args, cfg, bench, calibrate, syn, dev):
    """One shape of `gaincal`."""
    import torch

    _, _, model, wgt, _, _, _ = bench.make_inputs(cfg, 0, 1, dev)
    nrow, nchan, n_ant, dumps = cfg["rows"], cfg["nchan"], 64, 16
    nvis = nrow * nchan
    a1, a2, t = (torch.from_numpy(a).to(dev) for a in syn.baseline_indices(nrow, n_ant))
    interval = calibrate.solution_intervals(t, dumps)
    n_int = int(interval.max()) + 1
    truth = torch.from_numpy(syn.random_gains(n_int, n_ant, 0.2, 0.6, np.random.default_rng(1))).to(dev)
    alive = torch.ones((n_int, n_ant), dtype=torch.uint8, device=dev)
    # the data: the model column with the gains multiplied in
    vis, _ = calibrate.device_gain_apply(model, None, a1, a2, interval, truth, alive, mode="corrupt")
    cols = (a1, a2, interval)

    def best(fn):
        fn()  # warm-up: workspace buffers
        times = []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return min(times) * 1e3

    amax = float(max(torch.view_as_real(vis).abs().max(), torch.view_as_real(model).abs().max()))
    gc = calibrate.GainCorrelator(n_ant, n_int, amax, float(wgt.max()), nvis, dev)
    counts = {}

    def correlate():
        gc.corr.zero_()
        counts.update(gc.add_ms(vis, model, wgt, *cols))

    ms_correlate = best(correlate)
    solved = {}

    def solve():
        solved["out"] = gc.solve(niter=50, tol=0.0, refant=0)  # tol 0: all 50 iterations

    ms_solve = best(solve)
    gains, ok, _, _ = gc.solve(niter=50, tol=1e-8, refant=0)
    out_vis, out_wgt = torch.empty_like(vis), torch.empty_like(wgt)
    ms_apply = best(lambda: calibrate.device_gain_apply(vis, wgt, *cols, gains, ok, out=out_vis, wgt_out=out_wgt))
    info = {}

    def one_shot():
        info.update(calibrate.device_gaincal(vis, model, wgt, *cols, n_ant, n_int, niter=50, tol=1e-8, refant=0)[2])

    ms_total = best(one_shot)
    keep = {}

    def torch_run():
        key = (interval.to(torch.int64) * n_ant + a1) * n_ant + a2
        w64 = wgt.to(torch.float64)
        m128 = model.to(torch.complex128)
        c = (w64 * (vis.to(torch.complex128) * m128.conj())).sum(1)
        m2 = (w64 * (m128.real * m128.real + m128.imag * m128.imag)).sum(1)
        acc = torch.zeros((n_int * n_ant * n_ant, 3), dtype=torch.float64, device=dev)
        acc.index_add_(0, key, torch.stack([c.real, c.imag, m2], 1))
        keep["corr"] = acc.view(n_int, n_ant, n_ant, 3)

    ms_torch = best(torch_run)
    keep["sums"] = None

    def stream():  # reads the same 20 bytes per sample and nothing else
        keep["sums"] = (torch.view_as_real(vis).sum(), torch.view_as_real(model).sum(), wgt.sum())

    ms_stream = best(stream)
    mine = gc.corr.to(torch.float64) * gc.scale.quantum
    rel = float((mine - keep["corr"]).abs().max() / keep["corr"].abs().max())
    ref = truth * (truth[:, :1].conj() / truth[:, :1].abs())
    err = float((gains - ref).abs().max())
    bytes_per = 20.0
    result = {"data": f"bench.py {args.config} inputs (complex64 model column with seeded gains multiplied in, "
                      "float32 weights, 5% zero), baseline_indices of 64 antennas, intervals of 16 dumps",
              "rows": nrow, "channels": nchan, "visibilities": nvis, "n_ant": n_ant, "n_int": n_int,
              "metric": "ms per gain-calibration step, best of repeats", "value": round(ms_total, 3), "unit": "ms",
              "repeat": args.repeat, "correlate_ms": round(ms_correlate, 3), "solve_50_iterations_ms": round(ms_solve, 3),
              "apply_ms": round(ms_apply, 3), "one_shot_total_ms": round(ms_total, 3),
              "one_shot_iterations": int(info["max_iter_done"]),
              "torch_restatement_ms": round(ms_torch, 3),
              "torch_restatement": "fp64 w v conj(m) and w |m|^2, row sums, index_add_ into (n_int n_ant^2, 3)",
              "one_shot_speedup_over_torch_correlate": round(ms_torch / ms_total, 2),
              "correlate_speedup_over_torch": round(ms_torch / ms_correlate, 2),
              "torch_max_rel_diff": rel, "read_stream_ms": round(ms_stream, 3),
              "read_stream": "torch sums of vis, model and wgt: the same 20 bytes per sample",
              "correlate_GBs_at_20B_per_vis": round(bytes_per * nvis / ms_correlate / 1e6, 1),
              "read_stream_GBs": round(bytes_per * nvis / ms_stream / 1e6, 1),
              "apply_GBs_at_24B_per_vis": round(24.0 * nvis / ms_apply / 1e6, 1),
              "correlate_atomics": 3 * nrow, "n_added": counts["n_added"], "n_zero": counts["n_zero"],
              "n_outside": counts["n_outside"], "n_bad": counts["n_bad"], "shift": int(gc.scale.shift),
              "max_gain_error": err}
    return result


def dft(args):
    """ms per device_dft_predict call and per torch restatement of the same sum, on C3's rows."""
    import torch

    sys.path.insert(0, str(ROOT))
    import bench  # the flagship workload's own rows

    from ska_sdp_cip_amd import skymodel

    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[args.config]
    uvw, freq, _, wgt, px, _, _ = bench.make_inputs(cfg, 0, 1, dev)
    nrow, nchan = cfg["rows"], cfg["nchan"]
    nvis = nrow * nchan
    fx = freq / 299792458.0
    out = torch.empty((nrow, nchan), dtype=torch.complex64, device=dev)

    def best(fn, repeat):
        times = []
        for _ in range(repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return min(times) * 1e3

    def sky_of(ncomp, gauss):
        rng = np.random.default_rng(ncomp)
        fov = cfg["npix"] * px  # inside the C3 image
        lm = rng.uniform(-fov / 2, fov / 2, (ncomp, 2))
        flux = rng.uniform(0.1, 1.0, (ncomp, 1))
        shape = None
        if gauss:
            major = rng.uniform(2.0, 20.0, ncomp) * px
            shape = torch.from_numpy(np.stack([major, major * rng.uniform(0.3, 1.0, ncomp),
                                               rng.uniform(-np.pi, np.pi, ncomp)], axis=1))
        return skymodel.SkyModel(torch.from_numpy(lm), torch.from_numpy(flux), shape=shape).to(dev)

    def torch_run(sky, keep, chunk=16_384):  # the same sum in fp64: w term, envelope, weights, one rounding
        l, m = sky.lm[:, 0], sky.lm[:, 1]  # noqa: E741
        nm1 = -(l * l + m * m) / (torch.sqrt(1.0 - l * l - m * m) + 1.0)
        res = torch.empty_like(out)
        for a in range(0, nrow, chunk):
            u, v, w = (uvw[a:a + chunk, k:k + 1] for k in range(3))
            acc = torch.zeros((u.shape[0], nchan), dtype=torch.complex128, device=dev)
            for k in range(len(sky)):
                ph = (u * l[k] + v * m[k] - w * nm1[k]) * fx[None, :]
                term = torch.polar(sky.flux[k, 0].expand_as(ph), (-2.0 * np.pi) * (ph - torch.round(ph)))
                if sky.shape is not None:
                    sp, cp = torch.sin(sky.shape[k, 2]), torch.cos(sky.shape[k, 2])
                    q = 3.559707331246876 * ((sky.shape[k, 0] * (u * sp + v * cp)) ** 2
                                              + (sky.shape[k, 1] * (u * cp - v * sp)) ** 2)
                    term = term * torch.exp(-(fx * fx)[None, :] * q)
                acc += term
            res[a:a + chunk] = (wgt[a:a + chunk].to(torch.float64) * acc).to(torch.complex64)
        keep["torch"] = res

    cases = []
    for ncomp in (64, 1024):
        for gauss in (False, True):
            sky = sky_of(ncomp, gauss)
            row = {"ncomp": ncomp, "components": "gaussians" if gauss else "points", "pairs": nvis * ncomp}
            sigma = float(sky.flux.abs().sum())
            for name, fast in (("fp64", False), ("fast", True)):
                run = lambda: skymodel.device_dft_predict(uvw, freq, sky, wgt, out=out, fast=fast)  # noqa: E731
                run()  # warm-up: code object, workspace
                ms = best(run, args.repeat)
                row[f"{name}_ms"] = round(ms, 3)
                row[f"{name}_pairs_per_s"] = float(f"{nvis * ncomp / ms * 1e3:.4g}")
                row[f"{name}_column"] = out.clone() if name == "fp64" else None
            keep = {}
            if ncomp == 64:
                torch_run(sky_of(2, gauss), keep)  # warm-up at two components
            row["torch_fp64_ms"] = round(best(lambda: torch_run(sky, keep), args.repeat if ncomp == 64 else 1), 3)
            row["torch_runs"] = args.repeat if ncomp == 64 else 1
            row["fp64_speedup_over_torch"] = round(row["torch_fp64_ms"] / row["fp64_ms"], 1)
            row["fast_speedup_over_torch"] = round(row["torch_fp64_ms"] / row["fast_ms"], 1)
            row["fp64_vs_torch_max_diff_over_sigma"] = float((row.pop("fp64_column") - keep["torch"]).abs().max()) / sigma
            row.pop("fast_column")
            cases.append(row)
            del keep
            torch.cuda.empty_cache()
    result = {"data": f"bench.py {args.config} rows and weights (float32, 5% zero), seeded components inside the "
                      "image, one Taylor term, w term on, complex64 output",
              "rows": nrow, "channels": nchan, "visibilities": nvis,
              "metric": "ms per device_dft_predict call, best of repeats around a synchronised call",
              "value": cases[0]["fast_ms"], "unit": "ms", "repeat": args.repeat,
              "torch_restatement": "fp64, rows in chunks of 16384: path, phase reduced by round(), torch.polar, "
                                   "envelope exp, sum over components, weights, one rounding to complex64",
              "cases": cases}
    if args.config == "c3":  # the rows DESIGN.md 17 quotes
        (ROOT / "profiles" / "dft_predict_c3.json").write_text(json.dumps(result, indent=1) + "\n")
    return result


def restore(args):
    """ms per device_restore call (sparse and dense model) and per torch conv2d / fft2 restatement."""
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, str(ROOT))
    import bench  # the flagship workload's own inputs

    from ska_sdp_cip_amd import _lib, gridder, restore as rst

    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[args.config]
    uvw, freq, _, wgt, px, _, _ = bench.make_inputs(cfg, 0, 1, dev)
    psf, _ = gridder.device_ms2dirty(uvw, freq, None, wgt, cfg["npix"], cfg["npix"], px, px, support=8, psf=True,
                                     normalise=True)
    c = cfg["npix"] // 2
    psf = psf[c - 64:c + 65, c - 64:c + 65].contiguous()  # the cut keeps the peak at the patch's centre
    del uvw, wgt
    _lib.lib().cip_release_workspace()  # the invert's grid is not needed any more
    beam = rst.device_fit_beam(psf)
    try:
        radius = rst.beam_radius(beam)
    except ValueError:  # wider than 12.5 px: the largest support, the beam cut off above 1e-8
        radius = _lib.RESTORE_MAX_RADIUS
    taps =torch.from_numpy(rst.beam_taps(beam, radius)).to(dev)
    n = args.restore_npix
    g = torch.Generator(device=dev)
    g.manual_seed(20241020)
    residual = torch.randn((n, n), dtype=torch.float64, device=dev, generator=g)
    out = torch.empty_like(residual)

    def best(fn):
        fn()  # warm-up: workspace, the tap table, torch's own plans
        times = []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return min(times) * 1e3

    def torch_conv(model, dst):
        # dense fp64 conv2d in strips of rows: the unfolded strip stays under ~4 GB
        w = taps.flip(0, 1)[None, None]
        strip = max(32, int(4e9 / (8.0 * n * taps.numel())))
        for i0 in range(0, n, strip):
            i1 = min(n, i0 + strip)
            lo, hi = max(0, i0 - radius), min(n, i1 + radius)
            part = F.pad(model[lo:hi], (radius, radius, radius - (i0 - lo), radius - (hi - i1)))
            dst[i0:i1] = F.conv2d(part[None, None], w)[0, 0] + residual[i0:i1]

    kernel = torch.zeros((n, n), dtype=torch.float64, device=dev)
    kernel[:2 * radius + 1, :2 * radius + 1] = taps
    kernel_f = torch.fft.rfft2(torch.roll(kernel, (-radius, -radius), (0, 1)))  # not timed: it belongs to the beam
    del kernel

    def torch_fft(model, dst):
        torch.add(torch.fft.irfft2(torch.fft.rfft2(model) * kernel_f, s=(n, n)), residual, out=dst)

    rng = np.random.default_rng(20241020)
    cases = {}
    for name in ("sparse", "dense"):
        model = torch.zeros((n, n), dtype=torch.float64, device=dev)
        if name == "sparse":
            idx = torch.from_numpy(rng.choice(n * n, size=args.components, replace=False)).to(dev)
            model.view(-1)[idx] = torch.from_numpy(rng.lognormal(0.0, 1.0, args.components)).to(dev)
        else:
            o, m = n // 2 - args.patch // 2, args.patch
            model[o:o + m, o:o + m] = torch.randn((m, m), dtype=torch.float64, device=dev, generator=g)
        row = {"nonzero": int(torch.count_nonzero(model))}
        row["restore_ms"] = round(best(lambda: rst.device_restore(model, residual, beam, radius=radius, out=out)), 4)
        inplace = residual.clone()
        row["restore_inplace_ms"] = round(
            best(lambda: rst.device_restore(model, inplace, beam, radius=radius, inplace=True)), 4)
        del inplace
        first = out.clone()
        rst.device_restore(model, residual, beam, radius=radius, out=out)
        row["identical_bits_on_repeat"] = bool(torch.equal(first.view(torch.int64), out.view(torch.int64)))
        other = torch.empty_like(out)
        for what, fn in (("torch_conv2d", torch_conv), ("torch_fft2", torch_fft)):
            try:
                row[what + "_ms"] = round(best(lambda: fn(model, other)), 3)
                row[what + "_max_abs_diff"] = float((other - first).abs().max())
                # away from the border: the fft2 form is circular, it wraps components near an edge around
                row[what + "_max_abs_diff_interior"] = float(
                    (other - first)[radius:n - radius, radius:n - radius].abs().max())
                row["speedup_over_" + what] = round(row[what + "_ms"] / row["restore_ms"], 2)
            except RuntimeError as exc:  # e.g. no fp64 convolution on this build
                row[what + "_error"] = str(exc).splitlines()[0][:200]
        del other, first, model
        cases[name] = row
    # the floor: the bytes a restore has to move (model and residual read, out written)
    copy_ms = best(lambda: torch.add(residual, residual, out=out))
    result = {"data": f"beam fitted to a 129^2 cut of device_ms2dirty(psf=True) on bench.py {args.config} inputs; "
                      f"seeded {n}^2 residual; sparse: {args.components} seeded lognormal pixels; dense: a "
                      f"{args.patch}^2 normal patch",
              "npix": n, "beam": beam, "radius": radius, "taps": int(taps.numel()),
              "metric": "ms per device_restore call (sparse model, fp64), best of repeats",
              "value": cases["sparse"]["restore_ms"], "unit": "ms", "repeat": args.repeat,
              "sparse": cases["sparse"], "dense": cases["dense"],
              "torch_add_two_reads_one_write_ms": round(copy_ms, 4),
              "GBs_at_24B_per_pixel_sparse": round(24.0 * n * n / cases["sparse"]["restore_ms"] / 1e6, 1)}
    path = ROOT / "profiles" / f"restore_{args.config}.json"
    path.write_text(json.dumps(result, indent=1) + "\n")
    return result

SELECT_DIGITS = (12, 13, 13, 13, 13)  # kSelBits of csrc/cip_noise.hip
SELECT_COMPACT_CAP = 1 << 16  # kCompactCap


def _select_replay(values, rank):
    """The radix select of csrc/cip_noise.hip replayed in numpy on the finite
    `values`: (the value of `rank`, the full reads of the image it makes)."""
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    keys = np.where(bits >> np.uint64(63) != 0, ~bits, bits | top)
    shift, prefix, reads, compacted = 64, 0, 0, False
    for k, width in enumerate(SELECT_DIGITS):
        shift -= width
        digit = ((keys >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64)
        hist = np.bincount(digit, minlength=1 << width)
        reads += 0 if compacted else 1
        b = int(np.searchsorted(np.cumsum(hist), rank, side="right"))
        rank -= int(hist[:b].sum())
        prefix |= b << shift
        keys = keys[digit == b]
        if not compacted and k + 1 < len(SELECT_DIGITS) and keys.size <= SELECT_COMPACT_CAP:
            compacted, reads = True, reads + 1  # the compaction reads the image once more
    key = np.uint64(prefix)
    out = np.array([key & ~top if key >> np.uint64(63) else ~key], dtype=np.uint64)
    return float(out.view(np.float64)[0]), reads


def noise_rows(args):
    """ms per device_image_noise / device_auto_mask call beside torch.kthvalue, a copy and a C3 major cycle."""
    import torch

    sys.path.insert(0, str(ROOT))
    import bench  # the flagship workload's own inputs

    from ska_sdp_cip_amd import _lib, gridder, noise, predict, synthetic as syn

    dev = torch.device("cuda", 0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def scene(npix):
        """The image of --mode clean (lognormal point sources convolved with a PSF patch) plus Gaussian noise."""
        pn = min(args.patch, npix)
        uvw_h = syn.uvw_tracks(args.rows, 64, array_radius_m=4000.0)
        freq_h = syn.channel_frequencies(args.nchan)
        px = syn.pixel_size_for_grid(uvw_h, freq_h, npix, support=8)
        psf_full, _ = gridder.device_ms2dirty(torch.from_numpy(uvw_h).to(dev), torch.from_numpy(freq_h).to(dev), None,
                                              None, npix, npix, px, px, support=8, psf=True, normalise=True)
        o, c = npix // 2 - pn // 2, pn // 2
        psf = psf_full[o:o + pn, o:o + pn].contiguous()
        del psf_full
        _lib.lib().cip_release_workspace()  # the invert's grid is not needed any more
        rng = np.random.default_rng(20241019)
        g = torch.Generator(device=dev)
        g.manual_seed(20241021)
        image = torch.randn((npix, npix), dtype=torch.float64, device=dev, generator=g) * args.noise_sigma
        for i, j, flux in zip(rng.integers(0, npix, args.sources), rng.integers(0, npix, args.sources),
                              rng.lognormal(0.0, 1.0, args.sources)):
            i, j = int(i), int(j)
            i0, i1, j0, j1 = max(0, i - c), min(npix, i - c + pn), max(0, j - c), min(npix, j - c + pn)
            image[i0:i1, j0:j1] += float(flux) * psf[i0 - i + c:i1 - i + c, j0 - j + c:j1 - j + c]
        return image

    def torch_noise(image):
        flat = image.view(-1)
        k = (flat.numel() - 1) // 2 + 1  # kthvalue counts from 1
        median = torch.kthvalue(flat, k).values
        mad = torch.kthvalue((flat - median).abs(), k).values
        return float(median), float(mad)

    def noise_and_mask(image):
        got = noise.device_image_noise(image)
        return got, noise.device_auto_mask(image, 5.0 * got["sigma"], 3.0 * got["sigma"])[1]

    n = args.noise_npix
    image = scene(n)
    noise.device_image_noise(image)  # warm-up: workspace, kernels
    torch_noise(image)
    hip_ms, torch_ms = [], []
    for _ in range(args.repeat):  # interleaved: both see the same machine
        t, got = timed(lambda: noise.device_image_noise(image))
        hip_ms.append(round(t, 3))
        t, ref = timed(lambda: torch_noise(image))
        torch_ms.append(round(t, 3))
    # the same call with a region of ones: what the byte per pixel of the region costs
    ones = torch.ones((n, n), dtype=torch.uint8, device=dev)
    noise.device_image_noise(image, region=ones)
    region_ms = [round(timed(lambda: noise.device_image_noise(image, region=ones))[0], 3) for _ in range(args.repeat)]
    del ones
    host = image.cpu().numpy().ravel()
    rank = (host.size - 1) // 2
    median, reads_median = _select_replay(host, rank)
    mad, reads_mad = _select_replay(np.abs(host - median), rank)
    del host
    bytes_read = 8.0 * n * n * (reads_median + reads_mad)
    other = torch.empty_like(image)
    other.copy_(image)
    copy_ms = min(timed(lambda: other.copy_(image))[0] for _ in range(args.repeat))
    del other
    noise_and_mask(image)
    mask_ms, rounds, minfo = [], None, None
    for _ in range(args.repeat):
        t, (_, minfo) = timed(lambda: noise.device_auto_mask(image, 5.0 * got["sigma"], 3.0 * got["sigma"]))
        mask_ms.append(round(t, 3))
    result = {
        "data": f"the scene of --mode clean at {n}^2 ({args.sources} lognormal sources, {min(args.patch, n)}^2 PSF patch) "
                f"plus seeded Gaussian pixel noise of sigma {args.noise_sigma}",
        "npix": n, "repeat": args.repeat, "noise": got,
        "metric": "ms per device_image_noise call (median + MAD of an fp64 image), best of repeats",
        "value": min(hip_ms), "unit": "ms",
        "device_image_noise_ms": hip_ms, "torch_kthvalue_pair_ms": torch_ms,
        "device_image_noise_with_region_of_ones_ms": region_ms,
        "spread_ms": {"device_image_noise": round(max(hip_ms) - min(hip_ms), 3),
                      "torch_kthvalue_pair": round(max(torch_ms) - min(torch_ms), 3)},
        "speedup_over_torch_kthvalue_pair": round(min(torch_ms) / min(hip_ms), 2),
        "equal_to_torch": bool(got["median"] == ref[0] and got["mad"] == ref[1]),
        "equal_to_numpy_replay": bool(got["median"] == median and got["mad"] == mad),
        "full_image_reads": {"median": reads_median, "mad": reads_mad},
        "GBs_at_8B_per_pixel_per_read": round(bytes_read / min(hip_ms) / 1e6, 1),
        "device_copy_ms": round(copy_ms, 3), "device_copy_GBs_read_plus_write": round(16.0 * n * n / copy_ms / 1e6, 1),
        "auto_mask_5_3_ms": mask_ms, "auto_mask": minfo,
    }
    del image
    # one major cycle at C3: the predict of a model image and the re-invert through the first invert's plan
    cfg = bench.CONFIGS[args.config]
    uvw, freq, vis, wgt, px, _, _ = bench.make_inputs(cfg, 0, 1, dev)
    m = cfg["npix"]
    kw = dict(support=8, do_wstacking=False)
    residual, _ = gridder.device_ms2dirty(uvw, freq, vis, wgt, m, m, px, px, normalise=True, **kw)
    model = torch.zeros((m, m), dtype=torch.float64, device=dev)
    model.view(-1)[torch.from_numpy(np.random.default_rng(3).choice(m * m, 1000, replace=False)).to(dev)] = 1.0

    def cycle():
        vres = predict.device_residual(uvw, freq, vis, model, px, None, reuse_plan=True, **kw)
        gridder.device_ms2dirty(uvw, freq, vres, wgt, m, m, px, px, normalise=True, reuse_plan=True, out=residual, **kw)

    cycle()
    cycle_ms = min(timed(cycle)[0] for _ in range(args.repeat))
    del uvw, vis, wgt, model
    image = scene(m)
    noise_and_mask(image)
    both_ms = min(timed(lambda: noise_and_mask(image))[0] for _ in range(args.repeat))
    result["major_cycle"] = {
        "config": args.config, "npix": m, "visibilities": cfg["rows"] * cfg["nchan"],
        "predict_plus_reinvert_ms": round(cycle_ms, 2), "noise_plus_mask_ms": round(both_ms, 3),
        "noise_plus_mask_share_of_cycle": round(both_ms / cycle_ms, 4)}
    path = ROOT / "profiles" / f"noise_{args.config}.json"
    path.write_text(json.dumps(result, indent=1) + "\n")
    return result


def mosaic_rows(args):
    """ms per MosaicAccumulator.add and per mosaic at C5's size, LDS staging against direct loads, beside the traffic floor."""
    import os

    import torch

    from ska_sdp_cip_amd import synthetic as syn
    from ska_sdp_cip_amd.mosaic import MosaicAccumulator, facet_layout

    dev = torch.device("cuda", 0)
    fx, fy = args.facets_xy or (8, 4)
    fn, half, nplane = args.mosaic_facet, args.mosaic_half, args.mosaic_planes
    # C5's pixel size (tests/test_gpu_c5.py): C3's tracks imaged on 4096^2 facets
    uvw = syn.uvw_tracks(390_625, 64, array_radius_m=4000.0, seed=20241008)
    freq = syn.channel_frequencies(256)
    px = syn.pixel_size_for_grid(uvw, freq, 4096, support=8)
    nu_max = float(np.abs(uvw[:, :2]).max() * freq.max() / syn.SPEED_OF_LIGHT * px)
    del uvw
    # the largest plane that `facet_layout` covers with fx x fy such facets
    span = fn - 2 * half + 1
    nx, ny = fx * span, fy * span
    while len(centres := facet_layout(nx, ny, px, fn, half=half)) != fx * fy:
        nx, ny = nx - fx, ny - fy
    g = torch.Generator(device=dev)
    g.manual_seed(20241022)
    facet = torch.randn((nplane, fn, fn), dtype=torch.float64, device=dev, generator=g)

    def timed(fn_):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn_()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def one_mosaic(lds, planes=nplane):
        os.environ["CIP_MOSAIC_LDS"] = "1" if lds else "0"
        acc = MosaicAccumulator(nx, ny, px, px, planes, half=half, nu_max=nu_max)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        adds = [timed(lambda c=c: acc.add(facet[:planes], c[0], c[1]))[0] for c in centres]
        covered = float(acc.wsum.sum())  # feather 0: every weight is 1, so this counts the pixels the adds wrote
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        _, missed = acc.finish()
        torch.cuda.synchronize()
        return {"adds_ms": adds, "finish_ms": (time.perf_counter() - t1) * 1e3,
                "mosaic_ms": sum(adds) + (time.perf_counter() - t1) * 1e3, "covered": covered, "uncovered": missed,
                "wall_ms": (time.perf_counter() - t0) * 1e3}

    one_mosaic(True)  # warm-up: both kernels' code objects, the allocator
    one_mosaic(False)
    runs = {True: [], False: []}
    for _ in range(args.repeat):
        for lds in (True, False):
            runs[lds].append(one_mosaic(lds))
    # one plane: what an add costs before any plane's tap sums (the geometry and the taps) and per plane
    one_mosaic(True, 1)
    single = min(sum(one_mosaic(True, 1)["adds_ms"]) for _ in range(args.repeat)) / len(centres)
    os.environ.pop("CIP_MOSAIC_LDS", None)
    src = torch.empty((nx * ny,), dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    copy_ms = min(timed(lambda: dst.copy_(src))[0] for _ in range(args.repeat + 1))
    copy_gbs = 2 * src.numel() * 8 / copy_ms / 1e6
    del src, dst
    covered = runs[True][0]["covered"]
    facet_bytes = nplane * fn * fn * 8
    # each facet read once; num (nplane) and wsum of the footprint read and written once
    floor_bytes = len(centres) * facet_bytes + covered * (nplane + 1) * 16
    fma = covered * nplane * 4 * half * half

    def summary(rs):
        best = min(rs, key=lambda r: sum(r["adds_ms"]))
        adds_ms = sum(best["adds_ms"])
        return {"add_ms_best": round(min(best["adds_ms"]), 3), "add_ms_median": round(float(np.median(best["adds_ms"])), 3),
                "adds_ms_total": round(adds_ms, 2), "finish_ms": round(min(r["finish_ms"] for r in rs), 2),
                "mosaic_ms": round(min(r["mosaic_ms"] for r in rs), 2),
                "adds_ms_total_all_repeats": [round(sum(r["adds_ms"]), 2) for r in rs],
                "floor_GBs": round(floor_bytes / adds_ms / 1e6, 1),
                "fraction_of_copy_rate": round(floor_bytes / adds_ms / 1e6 / copy_gbs, 3),
                "tap_sum_fp64_TFMAs": round(fma / adds_ms / 1e9, 2)}

    result = {
        "data": "standard-normal facet planes (pure resampling: the values do not matter)",
        "facets": [fx, fy], "facet_pixels": fn, "planes": nplane, "half": half, "plane": [nx, ny],
        "pixel_size": px, "field_rad": [round(nx * px, 4), round(ny * px, 4)], "nu_max": round(nu_max, 4),
        "repeat": args.repeat, "uncovered": runs[True][0]["uncovered"],
        "metric": "ms per MosaicAccumulator.add (one facet, all planes), synchronised around each call",
        "covered_pixels_over_all_adds": covered, "traffic_floor_bytes": floor_bytes,
        "traffic_floor": "each facet read once + read and write of the footprint's num and wsum",
        "tap_sum_fma": fma, "device_copy_GBs": round(copy_gbs, 1),
        "lds_staging": summary(runs[True]), "direct_loads": summary(runs[False]),
    }
    if nplane > 1:
        mean = result["lds_staging"]["adds_ms_total"] / len(centres)
        per_plane = (mean - single) / (nplane - 1)
        result["plane_scaling_lds"] = {"add_ms_mean": round(mean, 3), "add_ms_mean_one_plane": round(single, 3),
                                       "ms_per_plane": round(per_plane, 3),
                                       "ms_geometry_and_taps": round(single - per_plane, 3)}
    path = ROOT / "profiles" / "mosaic_c5.json"
    path.write_text(json.dumps(result, indent=1) + "\n")
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("stream", "continuum", "degrid", "clean", "mfs_clean", "ms_clean", "weights",
                                      "restore", "gaincal", "dft", "noise", "mosaic"), required=True)
    ap.add_argument("--config", default="c3", help="weights / restore / gaincal / dft: the bench.py configuration whose inputs are used")
    ap.add_argument("--rows", type=int, default=156_250)
    ap.add_argument("--nchan", type=int, default=64)
    ap.add_argument("--npix", type=int, default=2048)
    ap.add_argument("--rows-per-chunk", type=int, default=32_768)
    ap.add_argument("--facets", type=int, default=2, help="facets per axis (continuum)")
    ap.add_argument("--facets-xy", type=int, nargs=2, default=None, help="continuum: facets along x and y")
    ap.add_argument("--world", type=int, default=1,
                    help="continuum: time rank 0's share of the facets of a `world`-GPU run (k %% world == 0)")
    ap.add_argument("--refcall", action="store_true",
                    help="continuum / degrid: the reference's gridder call (epsilon 1e-4, w-stacking; continuum: "
                         "float class) instead of 2-D support 8 fp64")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--psf-npix", type=int, default=None, help="clean: PSF edge (default: --npix)")
    ap.add_argument("--niter", type=int, default=1000, help="clean: iterations")
    ap.add_argument("--gain", type=float, default=0.1, help="clean: loop gain")
    ap.add_argument("--sources", type=int, default=300, help="clean: point sources in the image")
    ap.add_argument("--batch", type=int, default=0, help="clean: iterations queued per readback (0: default)")
    ap.add_argument("--nterms", type=int, default=2, help="mfs_clean: Taylor terms")
    ap.add_argument("--torch-niter", type=int, default=100, help="mfs_clean: iterations of the torch loop")
    ap.add_argument("--restore-npix", type=int, default=8192, help="restore: image edge")
    ap.add_argument("--components", type=int, default=10_000, help="restore: non-zero pixels of the sparse model")
    ap.add_argument("--patch", type=int, default=512,
                    help="restore: edge of the dense model patch; mfs_clean / ms_clean: edge of the PSF patch")
    ap.add_argument("--widths", type=float, nargs="+", default=[0.0, 4.0, 8.0, 16.0],
                    help="ms_clean: scale FWHMs in pixels")
    ap.add_argument("--full-niter", type=int, default=200, help="ms_clean: iterations of the full-PSF case at most")
    ap.add_argument("--noise-npix", type=int, default=8192, help="noise: image edge")
    ap.add_argument("--noise-sigma", type=float, default=0.05, help="noise: sigma of the added pixel noise")
    ap.add_argument("--mosaic-facet", type=int, default=4096, help="mosaic: facet edge")
    ap.add_argument("--mosaic-planes", type=int, default=4, help="mosaic: planes per facet")
    ap.add_argument("--mosaic-half", type=int, default=6, help="mosaic: taps either side")
    ap.add_argument("--no-reuse", action="store_true", help="continuum: plan every product (no CIP_REUSE_PLAN)")
    args = ap.parse_args()

    import torch

    from ska_sdp_cip_amd import synthetic as syn

    if args.mode == "degrid":
        print(json.dumps(degrid(args)), flush=True)
        return
    if args.mode == "weights":
        print(json.dumps(weights(args)), flush=True)
        return
    if args.mode == "restore":
        print(json.dumps(restore(args)), flush=True)
        return
    if args.mode == "gaincal":
        print(json.dumps(gaincal(args)), flush=True)
        return
    if args.mode == "dft":
        print(json.dumps(dft(args)), flush=True)
        return
    if args.mode == "noise":
        print(json.dumps(noise_rows(args)), flush=True)
        return
    if args.mode == "mosaic":
        print(json.dumps(mosaic_rows(args)), flush=True)
        return
    if args.mode == "mfs_clean":
        print(json.dumps(mfs_clean(args)), flush=True)
        return
    if args.mode == "ms_clean":
        print(json.dumps(ms_clean(args)), flush=True)
        return
    if args.mode == "clean":
        if args.psf_npix is None:
            args.psf_npix = args.npix
        print(json.dumps(clean(args)), flush=True)
        return
    ms = syn.make_measurement_set(args.rows, args.nchan, n_ant=64, array_radius_m=4000.0, cheap_visibilities=True)
    uvw, freq = ms.uvw(), ms.channel_frequencies()
    px = syn.pixel_size_for_grid(uvw, freq, args.npix, support=8)
    asec = float(np.degrees(np.arcsin(px)) * 3600.0)
    nvis = args.rows * args.nchan
    out = {"data": "synthetic (real uvw tracks, random complex64 values, 4 pols, 5% flagged)",
           "rows": args.rows, "channels": args.nchan, "npix": args.npix, "visibilities": nvis}
    if args.mode == "stream":
        from ska_sdp_cip_amd.streaming import invert_measurement_set_streamed

        run = lambda: invert_measurement_set_streamed(ms, args.npix, asec,  # noqa: E731
                                                      rows_per_chunk=args.rows_per_chunk, support=8)
        run()  # warm-up: workspace, pinned slots, FFT tables
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.repeat):
            run()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.repeat
        host_bytes = nvis * (8 * 4 + 1 * 4 + 4 * 4) + args.rows * 24
        out.update(metric="Mvis/s streamed host->HBM + invert (2-D, support 8)", value=round(nvis / dt / 1e6, 1),
                   unit="Mvis/s", ms_per_call=round(dt * 1e3, 2), host_bytes=host_bytes,
                   host_to_device_GBs=round(host_bytes / dt / 1e9, 1), rows_per_chunk=args.rows_per_chunk)
    else:
        from ska_sdp_cip_amd.continuum import continuum_invert, facet_centres

        dev = torch.device("cuda", 0)
        t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else a.astype(dt))).to(dev)  # noqa
        cols = (t(ms.visibilities()), t(ms.flags(), np.uint8), t(ms.weights()), t(uvw), t(freq))
        fx, fy = args.facets_xy or (args.facets, args.facets)
        facets = facet_centres(fx, fy, args.npix, px)
        call = (dict(epsilon=1e-4, do_wstacking=True, single_precision_accumulation=True) if args.refcall else
                dict(support=8, do_wstacking=False))
        run = lambda: continuum_invert(*cols, args.npix, asec, facets=facets, stokes="IQUV",  # noqa: E731
                                       psf=True, rank=0, world=args.world, reuse_plans=not args.no_reuse, **call)
        run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.repeat):
            res = run()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.repeat
        nimg = len(res)
        mode = ("the reference's call: epsilon 1e-4, w-stacking, float class" if args.refcall else
                "2-D, support 8, fp64")
        out.update(metric=f"continuum products: Stokes IQUV + PSF per facet ({mode})", world=args.world,
                   value=round(nimg / dt, 2), unit="images/s", images=nimg, facets=len(facets),
                   facets_this_rank=nimg // 5,
                   ms_per_call=round(dt * 1e3, 2), mvis_per_s_per_image=round(nvis * nimg / dt / 1e6, 1),
                   reuse_plans=not args.no_reuse)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
