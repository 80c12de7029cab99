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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("stream", "continuum", "degrid", "clean"), required=True)
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
    ap.add_argument("--no-reuse", action="store_true", help="continuum: plan every product (no CIP_REUSE_PLAN)")
    args = ap.parse_args()

    import torch

    from ska_sdp_cip_amd import synthetic as syn

    if args.mode == "degrid":
        print(json.dumps(degrid(args)), flush=True)
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
