"""
Deconvolution: Hogbom CLEAN on the GPU (`cip_hogbom_clean`) and the
device-resident major-cycle loop that joins it to the invert
(`cip_ms2dirty`) and the predict (`cip_dirty2ms`).

The operator is defined exactly in include/cip.h: peak under the mask (ties
to the lowest flat index, NaN never selected), stop rule checked before
subtracting, `res[win] -= f * psf[win']` with every product rounded before it
is subtracted, so a run is bit-identical to that numpy statement.
"""

from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np

from . import _lib
from ._call import STREAM, call, check_array, require_gpu, target_device, to_device
from .gridder import device_ms2dirty
from .invert import DO_WSTACKING, EPSILON
from .noise import device_auto_mask, device_image_noise
from .predict import device_residual
from .restore import device_fit_beam, device_restore
from .weighting import device_imaging_weights

try:
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None

_PF64 = ctypes.POINTER(ctypes.c_double)


def _device_clean(residual, psf, hinv, stack, *, gain, threshold, niter, mask, model, psf_centre, inplace,
                  return_components, batch):
    """The minor cycle behind `device_hogbom_clean` (`stack` False: 2-D images,
    no `hinv`, `cip_hogbom_clean`), `mfs.device_mfs_clean` (`stack` True:
    stacks and the host matrix `hinv`, `cip_mfs_clean`) and
    `multiscale.device_ms_clean` (`stack` "ms": stacks, `hinv` is the pair of
    host arrays (select_weight, flux_scale), `cip_ms_clean`)."""
    require_gpu()
    dev = residual.device
    ms = stack == "ms"
    stack = bool(stack)
    names, kind = (("residuals", "psfs"), "stack of 2-D images") if stack else (("residual", "psf"), "2-D image")
    for name, img in zip(names, (residual, psf)):
        if img.dim() != 2 + stack:
            raise ValueError(f"{name} must be a float64 {kind}, got {img.dtype} {tuple(img.shape)}")
        check_array(img, (torch.float64,), None, dev, name)
    shape = tuple(residual.shape[-2:])
    # what cip_mfs_clean takes and cip_hogbom_clean does not: nterms (the stacks' first axis too) and hinv;
    # cip_ms_clean: nscales and its two host arrays
    terms = matrix = ()
    if ms:
        nscales = int(residual.shape[0])
        host = [np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float64)
                for x in hinv]
        # nscales itself (1 .. 6) and the entries of the arrays are the library's to refuse
        if any(x.shape != (nscales,) for x in host) or int(psf.shape[0]) != nscales * (nscales + 1) // 2:
            raise ValueError(f"{nscales} residual scales need select_weight and flux_scale of shape ({nscales},) and "
                             f"{nscales * (nscales + 1) // 2} cross PSFs, got {[x.shape for x in host]} and "
                             f"{int(psf.shape[0])} PSFs")
        terms, matrix = (nscales,), tuple(x.ctypes.data_as(_PF64) for x in host)
    elif stack:
        nterms = int(residual.shape[0])
        h = np.ascontiguousarray(hinv.detach().cpu().numpy() if torch.is_tensor(hinv) else hinv, dtype=np.float64)
        if h.ndim != 2 or h.shape[0] != h.shape[1]:
            raise ValueError(f"hinv must be a square (nterms, nterms) matrix, got {h.shape}")
        # nterms itself (1 .. 3) and the entries of hinv are the library's to refuse
        if h.shape[0] != nterms or int(psf.shape[0]) != 2 * nterms - 1:
            raise ValueError(f"{nterms} residual terms need hinv ({nterms}, {nterms}) and {2 * nterms - 1} PSFs, got "
                             f"hinv {h.shape} and {int(psf.shape[0])} PSFs")
        terms, matrix = (nterms,), (h.ctypes.data_as(_PF64),)
    if mask is not None:
        check_array(mask, (torch.uint8, torch.bool), shape, dev, "mask")
        mask = mask.view(torch.uint8)
    if model is not None:
        check_array(model, (torch.float64,), (*terms, *shape), dev, "model")
    cx, cy = (-1, -1) if psf_centre is None else (int(psf_centre[0]), int(psf_centre[1]))
    if psf_centre is not None and (cx < 0 or cy < 0):
        raise ValueError("psf_centre must lie inside the PSF")
    niter = int(niter)
    res = residual if inplace else residual.clone()
    if model is None:
        model = torch.zeros((*terms, *shape), dtype=torch.float64, device=dev)
    comp_index = comp_flux = None
    comp_scale = (None,) if ms else ()  # cip_ms_clean's third component array: the scale of each component
    if return_components:
        comp_index = torch.empty(max(niter, 1), dtype=torch.int64, device=dev)
        comp_flux = torch.empty((max(niter, 1), *(() if ms else terms)), dtype=torch.float64, device=dev)
        if ms:
            comp_scale = (torch.empty(max(niter, 1), dtype=torch.int64, device=dev),)
    result = _lib.MsResult() if ms else _lib.CleanResult()
    call(dev, "cip_ms_clean" if ms else "cip_mfs_clean" if stack else "cip_hogbom_clean", res, *terms, shape[0],
         shape[1], psf, int(psf.shape[-2]), int(psf.shape[-1]), cx, cy, *matrix, mask, float(gain), float(threshold),
         niter, int(batch), STREAM, model, comp_index, *comp_scale, comp_flux, ctypes.byref(result))
    info = {
        "niter_done": int(result.niter_done),
        "stop_reason": int(result.stop_reason),
        "stop": _lib.CLEAN_STOP_REASONS[int(result.stop_reason)],
        "peak": float(result.peak),
        "peak_index": int(result.peak_index),
    }
    if ms:
        info["peak_scale"] = int(result.peak_scale)
    if return_components:
        info["comp_index"] = comp_index[: info["niter_done"]]
        info["comp_flux"] = comp_flux[: info["niter_done"]]
        if ms:
            info["comp_scale"] = comp_scale[0][: info["niter_done"]]
    return model, res, info


def _host_clean(device_clean, residual, psf, *hinv, mask, model, return_components, device, **kw):
    """`hogbom_clean`, `mfs.mfs_clean` and `multiscale.ms_clean`: `device_clean`
    on copies of host or device arrays, numpy in -> numpy out."""
    require_gpu()
    dev = target_device(device)
    numpy_in = isinstance(residual, np.ndarray)
    with torch.cuda.device(dev):
        res_d = to_device(residual, torch.float64, dev)
        psf_d = to_device(psf, torch.float64, dev)
        mask_d = None
        if mask is not None:
            m = np.asarray(mask) if not torch.is_tensor(mask) else mask
            mask_d = to_device(m != 0, torch.bool, dev)
        model_d = None if model is None else to_device(model, torch.float64, dev).clone()
        model_d, res_d, info = device_clean(res_d, psf_d, *hinv, mask=mask_d, model=model_d, inplace=False,
                                            return_components=return_components, **kw)
        if numpy_in:
            model_d, res_d = model_d.cpu().numpy(), res_d.cpu().numpy()
            if return_components:
                for key in ("comp_index", "comp_flux", "comp_scale"):
                    if key in info:
                        info[key] = info[key].cpu().numpy()
    return model_d, res_d, info


def _auto_options(auto_threshold, auto_mask):
    """The two noise options as `_major_cycles` takes them: `auto_threshold` as a
    float, `auto_mask` as (seed_sigmas, grow_sigmas), a single number meaning
    both; None stays None. The drivers call this before any device work, so a
    bad option raises ValueError without an invert."""
    if auto_threshold is not None:
        auto_threshold = float(auto_threshold)
        if not auto_threshold >= 0.0:
            raise ValueError(f"auto_threshold must be >= 0 and not NaN, got {auto_threshold}")
    if auto_mask is not None:
        pair = tuple(auto_mask) if isinstance(auto_mask, (tuple, list)) else (auto_mask, auto_mask)
        if len(pair) != 2:
            raise ValueError(f"auto_mask must be (seed_sigmas, grow_sigmas) or one number, got {auto_mask!r}")
        seed, grow = float(pair[0]), float(pair[1])
        if not (math.isfinite(seed) and seed >= grow > 0.0):
            raise ValueError(f"auto_mask needs finite seed_sigmas >= grow_sigmas > 0, got {auto_mask!r}")
        auto_mask = (seed, grow)
    return auto_threshold, auto_mask


def _major_cycles(result, n_major, threshold, cycle_fraction, clean, reinvert, restore, *, mask=None,
                  noise_image=None, auto_threshold=None, auto_mask=None):
    """The cycle loop of `device_major_cycles`, `mfs.device_mfs_major_cycles`
    and `multiscale.device_ms_major_cycles`. `clean(threshold, probe, mask)`
    returns the minor cycle's info (`probe`: niter=0, the peak under the mask
    with nothing changed), `reinvert()` replaces the residual by the
    re-inverted one, `restore(result)` (or None) adds the restored images. Adds
    `peaks`, `components` and `stop_reason` to `result`.

    With `auto_threshold` or `auto_mask` every cycle starts from the noise
    sigma_c of `noise_image()` (`noise.device_image_noise`): a sigma_c that is
    not finite and > 0 ends the loop ("noise"); `auto_mask` = (seed, grow) grows
    the mask A (zeros at first) by the islands of `noise_image()` above seed
    sigma_c that extend down to grow sigma_c inside `mask`, and A stands in for
    `mask`; max(threshold, auto_threshold sigma_c) stands in for `threshold`.
    `result` then gains `noise` (sigma_c of every cycle begun) and, with
    `auto_mask`, `auto_mask` (the final A). Both options come through
    `_auto_options`."""
    peaks, components, sigmas = [], [], []
    stop_reason = "n_major"
    measure = auto_threshold is not None or auto_mask is not None
    grown = None
    if auto_mask is not None:
        seed_sigmas, grow_sigmas = auto_mask
        image = noise_image()
        grown = torch.zeros(tuple(image.shape), dtype=torch.uint8, device=image.device)
    for _cycle in range(int(n_major)):
        cycle_mask, cycle_floor = mask, threshold
        if measure:
            image = noise_image()
            sigma = device_image_noise(image)["sigma"]
            sigmas.append(sigma)
            if not (math.isfinite(sigma) and sigma > 0.0):
                stop_reason = "noise"
                break
            if grown is not None:
                device_auto_mask(image, seed_sigmas * sigma, grow_sigmas * sigma, region=mask, base=grown, out=grown)
                cycle_mask = grown
            if auto_threshold is not None:
                cycle_floor = max(threshold, auto_threshold * sigma)
        start = clean(cycle_floor, True, cycle_mask)
        if start["stop_reason"] == _lib.CIP_CLEAN_EMPTY:
            stop_reason = "empty"
            break
        peak = abs(start["peak"])
        if peak <= cycle_floor:
            stop_reason = "threshold"
            break
        peaks.append(peak)
        components.append(clean(max(cycle_floor, cycle_fraction * peak), False, cycle_mask)["niter_done"])
        reinvert()
    result.update(peaks=peaks, components=components, stop_reason=stop_reason)
    if measure:
        result["noise"] = sigmas
    if grown is not None:
        result["auto_mask"] = grown
    if restore is not None:
        restore(result)
    return result


def device_hogbom_clean(
    residual: "torch.Tensor",
    psf: "torch.Tensor",
    *,
    gain: float = 0.1,
    threshold: float = 0.0,
    niter: int = 1000,
    mask: Optional["torch.Tensor"] = None,
    model: Optional["torch.Tensor"] = None,
    psf_centre: Optional[tuple] = None,
    inplace: bool = False,
    return_components: bool = False,
    batch: int = 0,
):
    """
    Hogbom CLEAN of the device float64 image `residual` (nx, ny) with `psf`
    (px, py), whose centre pixel is `psf_centre` (default (px // 2, py // 2),
    where `device_ms2dirty(psf=True)` puts the peak). Returns
    (model, residual, info).

    `mask` (nx, ny) uint8 / bool: nonzero where a component may be placed
    (pixels outside it are still subtracted). `model` is accumulated into
    (None: zeros). `inplace=False` works on a clone of `residual`. `info` holds
    `niter_done`, `stop_reason` (CIP_CLEAN_*), `stop` (its name), `peak`
    (signed value of the largest |residual| under the mask on exit) and
    `peak_index` (flat index, -1 when no pixel is allowed); with
    `return_components=True` also `comp_index` (int64) and `comp_flux`
    (float64) of length `niter_done`. `batch`: iterations queued between two
    readbacks of the device state (0: library default); the result does not
    depend on it.
    """
    return _device_clean(residual, psf, None, False, gain=gain, threshold=threshold, niter=niter, mask=mask,
                         model=model, psf_centre=psf_centre, inplace=inplace, return_components=return_components,
                         batch=batch)


def hogbom_clean(
    residual,
    psf,
    *,
    gain: float = 0.1,
    threshold: float = 0.0,
    niter: int = 1000,
    mask=None,
    model=None,
    psf_centre: Optional[tuple] = None,
    return_components: bool = False,
    batch: int = 0,
    device=None,
):
    """
    `device_hogbom_clean` for host or device arrays: numpy in -> numpy out,
    torch in -> torch out (on the GPU). The inputs are never modified. Returns
    (model, residual, info) as `device_hogbom_clean`.
    """
    return _host_clean(device_hogbom_clean, residual, psf, gain=gain, threshold=threshold, niter=niter, mask=mask,
                       model=model, psf_centre=psf_centre, return_components=return_components, batch=batch,
                       device=device)


def device_major_cycles(
    uvw: "torch.Tensor",
    freq: "torch.Tensor",
    vis: "torch.Tensor",
    wgt: Optional["torch.Tensor"],
    npix: int,
    pixsize: float,
    *,
    n_major: int,
    niter: int,
    gain: float = 0.1,
    threshold: float = 0.0,
    cycle_fraction: float = 0.0,
    mask: Optional["torch.Tensor"] = None,
    epsilon: float = EPSILON,
    do_wstacking: bool = DO_WSTACKING,
    support: Optional[int] = None,
    weighting: str = "natural",
    robust: float = 0.0,
    restore: bool = False,
    beam: Optional[dict] = None,
    auto_threshold: Optional[float] = None,
    auto_mask: Optional[tuple] = None,
):
    """
    Major cycles on device-resident data (an `npix` x `npix` image with pixels
    of `pixsize` radians); nothing leaves the GPU but a few scalars per cycle.

    The PSF and the dirty image are normalised inverts (`device_ms2dirty`;
    the second reuses the first's tile plan). Each of up to `n_major` cycles
    CLEANs the residual image down to max(threshold, cycle_fraction * |peak at
    the cycle's start|) with at most `niter` components, accumulating into one
    model; then the residual visibilities `vis - dirty2ms(model)`
    (`device_residual`, unweighted: the invert applies `wgt`) are re-inverted,
    both through the same tile plan. The residual CLEAN leaves behind is
    discarded in favour of the re-inverted one. The loop ends early once a
    cycle starts at or below `threshold`.

    `weighting` ("natural", "uniform" or "briggs" with `robust`): the imaging
    weights (`device_imaging_weights`) are formed once from `wgt` and used for
    the PSF and every invert of the loop; the predict stays unweighted.
    "natural" uses `wgt` as it is.

    Returns a dict: `model`, `residual` (image), `psf`, `peaks` (|peak| at the
    start of each cycle run), `components` (count per cycle) and `stop_reason`
    ("threshold": a cycle started at or below it; "n_major": the cycles ran
    out; "empty": the mask allows no pixel).

    `restore=True` adds `beam` (the clean beam, `restore.device_fit_beam` of
    the loop's PSF unless `beam` is passed) and `restored` (the final model
    convolved with it plus the final residual, `restore.device_restore`).

    `auto_threshold` (a number of sigmas) and `auto_mask` ((seed_sigmas,
    grow_sigmas), or one number for both) drive the loop by the noise of the
    residual image, measured on the device at the start of every cycle
    (`noise.device_image_noise`; sigma_c = 1.4826 MAD): the cycle's threshold
    is max(threshold, auto_threshold sigma_c) wherever `threshold` stands
    above, and components go only into the mask A, which starts empty and
    every cycle gains the islands of the residual above seed_sigmas sigma_c
    that extend down to grow_sigmas sigma_c (`noise.device_auto_mask`, inside
    `mask` when one is given). A sigma_c that is not finite and > 0 ends the
    loop with `stop_reason` "noise". The result then also holds `noise` (the
    sigma_c of every cycle begun, the stopping one included) and, with
    `auto_mask`, `auto_mask` (the final A). With both None (the default)
    nothing is measured and neither key exists.
    """
    require_gpu()
    auto_threshold, auto_mask = _auto_options(auto_threshold, auto_mask)
    npix = int(npix)
    kw = dict(epsilon=epsilon, support=support, do_wstacking=do_wstacking)
    wgt, _ = device_imaging_weights(uvw, freq, wgt, npix, npix, pixsize, pixsize, weighting=weighting, robust=robust)
    psf, _ = device_ms2dirty(uvw, freq, None, wgt, npix, npix, pixsize, pixsize, psf=True, normalise=True, **kw)
    residual, _ = device_ms2dirty(uvw, freq, vis, wgt, npix, npix, pixsize, pixsize, normalise=True,
                                  reuse_plan=True, **kw)
    model = torch.zeros((npix, npix), dtype=torch.float64, device=uvw.device)

    def clean(cycle_threshold, probe, cycle_mask):
        return device_hogbom_clean(residual, psf, gain=gain, threshold=cycle_threshold, niter=0 if probe else niter,
                                   mask=cycle_mask, model=None if probe else model, inplace=True)[2]

    def reinvert():
        vis_res = device_residual(uvw, freq, vis, model, pixsize, None, reuse_plan=True, **kw)
        device_ms2dirty(uvw, freq, vis_res, wgt, npix, npix, pixsize, pixsize, normalise=True, reuse_plan=True,
                        out=residual, **kw)

    def add_restored(result):
        result["beam"] = device_fit_beam(psf) if beam is None else dict(beam)
        result["restored"] = device_restore(model, residual, result["beam"])

    return _major_cycles({"model": model, "residual": residual, "psf": psf}, n_major, threshold, cycle_fraction,
                         clean, reinvert, add_restored if restore else None, mask=mask,
                         noise_image=lambda: residual, auto_threshold=auto_threshold, auto_mask=auto_mask)
