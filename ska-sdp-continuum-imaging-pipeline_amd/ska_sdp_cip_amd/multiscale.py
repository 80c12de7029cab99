"""
Multiscale CLEAN (Cornwell 2008) on the GPU with circular Gaussian scale
kernels: the separable scale convolution (`cip_ms_convolve`), the minor cycle
over S scale-smoothed residuals (`cip_ms_clean`) and the major-cycle loop
around them.

The sky is modelled as sum_s scale_s (*) model_s, where scale_s is a unit-sum
Gaussian of FWHM `widths[s]` pixels (width 0: a pixel) and model_s a delta
model. Residual plane s is the residual smoothed with scale s, cross PSF
(s, q) the PSF smoothed with scales s and q; the minor cycle picks the (scale,
pixel) pair with the largest weighted residual and subtracts the matching
cross PSF from every plane. The operators are defined exactly, rounding
included, in include/cip_ms.h.
"""

from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib
from ._call import STREAM, call, check_array, require_gpu
from .deconvolve import _auto_options, _device_clean, _host_clean, _major_cycles
from .gridder import device_ms2dirty
from .invert import DO_WSTACKING, EPSILON
from .predict import device_residual
from .restore import _status, device_fit_beam, device_restore
from .weighting import device_imaging_weights

try:
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None

_PF64 = ctypes.POINTER(ctypes.c_double)


def _check_widths(widths) -> list:
    """`widths` as a list of floats: ascending, each 0 or >= 1, at most 6."""
    try:
        out = [float(w) for w in widths]
    except TypeError as exc:
        raise ValueError("widths must be a sequence of scale FWHMs in pixels") from exc
    if not 1 <= len(out) <= _lib.MS_MAX_SCALES:
        raise ValueError(f"widths must hold 1 .. {_lib.MS_MAX_SCALES} scales, got {len(out)}")
    if any(not (np.isfinite(w) and (w == 0.0 or w >= 1.0)) for w in out):
        raise ValueError(f"widths must each be 0 or a finite value >= 1 (FWHM in pixels), got {out}")
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"widths must ascend, got {out}")
    return out


def tri(s: int, q: int, nscales: int) -> int:
    """The plane of the packed cross-PSF stack that holds the pair (s, q), s <= q."""
    return s * nscales - s * (s - 1) // 2 + (q - s)


# ------------------------------------------------------------- host only ----
def scale_radius(width: float, tol: float = 1e-8) -> int:
    """The least radius at which the scale of FWHM `width` pixels has fallen to
    `tol` (`cip_ms_scale_radius`; 0 for width 0). Host-only."""
    return _status(_lib.lib().cip_ms_scale_radius(float(width), float(tol)))


def scale_taps(width: float, radius: Optional[int] = None, *, tol: float = 1e-8) -> np.ndarray:
    """The 2 R + 1 float64 taps of the scale of FWHM `width` pixels
    (`cip_ms_scale_taps`): a Gaussian normalised to unit sum, [1.0] for width
    0. `radius` None: `scale_radius(width, tol)`. Host-only."""
    r = scale_radius(width, tol) if radius is None else int(radius)
    taps = np.empty(2 * max(r, 0) + 1, dtype=np.float64)
    _lib.check(_lib.lib().cip_ms_scale_taps(float(width), r, taps.ctypes.data_as(_PF64)))
    return taps


def scale_weights(cross_psfs, widths, scale_bias: float = 0.6, centre: Optional[tuple] = None):
    """(select_weight, flux_scale), float64 numpy (S,), of the packed cross-PSF
    stack `cross_psfs` (S (S + 1) / 2, px, py): flux_scale[s] = 1 / P_ss[centre]
    (default centre (px // 2, py // 2)), which turns a smoothed residual's peak
    into the flux of a scale-s component, and select_weight[s] =
    (1 - scale_bias width_s / width_max) flux_scale[s], the small-scale bias of
    Cornwell (2008) (the bias is 1 when width_max is 0). ValueError when a
    centre value is not finite or not > 0."""
    widths = _check_widths(widths)
    nscales = len(widths)
    if len(cross_psfs.shape) != 3 or int(cross_psfs.shape[0]) != nscales * (nscales + 1) // 2:
        raise ValueError(f"cross_psfs must be ({nscales * (nscales + 1) // 2}, px, py) for {nscales} scales, got "
                         f"{tuple(cross_psfs.shape)}")
    px, py = int(cross_psfs.shape[1]), int(cross_psfs.shape[2])
    cx, cy = (px // 2, py // 2) if centre is None else (int(centre[0]), int(centre[1]))
    if not (0 <= cx < px and 0 <= cy < py):
        raise ValueError("centre must lie inside the PSF")
    peaks = cross_psfs[:, cx, cy]
    peaks = peaks.detach().cpu().numpy() if torch is not None and torch.is_tensor(peaks) else np.asarray(peaks)
    diag = np.array([peaks[tri(s, s, nscales)] for s in range(nscales)], dtype=np.float64)
    if not (np.isfinite(diag).all() and (diag > 0.0).all()):
        raise ValueError(f"scale_weights: the cross PSFs' centre values must be finite and > 0, got {diag.tolist()}")
    flux_scale = 1.0 / diag
    wmax = widths[-1]
    bias = np.array([1.0 if wmax == 0.0 else 1.0 - float(scale_bias) * w / wmax for w in widths], dtype=np.float64)
    return bias * flux_scale, flux_scale


# ---------------------------------------------------------------- device ----
def _check_image(img, shape, dev, name):
    if img.dim() != 2:
        raise ValueError(f"{name} must be a float64 2-D image, got {img.dtype} {tuple(img.shape)}")
    check_array(img, (torch.float64,), shape, dev, name)


def device_ms_convolve(image: "torch.Tensor", width: float, *, tol: float = 1e-8,
                       out: Optional["torch.Tensor"] = None, taps=None):
    """
    The device float64 `image` (nx, ny) smoothed with the scale of FWHM `width`
    pixels (`cip_ms_convolve`: two 1-D passes with `scale_taps(width, tol=tol)`,
    terms outside the image skipped), queued on the current stream. Width 0
    returns a copy. `out` receives the result (it may be `image`). `taps`: a
    host table of 2 R + 1 values to use instead of the scale's (`width` is then
    not consulted).
    """
    require_gpu()
    dev, shape = image.device, tuple(image.shape)
    _check_image(image, None, dev, "image")
    if out is not None:
        _check_image(out, shape, dev, "out")
    if out is None:
        out = torch.empty_like(image)
    if taps is None:
        if float(width) == 0.0:  # the identity: a copy keeps every bit (the passes would turn -0.0 into +0.0)
            if out.data_ptr() != image.data_ptr():
                out.copy_(image)
            return out
        taps = scale_taps(width, tol=tol)
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    if taps.ndim != 1 or taps.size % 2 == 0:
        raise ValueError(f"taps must be a 1-D table of 2 R + 1 values, got shape {taps.shape}")
    call(dev, "cip_ms_convolve", image, shape[0], shape[1], taps.ctypes.data_as(_PF64), taps.size // 2, STREAM, out)
    return out


def device_scale_residuals(residual: "torch.Tensor", widths, *, tol: float = 1e-8,
                           out: Optional["torch.Tensor"] = None):
    """(S, nx, ny): the device image `residual` smoothed with every scale of `widths`."""
    widths = _check_widths(widths)
    require_gpu()
    _check_image(residual, None, residual.device, "residual")
    if out is None:
        out = torch.empty((len(widths), *residual.shape), dtype=torch.float64, device=residual.device)
    else:
        check_array(out, (torch.float64,), (len(widths), *residual.shape), residual.device, "out")
    for s, w in enumerate(widths):
        device_ms_convolve(residual, w, tol=tol, out=out[s])
    return out


def device_cross_psfs(psf: "torch.Tensor", widths, *, tol: float = 1e-8):
    """The packed cross-PSF stack (S (S + 1) / 2, px, py) of the device image
    `psf`: plane `tri(s, q, S)`, s <= q, is `psf` smoothed with scale s first,
    then with scale q."""
    widths = _check_widths(widths)
    require_gpu()
    _check_image(psf, None, psf.device, "psf")
    nscales = len(widths)
    out = torch.empty((nscales * (nscales + 1) // 2, *psf.shape), dtype=torch.float64, device=psf.device)
    for s in range(nscales):
        once = device_ms_convolve(psf, widths[s], tol=tol)
        for q in range(s, nscales):
            device_ms_convolve(once, widths[q], tol=tol, out=out[tri(s, q, nscales)])
    return out


def device_ms_clean(
    residuals: "torch.Tensor",
    cross_psfs: "torch.Tensor",
    select_weight,
    flux_scale,
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
    The multiscale minor cycle (`cip_ms_clean`) on the device float64 stacks
    `residuals` (S, nx, ny) and `cross_psfs` (S (S + 1) / 2, px, py), every PSF
    with its centre at `psf_centre` (default (px // 2, py // 2));
    `select_weight` and `flux_scale` (S,) are the host arrays `scale_weights`
    returns. Returns (model, residuals, info) in the shape of
    `deconvolve.device_hogbom_clean`: `model` is (S, nx, ny), one delta model
    per scale, `mask` (nx, ny) holds for all scales, `info["peak"]` is the
    signed select_weight[s] r_s of the largest allowed magnitude,
    `info["peak_scale"]` its scale, and with `return_components=True`
    `comp_index`, `comp_scale` and `comp_flux` are (niter_done,). S = 1 with
    both arrays [1.0] is `device_hogbom_clean` to the bit.
    """
    return _device_clean(residuals, cross_psfs, (select_weight, flux_scale), "ms", gain=gain, threshold=threshold,
                         niter=niter, mask=mask, model=model, psf_centre=psf_centre, inplace=inplace,
                         return_components=return_components, batch=batch)


def ms_clean(
    residuals,
    cross_psfs,
    select_weight,
    flux_scale,
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
    `device_ms_clean` for host or device arrays: numpy in -> numpy out, torch
    in -> torch out (on the GPU). The inputs are never modified. Returns
    (model, residuals, info) as `device_ms_clean`.
    """
    return _host_clean(device_ms_clean, residuals, cross_psfs, select_weight, flux_scale, gain=gain,
                       threshold=threshold, niter=niter, mask=mask, model=model, psf_centre=psf_centre,
                       return_components=return_components, batch=batch, device=device)


def device_ms_model(models: "torch.Tensor", widths, *, tol: float = 1e-8, out: Optional["torch.Tensor"] = None):
    """The model image sum_s scale_s (*) models[s] of the per-scale delta
    models (S, nx, ny), added in ascending s with plain float64 adds."""
    widths = _check_widths(widths)
    require_gpu()
    if models.dim() != 3 or int(models.shape[0]) != len(widths):
        raise ValueError(f"models must be a float64 ({len(widths)}, nx, ny) stack, got {tuple(models.shape)}")
    check_array(models, (torch.float64,), None, models.device, "models")
    total = device_ms_convolve(models[0], widths[0], tol=tol, out=out)
    for s in range(1, len(widths)):
        total.add_(device_ms_convolve(models[s], widths[s], tol=tol))
    return total


def device_ms_major_cycles(
    uvw: "torch.Tensor",
    freq: "torch.Tensor",
    vis: "torch.Tensor",
    wgt: Optional["torch.Tensor"],
    npix: int,
    pixsize: float,
    *,
    widths,
    scale_bias: float = 0.6,
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
    Multiscale major cycles on device-resident data: the structure of
    `deconvolve.device_major_cycles` with the multiscale minor cycle in place
    of Hogbom's. The PSF, its cross PSFs (`device_cross_psfs`) and the weights
    (`scale_weights` with `scale_bias`) are computed once. Each cycle smooths
    the residual with every scale (`device_scale_residuals`), CLEANs the stack
    down to the cycle threshold (`device_ms_clean`; peaks and `threshold` refer
    to select_weight[s] r_s), forms the model image (`device_ms_model`) and
    re-inverts the residual visibilities (`device_residual`) through the first
    invert's tile plan. With `widths=[0]` both weights are 1 (the PSF's centre
    value is not divided out) and the loop computes what `device_major_cycles`
    computes.

    Returns a dict: `model` (the summed model image), `models` (S, npix, npix),
    `residual` (image), `psf`, `cross_psfs`, `select_weight`, `flux_scale`,
    `widths`, `peaks`, `components` and `stop_reason` as `device_major_cycles`.

    `restore=True` adds `beam` (`restore.device_fit_beam` of the PSF unless
    `beam` is passed) and `restored` (`device_restore` of the summed model and
    the final residual).

    `auto_threshold` and `auto_mask` as for `device_major_cycles`; the noise
    and the islands are those of the unsmoothed residual image, and the one
    mask holds for every scale.
    """
    require_gpu()
    auto_threshold, auto_mask = _auto_options(auto_threshold, auto_mask)
    widths, npix = _check_widths(widths), int(npix)
    nscales = len(widths)
    kw = dict(epsilon=epsilon, support=support, do_wstacking=do_wstacking)
    wgt, _ = device_imaging_weights(uvw, freq, wgt, npix, npix, pixsize, pixsize, weighting=weighting, robust=robust)
    psf, _ = device_ms2dirty(uvw, freq, None, wgt, npix, npix, pixsize, pixsize, psf=True, normalise=True, **kw)
    residual, _ = device_ms2dirty(uvw, freq, vis, wgt, npix, npix, pixsize, pixsize, normalise=True,
                                  reuse_plan=True, **kw)
    cross_psfs = device_cross_psfs(psf, widths)
    if widths == [0.0]:  # nothing to weigh: the Hogbom loop, which leaves the PSF's centre value in
        select_weight = flux_scale = np.ones(1)
    else:
        select_weight, flux_scale = scale_weights(cross_psfs, widths, scale_bias)
    models = torch.zeros((nscales, npix, npix), dtype=torch.float64, device=uvw.device)
    model = torch.zeros((npix, npix), dtype=torch.float64, device=uvw.device)
    residuals = torch.empty_like(models)
    smoothed = False  # whether `residuals` holds the scales of the current `residual`

    def clean(cycle_threshold, probe, cycle_mask):
        nonlocal smoothed
        if not smoothed:  # once per cycle: the probe changes nothing, so the CLEAN after it starts from the same stack
            device_scale_residuals(residual, widths, out=residuals)
            smoothed = True
        return device_ms_clean(residuals, cross_psfs, select_weight, flux_scale, gain=gain, threshold=cycle_threshold,
                               niter=0 if probe else niter, mask=cycle_mask, model=None if probe else models,
                               inplace=True)[2]

    def reinvert():
        nonlocal smoothed
        device_ms_model(models, widths, out=model)
        vis_res = device_residual(uvw, freq, vis, model, pixsize, None, reuse_plan=True, **kw)
        device_ms2dirty(uvw, freq, vis_res, wgt, npix, npix, pixsize, pixsize, normalise=True, reuse_plan=True,
                        out=residual, **kw)
        smoothed = False

    def add_restored(result):
        result["beam"] = device_fit_beam(psf) if beam is None else dict(beam)
        result["restored"] = device_restore(model, residual, result["beam"])

    result = {"model": model, "models": models, "residual": residual, "psf": psf, "cross_psfs": cross_psfs,
              "select_weight": select_weight, "flux_scale": flux_scale, "widths": widths}
    return _major_cycles(result, n_major, threshold, cycle_fraction, clean, reinvert, add_restored if restore else None,
                         mask=mask, noise_image=lambda: residual, auto_threshold=auto_threshold, auto_mask=auto_mask)
