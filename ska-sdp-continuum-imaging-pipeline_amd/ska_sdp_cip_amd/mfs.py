"""
Multi-term multi-frequency synthesis (MT-MFS, Rau & Cornwell 2011, point
sources only) on the GPU: Taylor-term inverts, the joint minor cycle
(`cip_mfs_clean`) and the major-cycle loop that gives an intensity image at a
reference frequency and a spectral-index image.

The sky is modelled per pixel as sum_t I_t x^t with x = (nu - nu_ref) / nu_ref
and T = `nterms` terms. Residual term t is the normalised invert of the
visibilities times x^t, PSF k (k < 2T - 1) that of the real visibilities x^k,
and H[t][q] = psfs[t + q][centre] couples the terms; the minor cycle picks the
pixel with the largest principal solution (H^-1 r)_0 and subtracts all T
components from all T residuals at once. The operator is defined exactly,
rounding included, in include/cip_mfs.h.
"""

from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib
from ._call import check_array, check_rows, require_gpu
from .deconvolve import _auto_options, _device_clean, _host_clean, _major_cycles
from .gridder import device_dirty2ms, device_ms2dirty
from .invert import DO_WSTACKING, EPSILON
from .restore import device_fit_beam, device_restore
from .weighting import device_imaging_weights

try:
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None


def _check_nterms(nterms) -> int:
    nterms = int(nterms)
    if not 1 <= nterms <= _lib.MFS_MAX_TERMS:
        raise ValueError(f"nterms must be 1 .. {_lib.MFS_MAX_TERMS}, got {nterms}")
    return nterms


def _is_tensor(x) -> bool:
    return torch is not None and torch.is_tensor(x)


def _mid_band(freq) -> float:
    return 0.5 * (float(freq.min()) + float(freq.max()))


# ------------------------------------------------------------- host only ----
def taylor_basis(freq, ref_freq: float, nterms: int):
    """(nterms, nchan) float64: x_c^t with x_c = (freq_c - ref_freq) / ref_freq
    (row 0 is all ones). numpy in -> numpy out, torch in -> torch out (same device)."""
    nterms = _check_nterms(nterms)
    ref = float(ref_freq)
    if not (np.isfinite(ref) and ref > 0.0):
        raise ValueError("ref_freq must be finite and > 0")
    if _is_tensor(freq):
        x = (freq.to(torch.float64) - ref) / ref
        return torch.stack([x ** t for t in range(nterms)])
    x = (np.asarray(freq, dtype=np.float64) - ref) / ref
    return np.stack([x ** t for t in range(nterms)])


def mfs_hessian(psfs, centre: Optional[tuple] = None):
    """(H, hinv), float64 numpy (T, T), of the PSF stack `psfs` (2T - 1, px, py):
    H[t][q] = psfs[t + q][centre] (default centre (px // 2, py // 2)) and
    hinv = np.linalg.inv(H). ValueError when H is not finite or its condition
    number exceeds 1e12 (for instance a single channel, where every x is 0)."""
    if len(psfs.shape) != 3 or psfs.shape[0] % 2 == 0 or psfs.shape[0] > 2 * _lib.MFS_MAX_TERMS - 1:
        raise ValueError(f"psfs must be (2 nterms - 1, px, py) with nterms 1 .. {_lib.MFS_MAX_TERMS}, "
                         f"got {tuple(psfs.shape)}")
    nterms = (int(psfs.shape[0]) + 1) // 2
    cx, cy = (int(psfs.shape[1]) // 2, int(psfs.shape[2]) // 2) if centre is None else (int(centre[0]), int(centre[1]))
    if not (0 <= cx < psfs.shape[1] and 0 <= cy < psfs.shape[2]):
        raise ValueError("centre must lie inside the PSF")
    peaks = psfs[:, cx, cy]
    peaks = peaks.detach().cpu().numpy() if _is_tensor(peaks) else np.asarray(peaks)
    peaks = peaks.astype(np.float64)
    hessian = np.array([[peaks[t + q] for q in range(nterms)] for t in range(nterms)], dtype=np.float64)
    if not np.isfinite(hessian).all():
        raise ValueError("mfs_hessian: the PSF centre values are not finite")
    cond = float(np.linalg.cond(hessian))
    if not cond <= 1e12:
        raise ValueError(f"mfs_hessian: H is singular or ill-conditioned (condition number {cond:.3g} > 1e12); "
                         "use fewer terms or a wider band")
    return hessian, np.linalg.inv(hessian)


# ---------------------------------------------------------------- device ----
def device_mfs_clean(
    residuals: "torch.Tensor",
    psfs: "torch.Tensor",
    hinv,
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
    The joint minor cycle (`cip_mfs_clean`) on the device float64 stacks
    `residuals` (T, nx, ny) and `psfs` (2T - 1, px, py), every PSF with its
    centre at `psf_centre` (default (px // 2, py // 2)); `hinv` (T, T) is the
    host matrix `mfs_hessian` returns. Returns (model, residuals, info) in the
    shape of `deconvolve.device_hogbom_clean`: `model` is (T, nx, ny), `mask`
    (nx, ny) holds for all terms, `info["peak"]` is the signed principal
    solution (hinv r)_0 at its largest allowed magnitude, and with
    `return_components=True` `comp_index` is (niter_done,) and `comp_flux`
    (niter_done, T). T = 1 with hinv = [[1.0]] is `device_hogbom_clean` to
    the bit.
    """
    return _device_clean(residuals, psfs, hinv, True, gain=gain, threshold=threshold, niter=niter, mask=mask,
                         model=model, psf_centre=psf_centre, inplace=inplace, return_components=return_components,
                         batch=batch)


def mfs_clean(
    residuals,
    psfs,
    hinv,
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
    `device_mfs_clean` for host or device arrays: numpy in -> numpy out, torch
    in -> torch out (on the GPU). The inputs are never modified. Returns
    (model, residuals, info) as `device_mfs_clean`.
    """
    return _host_clean(device_mfs_clean, residuals, psfs, hinv, gain=gain, threshold=threshold, niter=niter, mask=mask,
                       model=model, psf_centre=psf_centre, return_components=return_components, batch=batch,
                       device=device)


def device_mfs_invert(
    uvw: "torch.Tensor",
    freq: "torch.Tensor",
    vis: "torch.Tensor",
    wgt: Optional["torch.Tensor"],
    npix: int,
    pixsize: float,
    *,
    nterms: int,
    ref_freq: Optional[float] = None,
    epsilon: float = EPSILON,
    do_wstacking: bool = DO_WSTACKING,
    support: Optional[int] = None,
    want_psfs: bool = True,
    reuse_plan: bool = False,
    out: Optional["torch.Tensor"] = None,
    scratch: Optional["torch.Tensor"] = None,
):
    """
    The Taylor-term images of device-resident visibilities: (residuals, psfs)
    with residuals (nterms, npix, npix), term t the normalised invert
    (`device_ms2dirty`, divided by the sum of `wgt`) of vis x^t, and psfs
    (2 nterms - 1, npix, npix), PSF k the normalised invert of the real
    visibilities x^k. The Taylor factor goes into the visibilities; the
    weights stay as they are (non-negative, the same sum for every image).

    `ref_freq=None`: the middle of the band. The first invert plans (unless
    `reuse_plan=True` promises a matching plan from this thread's previous
    call) and every other runs through its tile plan. `want_psfs=False`
    returns (residuals, None). `out` (nterms, npix, npix) receives the
    residuals; `scratch` (nrow, nchan, the dtype of `vis`) is the one
    visibility buffer the scaled columns are formed in (None: allocated).
    """
    require_gpu()
    nterms, npix = _check_nterms(nterms), int(npix)
    nrow, nchan = check_rows(uvw, freq, "device_mfs_invert inputs")
    dev = uvw.device
    check_array(vis, (torch.complex64, torch.complex128), (nrow, nchan), dev, "vis")
    ref = _mid_band(freq) if ref_freq is None else float(ref_freq)
    real = torch.float32 if vis.dtype == torch.complex64 else torch.float64
    basis = taylor_basis(freq, ref, 2 * nterms - 1).to(real)  # (2T - 1, nchan)
    if scratch is None:
        scratch = torch.empty_like(vis)
    else:
        check_array(scratch, (vis.dtype,), (nrow, nchan), dev, "scratch")
    if out is None:
        out = torch.empty((nterms, npix, npix), dtype=torch.float64, device=dev)
    else:
        check_array(out, (torch.float64,), (nterms, npix, npix), dev, "out")
    kw = dict(epsilon=epsilon, support=support, do_wstacking=do_wstacking, normalise=True)
    psfs = None
    if want_psfs:
        psfs = torch.empty((2 * nterms - 1, npix, npix), dtype=torch.float64, device=dev)
        for k in range(2 * nterms - 1):
            scratch.copy_(basis[k].expand(nrow, nchan))
            device_ms2dirty(uvw, freq, scratch, wgt, npix, npix, pixsize, pixsize, out=psfs[k],
                            reuse_plan=reuse_plan or k > 0, **kw)
    for t in range(nterms):
        src = vis
        if t > 0:
            torch.mul(vis, basis[t], out=scratch)
            src = scratch
        device_ms2dirty(uvw, freq, src, wgt, npix, npix, pixsize, pixsize, out=out[t],
                        reuse_plan=reuse_plan or want_psfs or t > 0, **kw)
    return out, psfs


def device_mfs_residual(
    uvw: "torch.Tensor",
    freq: "torch.Tensor",
    vis: "torch.Tensor",
    models: "torch.Tensor",
    pixsize: float,
    ref_freq: float,
    *,
    epsilon: float = EPSILON,
    do_wstacking: bool = DO_WSTACKING,
    support: Optional[int] = None,
    inplace: bool = False,
    reuse_plan: bool = False,
    scratch: Optional["torch.Tensor"] = None,
):
    """
    The wide-band major cycle's residual vis - sum_t x^t dirty2ms(models[t])
    on device-resident tensors (`models` (T, npix, npix) float64, pixels of
    `pixsize` radians, unweighted as `predict.device_residual`). Each term is
    degridded into the scratch column (`scratch`, complex128 (nrow, nchan);
    None: allocated) and combined with its Taylor factor in torch. Returns a
    new tensor, or `vis` itself updated in place with `inplace=True`.
    `reuse_plan`: as `device_dirty2ms`; the terms after the first always run
    through the first's plan.
    """
    require_gpu()
    nrow, nchan = check_rows(uvw, freq, "device_mfs_residual inputs")
    dev = uvw.device
    check_array(vis, (torch.complex64, torch.complex128), (nrow, nchan), dev, "vis")
    if models.dim() != 3:
        raise ValueError(f"models must be a float64 (nterms, npix_x, npix_y) stack, got {tuple(models.shape)}")
    nterms = _check_nterms(models.shape[0])
    check_array(models, (torch.float64,), None, dev, "models")
    basis = taylor_basis(freq, float(ref_freq), nterms)
    if scratch is None:
        scratch = torch.empty((nrow, nchan), dtype=torch.complex128, device=dev)
    else:
        check_array(scratch, (torch.complex128,), (nrow, nchan), dev, "scratch")
    out = vis if inplace else vis.clone()
    for t in range(nterms):
        device_dirty2ms(uvw, freq, models[t], None, pixsize, pixsize, epsilon=epsilon, support=support,
                        do_wstacking=do_wstacking, out=scratch, reuse_plan=reuse_plan or t > 0)
        if t > 0:
            scratch.mul_(basis[t])
        out.sub_(scratch)
    return out


def device_mfs_major_cycles(
    uvw: "torch.Tensor",
    freq: "torch.Tensor",
    vis: "torch.Tensor",
    wgt: Optional["torch.Tensor"],
    npix: int,
    pixsize: float,
    *,
    nterms: int = 2,
    ref_freq: Optional[float] = None,
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
    alpha_cut: float = 0.0,
    auto_threshold: Optional[float] = None,
    auto_mask: Optional[tuple] = None,
):
    """
    Wide-band major cycles on device-resident data: the structure of
    `deconvolve.device_major_cycles` with `device_mfs_invert`,
    `device_mfs_clean` and `device_mfs_residual` in place of the invert, the
    Hogbom minor cycle and the residual. Peaks and `threshold` refer to the
    principal solution (hinv r)_0, the intensity at `ref_freq` (None: the
    middle of the band); a cycle starts from `niter=0` of `device_mfs_clean`.
    With `nterms=1` the matrix is the identity: the PSF's centre value is not
    divided out, and the loop computes what `device_major_cycles` computes.

    Returns a dict: `models` (T, npix, npix; term 0 is the intensity at
    `ref_freq`, term 1 intensity times spectral index for a power law),
    `residuals` (T, npix, npix), `psfs` (2T - 1, npix, npix), `hessian`,
    `hinv` (numpy (T, T)), `ref_freq`, `peaks`, `components` and `stop_reason`
    as `device_major_cycles`.

    `restore=True` adds `beam` (`restore.device_fit_beam` of psfs[0] unless
    `beam` is passed), `restored` (T, npix, npix), term t being
    `device_restore(models[t], sum_q hinv[t][q] residuals[q], beam)`, and, for
    nterms >= 2, `alpha` = restored[1] / restored[0] where |restored[0]| >
    `alpha_cut`, NaN elsewhere.

    `auto_threshold` and `auto_mask` as for `device_major_cycles`; the noise
    and the islands are those of the term-0 residual, residuals[0].
    """
    require_gpu()
    auto_threshold, auto_mask = _auto_options(auto_threshold, auto_mask)
    nterms, npix = _check_nterms(nterms), int(npix)
    ref = _mid_band(freq) if ref_freq is None else float(ref_freq)
    kw = dict(epsilon=epsilon, support=support, do_wstacking=do_wstacking)
    wgt, _ = device_imaging_weights(uvw, freq, wgt, npix, npix, pixsize, pixsize, weighting=weighting, robust=robust)
    scratch = torch.empty_like(vis)
    residuals, psfs = device_mfs_invert(uvw, freq, vis, wgt, npix, pixsize, nterms=nterms, ref_freq=ref,
                                        scratch=scratch, **kw)
    hessian, hinv = mfs_hessian(psfs)
    if nterms == 1:  # nothing to decouple: the narrow-band loop, which leaves the PSF's centre value in
        hinv = np.ones((1, 1))
    models = torch.zeros_like(residuals)
    degrid = scratch if scratch.dtype == torch.complex128 else None

    def clean(cycle_threshold, probe, cycle_mask):
        return device_mfs_clean(residuals, psfs, hinv, gain=gain, threshold=cycle_threshold,
                                niter=0 if probe else niter, mask=cycle_mask, model=None if probe else models,
                                inplace=True)[2]

    def reinvert():
        vis_res = device_mfs_residual(uvw, freq, vis, models, pixsize, ref, reuse_plan=True, scratch=degrid, **kw)
        device_mfs_invert(uvw, freq, vis_res, wgt, npix, pixsize, nterms=nterms, ref_freq=ref, want_psfs=False,
                          reuse_plan=True, out=residuals, scratch=scratch, **kw)

    def add_restored(result):
        result["beam"] = device_fit_beam(psfs[0]) if beam is None else dict(beam)
        solved = torch.einsum("tq,qij->tij", torch.from_numpy(hinv).to(residuals.device), residuals)
        result["restored"] = torch.stack([device_restore(models[t], solved[t].contiguous(), result["beam"])
                                          for t in range(nterms)])
        if nterms >= 2:
            i0 = result["restored"][0]
            result["alpha"] = torch.where(i0.abs() > alpha_cut, result["restored"][1] / i0,
                                          torch.full_like(i0, float("nan")))

    result = {"models": models, "residuals": residuals, "psfs": psfs, "hessian": hessian, "hinv": hinv,
              "ref_freq": ref}
    return _major_cycles(result, n_major, threshold, cycle_fraction, clean, reinvert, add_restored if restore else None,
                         mask=mask, noise_image=lambda: residuals[0], auto_threshold=auto_threshold,
                         auto_mask=auto_mask)
