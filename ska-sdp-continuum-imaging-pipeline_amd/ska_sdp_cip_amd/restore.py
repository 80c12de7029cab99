"""
The restoring step: the clean beam fitted to the PSF's main lobe
(`cip_beam_fit`) and the restored image, the model convolved with that beam
plus the residual (`cip_restore`), on the GPU.

The operators are defined exactly in include/cip_restore.h. A beam is a plain
dict with `a`, `b`, `c` (the form of exp(-(a da^2 + 2 b da db + c db^2)) in
pixels, da along axis 0), `fwhm_major`, `fwhm_minor` (pixels), `pa` (radians)
and `n_fit`. The restore adds, per output pixel, the model's non-zero pixels
within `radius` in ascending flat index, product and add each rounded: it is
bit-identical to the numpy loop over `np.flatnonzero(model)` with the table
`beam_taps` returns.
"""

from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np

from . import _lib
from ._call import STREAM, call, check_array, require_gpu, target_device, to_device

try:
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None

_PF64 = ctypes.POINTER(ctypes.c_double)


def _as_struct(beam) -> "_lib.Beam":
    """`beam` (a dict with at least a, b, c, or a `_lib.Beam`) as the C struct."""
    if isinstance(beam, _lib.Beam):
        return beam
    try:
        out = _lib.Beam(a=float(beam["a"]), b=float(beam["b"]), c=float(beam["c"]))
    except (KeyError, TypeError) as exc:
        raise ValueError("beam must be a dict with a, b and c (beam_from_fwhm, device_fit_beam)") from exc
    for name in ("fwhm_major", "fwhm_minor", "pa"):
        setattr(out, name, float(beam.get(name, math.nan)))
    out.n_fit = int(beam.get("n_fit", 0))
    return out


def _status(rc: int) -> int:
    """A non-negative result of the library, or the exception of its code."""
    if rc < 0:
        _lib.check(rc)
    return rc


# ------------------------------------------------------------- host only ----
def beam_from_fwhm(major: float, minor: float, pa: float = 0.0) -> dict:
    """The beam with FWHMs `major` >= `minor` > 0 (pixels) and position angle
    `pa` (radians, from +axis 1 towards +axis 0). Host-only."""
    out = _lib.Beam()
    _lib.check(_lib.lib().cip_beam_from_fwhm(float(major), float(minor), float(pa), ctypes.byref(out)))
    return out.as_dict()


def beam_fit_window(window, *, cut: float = _lib.BEAM_FIT_CUT) -> dict:
    """The fit of `cip_beam_fit_window` on a host (2 r + 1, 2 r + 1) window
    whose centre is the PSF's centre pixel (NaN: outside the PSF). Host-only."""
    win = np.ascontiguousarray(window, dtype=np.float64)
    if win.ndim != 2 or win.shape[0] != win.shape[1] or win.shape[0] % 2 == 0:
        raise ValueError(f"window must be (2 r + 1, 2 r + 1), got {win.shape}")
    out = _lib.Beam()
    _lib.check(_lib.lib().cip_beam_fit_window(win.ctypes.data_as(_PF64), win.shape[0] // 2, float(cut),
                                              ctypes.byref(out)))
    return out.as_dict()


def beam_radius(beam, tol: float = 1e-8) -> int:
    """The least radius at which the beam has fallen to `tol` along its major
    axis (`cip_beam_radius`). Host-only."""
    return _status(_lib.lib().cip_beam_radius(ctypes.byref(_as_struct(beam)), float(tol)))


def beam_taps(beam, radius: Optional[int] = None) -> np.ndarray:
    """The (2 R + 1, 2 R + 1) float64 table `cip_restore` uploads for `beam`
    and `radius` (None: `beam_radius(beam, 1e-8)`). Host-only."""
    b = _as_struct(beam)
    r = beam_radius(b) if radius is None else int(radius)
    taps = np.empty((2 * max(r, 0) + 1,) * 2, dtype=np.float64)
    _lib.check(_lib.lib().cip_beam_taps(ctypes.byref(b), r, taps.ctypes.data_as(_PF64)))
    return taps


def beam_to_sky(beam, pixsize_x: float, pixsize_y: float) -> dict:
    """`fwhm_major`, `fwhm_minor` (radians) and `pa` of `beam` on a sky whose
    pixels are `pixsize_x` by `pixsize_y` radians: a / px^2, b / (px py) and
    c / py^2, then the shape formulas of include/cip_restore.h. Host-only."""
    px, py = float(pixsize_x), float(pixsize_y)
    if not (math.isfinite(px) and math.isfinite(py) and px > 0.0 and py > 0.0):
        raise ValueError("pixel sizes must be finite and > 0")
    b = _as_struct(beam)
    a, bb, c = b.a / (px * px), b.b / (px * py), b.c / (py * py)
    tr, d = a + c, math.hypot(a - c, 2.0 * bb)
    lmin, lmax = 0.5 * (tr - d), 0.5 * (tr + d)
    if not (a > 0.0 and c > 0.0 and a * c - bb * bb > 0.0 and lmin > 0.0):
        raise ValueError("the beam's form is not positive definite")
    pa = -0.5 * math.atan2(2.0 * bb, a - c)
    if pa <= -0.5 * math.pi:
        pa += math.pi
    return {"fwhm_major": 2.0 * math.sqrt(math.log(2.0) / lmin), "fwhm_minor": 2.0 * math.sqrt(math.log(2.0) / lmax),
            "pa": pa}


# ---------------------------------------------------------------- device ----
def _check_image(img, shape, dev, name):
    if img.dim() != 2:
        raise ValueError(f"{name} must be a float64 2-D image, got {img.dtype} {tuple(img.shape)}")
    check_array(img, (torch.float64,), shape, dev, name)


def device_fit_beam(psf: "torch.Tensor", *, psf_centre: Optional[tuple] = None, cut: float = _lib.BEAM_FIT_CUT,
                    radius: int = _lib.BEAM_FIT_RADIUS) -> dict:
    """
    The clean beam of the device float64 `psf` (px, py): the least-squares
    Gaussian through the pixels at or above `cut` times the centre pixel, within
    `radius` pixels of `psf_centre` (default (px // 2, py // 2), where
    `device_ms2dirty(psf=True)` puts the peak). Only the small window is copied
    to the host; the fit itself is `cip_beam_fit_window`.
    """
    require_gpu()
    _check_image(psf, None, psf.device, "psf")
    cx, cy = (-1, -1) if psf_centre is None else (int(psf_centre[0]), int(psf_centre[1]))
    if psf_centre is not None and (cx < 0 or cy < 0):
        raise ValueError("psf_centre must lie inside the PSF")
    out = _lib.Beam()
    call(psf.device, "cip_beam_fit", psf, int(psf.shape[0]), int(psf.shape[1]), cx, cy, float(cut), int(radius), STREAM,
         ctypes.byref(out))
    return out.as_dict()


def device_restore(model: "torch.Tensor", residual: Optional["torch.Tensor"], beam, *, radius: Optional[int] = None,
                   tol: float = 1e-8, out: Optional["torch.Tensor"] = None, inplace: bool = False):
    """
    The restored image of the device float64 `model` (nx, ny): the model
    convolved with `beam` over a (2 R + 1)^2 support, plus `residual` (None:
    nothing added). Returns the image, queued on the current stream.

    `radius`: R, at most 32; None takes `beam_radius(beam, tol)`, where the
    beam has fallen to `tol`. `out` receives the image (it may be `residual`,
    never `model`); `inplace=True` writes it into `residual`. Work is done
    only around the model's non-zero pixels.
    """
    require_gpu()
    dev, shape = model.device, tuple(model.shape)
    _check_image(model, None, dev, "model")
    if residual is not None:
        _check_image(residual, shape, dev, "residual")
    if inplace:
        if residual is None or out is not None:
            raise ValueError("inplace=True writes into residual: it needs one, and no out")
        out = residual
    if out is not None:
        _check_image(out, shape, dev, "out")
        if out.data_ptr() == model.data_ptr():
            raise ValueError("out must not be the model (it may be the residual)")
    b = _as_struct(beam)
    if radius is None:
        r = beam_radius(b, tol)
    else:
        r = int(radius)
        if r < 0:
            raise ValueError("radius must be >= 0 (None: from the beam and tol)")
    if out is None:
        out = torch.empty_like(model)
    call(dev, "cip_restore", model, residual, shape[0], shape[1], ctypes.byref(b), r, STREAM, out)
    return out


def restore(model, residual, beam, *, radius: Optional[int] = None, tol: float = 1e-8, device=None):
    """
    `device_restore` for host or device arrays: numpy in -> numpy out, torch
    in -> torch out (on the GPU). The inputs are never modified.
    """
    require_gpu()
    dev = target_device(device)
    numpy_in = isinstance(model, np.ndarray)
    with torch.cuda.device(dev):
        model_d = to_device(model, torch.float64, dev)
        res_d = None if residual is None else to_device(residual, torch.float64, dev)
        out = device_restore(model_d, res_d, beam, radius=radius, tol=tol)
        return out.cpu().numpy() if numpy_in else out
