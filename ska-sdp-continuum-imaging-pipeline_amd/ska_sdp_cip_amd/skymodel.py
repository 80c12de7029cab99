"""
Sky-model predict on the GPU: the visibilities of a component list (point and
Gaussian sources with positions, fluxes and Taylor-term spectra) by the direct
Fourier sum, `cip_dft_predict` of libcip_hip.so.

The operator is defined exactly in include/cip_dft.h:

    model[r, c] = sum_k S_k(c) G_k(r, c) exp(-2 pi i f_c / c0 (u_r l_k + v_r m_k - w_r (n_k - 1)))

with `S_k(c) = sum_t flux[k, t] x_c^t` in the basis of `mfs.taylor_basis` and
G the Gaussian envelope of a component with a shape. It is the sign of
`synthetic.predict_visibilities` and of the degridder. A component's flux is
what the visibilities see (no 1 / n), so `SkyModel.from_image` divides the
pixels of a w-stacking image by n. The sum is exact in the positions: no grid,
no pixel, and nothing of the gridder's epsilon.
"""

from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._call import (STREAM, VIS_DTYPES, WGT_DTYPES, call, check_array, check_rows, require_gpu, target_device,
                    to_device, vis_arg, wgt_arg)

try:
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None


class SkyModel:
    """
    A component list as tensors on one device (CPU tensors are allowed: the
    model is built on the host and moved with `.to(device)`):

    * `lm` (ncomp, 2) float64 direction cosines,
    * `flux` (ncomp, nterms) float64 Taylor coefficients about `ref_freq`
      (nterms 1 .. 3; `ref_freq` is not used when nterms == 1),
    * `shape` None (point sources) or (ncomp, 3) float64: FWHM of the major
      and the minor axis (radians) and the position angle (radians, from +m
      towards +l); a row with both FWHM 0 is a point source.

    Validated on construction; the tensors are not copied.
    """

    def __init__(self, lm, flux, ref_freq: Optional[float] = None, shape=None):
        if not (torch.is_tensor(lm) and torch.is_tensor(flux)) or (shape is not None and not torch.is_tensor(shape)):
            raise ValueError("lm, flux and shape must be torch tensors")
        if lm.dim() != 2 or lm.shape[1] != 2 or lm.dtype != torch.float64:
            raise ValueError(f"lm must be float64 of shape (ncomp, 2), got {lm.dtype} {tuple(lm.shape)}")
        ncomp = int(lm.shape[0])
        if flux.dim() != 2 or flux.shape[0] != ncomp or flux.dtype != torch.float64:
            raise ValueError(f"flux must be float64 of shape ({ncomp}, nterms), got {flux.dtype} {tuple(flux.shape)}")
        nterms = int(flux.shape[1])
        if not 1 <= nterms <= _lib.MFS_MAX_TERMS:
            raise ValueError(f"nterms must be in 1 .. {_lib.MFS_MAX_TERMS}, got {nterms}")
        if shape is not None and (tuple(shape.shape) != (ncomp, 3) or shape.dtype != torch.float64):
            raise ValueError(f"shape must be float64 of shape ({ncomp}, 3), got {shape.dtype} {tuple(shape.shape)}")
        if nterms > 1 and (ref_freq is None or not np.isfinite(ref_freq) or not ref_freq > 0.0):
            raise ValueError("ref_freq must be finite and > 0 when nterms > 1")
        for name, t in (("flux", flux), ("shape", shape)):
            if t is not None and t.device != lm.device:
                raise ValueError(f"{name} on {t.device}, lm on {lm.device}")
        self.lm = lm.contiguous()
        self.flux = flux.contiguous()
        self.shape = None if shape is None else shape.contiguous()
        self.ref_freq = 0.0 if ref_freq is None else float(ref_freq)

    def __len__(self) -> int:
        return int(self.lm.shape[0])

    @property
    def nterms(self) -> int:
        return int(self.flux.shape[1])

    @property
    def device(self):
        return self.lm.device

    def to(self, device) -> "SkyModel":
        """The same model on `device`."""
        shape = None if self.shape is None else self.shape.to(device)
        return SkyModel(self.lm.to(device), self.flux.to(device), self.ref_freq or None, shape)

    @classmethod
    def from_point_sources(cls, sources: Sequence, ref_freq: Optional[float] = None, device=None) -> "SkyModel":
        """
        From `synthetic.PointSource`s (`l`, `m`, `flux`); a `flux` that is a
        sequence holds the Taylor coefficients about `ref_freq` (the same
        number for every source).
        """
        lm = np.array([[float(s.l), float(s.m)] for s in sources], dtype=np.float64).reshape(-1, 2)
        flux = [np.atleast_1d(np.asarray(s.flux, dtype=np.float64)) for s in sources]
        if len({f.shape for f in flux}) > 1:
            raise ValueError("every source needs the same number of Taylor coefficients")
        flux = np.array(flux, dtype=np.float64).reshape(len(lm), -1) if len(lm) else np.zeros((0, 1))
        return cls(torch.from_numpy(lm).to(device), torch.from_numpy(flux).to(device), ref_freq)

    @classmethod
    def from_image(cls, model, pixsize_x: float, pixsize_y: float, do_wstacking: bool, threshold: float = 0.0,
                   ref_freq: Optional[float] = None) -> "SkyModel":
        """
        The pixels of a model image with |value| > `threshold` as point
        sources, on the image's device. Pixel (i, j) of an (npix_x, npix_y)
        image lies at l = (i - npix_x // 2) pixsize_x, m = (j - npix_y // 2)
        pixsize_y (the gridder's rule). Under w-stacking the gridder's pixel
        value I is a flux of I / n, n = sqrt(1 - l^2 - m^2), so `flux = I / n`;
        without it `flux = I`. A list (or a 3-D stack) of Taylor-term images
        gives `nterms > 1` about `ref_freq`, over the union of the terms'
        supports; components come in row-major pixel order.
        """
        stack = torch.stack(list(model)) if isinstance(model, (list, tuple)) else model
        if stack.dim() == 2:
            stack = stack[None]
        if stack.dim() != 3 or not 1 <= stack.shape[0] <= _lib.MFS_MAX_TERMS:
            raise ValueError(f"model must be an (npix_x, npix_y) image or 1 .. {_lib.MFS_MAX_TERMS} of them, got "
                             f"{tuple(stack.shape)}")
        stack = stack.to(torch.float64)
        nx, ny = int(stack.shape[1]), int(stack.shape[2])
        ij = torch.nonzero((stack.abs() > float(threshold)).any(dim=0))  # (ncomp, 2), row-major order
        l = (ij[:, 0] - nx // 2).to(torch.float64) * float(pixsize_x)  # noqa: E741
        m = (ij[:, 1] - ny // 2).to(torch.float64) * float(pixsize_y)
        flux = stack[:, ij[:, 0], ij[:, 1]].T
        if do_wstacking:
            e = l * l + m * m
            nm1 = -e / (torch.sqrt(1.0 - e) + 1.0)
            flux = flux / (nm1 + 1.0)[:, None]
        return cls(torch.stack([l, m], dim=1), flux.contiguous(), ref_freq)


def device_dft_predict(uvw, freq, sky: SkyModel, wgt=None, *, out=None, mode: str = "set", w_term: bool = True,
                       fast: bool = False, dtype=None):
    """
    `cip_dft_predict` on device tensors: the visibilities of `sky` at (uvw
    (nrow, 3), freq (nchan,)), both float64. `mode="set"` writes `wgt * model`
    (`model` without `wgt`) into `out`, or into a new (nrow, nchan) tensor of
    `dtype` (default complex64); "add" and "subtract" need `out`, which holds
    a column and receives `out +- wgt * model`. A sample of weight zero becomes
    exactly 0 under "set" and keeps its bits under the other two. `w_term`:
    the w term of wide-field data (False: the 2-D convention of a
    `do_wstacking=False` image). `fast=True` selects the single-precision
    class (include/cip_dft.h). Stream-ordered; returns the column.
    """
    require_gpu()
    if mode not in _lib.DFT_MODES:
        raise ValueError(f"mode must be one of {sorted(_lib.DFT_MODES)}, got {mode!r}")
    nrow, nchan = check_rows(uvw, freq, "device_dft_predict inputs")
    dev = uvw.device
    ncomp = len(sky)
    check_array(sky.lm, (torch.float64,), (ncomp, 2), dev, "sky.lm")
    check_array(sky.flux, (torch.float64,), (ncomp, sky.nterms), dev, "sky.flux")
    if sky.shape is not None:
        check_array(sky.shape, (torch.float64,), (ncomp, 3), dev, "sky.shape")
    if wgt is not None:
        check_array(wgt, WGT_DTYPES, (nrow, nchan), dev, "wgt")
    if out is None:
        if mode != "set":
            raise ValueError(f"mode={mode!r} needs `out` holding the column to change")
        dtype = torch.complex64 if dtype is None else dtype
        if dtype not in VIS_DTYPES:
            raise ValueError(f"dtype must be complex64/complex128, got {dtype}")
        out = torch.empty((nrow, nchan), dtype=dtype, device=dev)
    else:  # the library writes nrow * nchan cells through the raw pointer
        check_array(out, VIS_DTYPES, (nrow, nchan), dev, "out")
    flags = _lib.DFT_MODES[mode] | (_lib.DFT_WTERM if w_term else 0) | (_lib.DFT_FAST if fast else 0)
    call(dev, "cip_dft_predict", uvw, nrow, freq, nchan, sky.lm, sky.flux, sky.shape, ncomp, sky.nterms,
         float(sky.ref_freq), flags, *wgt_arg(wgt), STREAM, *vis_arg(out))
    return out


def dft_predict(uvw, freq, sky: SkyModel, wgt=None, *, out=None, mode: str = "set", w_term: bool = True,
                fast: bool = False, dtype=None, device=None):
    """
    `device_dft_predict` for host arrays: numpy in -> numpy out. `out` (for
    "add" and "subtract") is a numpy column that is not modified; the changed
    column is returned.
    """
    require_gpu()
    dev = target_device(device)
    with torch.cuda.device(dev):
        wgt_d = None
        if wgt is not None:
            wgt_d = to_device(wgt, torch.float32 if wgt.dtype == np.float32 else torch.float64, dev)
        out_d = None
        if out is not None:
            out_d = to_device(out, torch.complex64 if out.dtype == np.complex64 else torch.complex128, dev)
        res = device_dft_predict(to_device(uvw, torch.float64, dev), to_device(freq, torch.float64, dev), sky.to(dev),
                                 wgt_d, out=out_d, mode=mode, w_term=w_term, fast=fast, dtype=dtype)
        return res.cpu().numpy()
