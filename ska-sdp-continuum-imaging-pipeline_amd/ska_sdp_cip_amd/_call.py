"""
The one call path from the Python modules into libcip_hip.so.

`call(device, "cip_x", ...)` makes `device` current for the call (the library
works on the current device), puts that device's current HIP stream where the
arguments hold `STREAM`, passes tensors as `ptr(t)` and maps the status through
`_lib.check`. The helpers around it state once what every call site needs:
NULL for None and for empty tensors (`ptr`), the dtype codes of visibilities
and weights (`vis_arg`, `wgt_arg`) and the checks that several entry points
share. This module imports `_lib` and torch and nothing else of the package.
"""

from __future__ import annotations

import numpy as np

from . import _lib

try:  # torch is plumbing (device memory, streams)
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None

STREAM = object()  # in `call`'s arguments: the device's current HIP stream
_VIS_CODES = {} if torch is None else {torch.complex64: _lib.CIP_C64, torch.complex128: _lib.CIP_C128}
_WGT_CODES = {} if torch is None else {torch.float32: _lib.CIP_F32, torch.float64: _lib.CIP_F64}
VIS_DTYPES, WGT_DTYPES = tuple(_VIS_CODES), tuple(_WGT_CODES)


def require_gpu():
    if torch is None or not torch.cuda.is_available():
        raise RuntimeError(
            "ska_sdp_cip_amd.ms2dirty needs a ROCm GPU (MI355X); no CPU fallback"
        )


def target_device(device=None):
    """`device` as a torch.device; None: the current GPU."""
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def to_device(x, dtype, device):
    if isinstance(x, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(x))
        return t.to(device=device, dtype=dtype, non_blocking=False)
    return x.to(device=device, dtype=dtype).contiguous()


def check_tensor(t, device, what):
    """Contiguous, on a GPU, and on `device` (`call` makes it current)."""
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what}: need contiguous device tensors")
    if t.device != device:
        raise ValueError(f"{what}: tensor on {t.device}, expected {device}")


def check_array(t, dtypes, shape, device, what):
    """`t` has one of `dtypes`, the shape `shape` (None: any) and passes `check_tensor`."""
    if t.dtype not in dtypes or (shape is not None and tuple(t.shape) != tuple(shape)):
        names = "/".join(str(d).replace("torch.", "") for d in dtypes)
        raise ValueError(f"{what} must be {names}" + ("" if shape is None else f" of shape {tuple(shape)}")
                         + f", got {t.dtype} {tuple(t.shape)}")
    check_tensor(t, device, what)


def check_rows(uvw, freq, what):
    """uvw (nrow, 3) and freq (nchan,), float64, on uvw's device; returns (nrow, nchan)."""
    if uvw.dim() != 2 or uvw.shape[1] != 3 or freq.dim() != 1:
        raise ValueError("uvw must have shape (nrow, 3) and freq (nchan,)")
    if uvw.dtype != torch.float64 or freq.dtype != torch.float64:
        raise ValueError("uvw and freq must be float64")
    check_tensor(uvw, uvw.device, what)
    check_tensor(freq, uvw.device, what)
    return int(uvw.shape[0]), int(freq.shape[0])


def ptr(t):
    """The device pointer of `t`; None (NULL) for None and for a tensor without elements."""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def vis_arg(t):
    """(pointer, dtype code) of a visibility tensor; None -> (None, CIP_C64)."""
    if t is None:
        return None, _lib.CIP_C64
    if t.dtype not in _VIS_CODES:
        raise ValueError(f"vis dtype must be complex64/complex128, got {t.dtype}")
    return ptr(t), _VIS_CODES[t.dtype]


def wgt_arg(t):
    """(pointer, dtype code) of a weight tensor; None -> (None, CIP_NONE)."""
    if t is None:
        return None, _lib.CIP_NONE
    if t.dtype not in _WGT_CODES:
        raise ValueError(f"wgt dtype must be float32/float64, got {t.dtype}")
    return ptr(t), _WGT_CODES[t.dtype]


def call(device, name: str, *args) -> None:
    """`name(*args)` of the library on `device`: tensors go as `ptr(t)`, `STREAM`
    as the device's current stream; a negative status raises (`_lib.check`)."""
    if device.index not in (None, torch.cuda.current_device()):
        with torch.cuda.device(device):  # the guard costs microseconds: only entered when it changes the device
            call(device, name, *args)
        return
    stream = torch.cuda.current_stream(device).cuda_stream
    _lib.check(getattr(_lib.lib(), name)(
        *[stream if a is STREAM else ptr(a) if isinstance(a, torch.Tensor) else a for a in args]))
