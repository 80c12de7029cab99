"""
The noise of an image and the island mask built on it: an exact order
statistic (`cip_image_select`), the robust noise estimate from the median and
the median absolute deviation (`cip_image_noise`) and the hysteresis mask
(`cip_auto_mask`), all on the GPU.

The operators are defined exactly in include/cip_noise.h: samples are the
finite pixels inside `region`, the median is the lower median (a selection,
never a mean of two), `mad` the same rank among |x - median| and `sigma` =
`MAD_TO_SIGMA` * mad; the mask is every pixel at or above `grow` that an
8-connected (or 4-connected) path of such pixels joins to a pixel at or above
`seed`. Both are bit-identical to that numpy statement. The major-cycle loops
use them for `auto_threshold` and `auto_mask` (`deconvolve._major_cycles`).
"""

from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib
from ._call import STREAM, call, check_array, require_gpu, target_device, to_device

try:
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None

MAD_TO_SIGMA = _lib.MAD_TO_SIGMA


def _check_image(image, region=None, **masks):
    """A float64 contiguous 2-D device image; `region` and `masks` uint8 / bool
    of its shape on its device. Returns the masks as uint8 views."""
    if image.dim() != 2:
        raise ValueError(f"image must be a float64 2-D image, got {image.dtype} {tuple(image.shape)}")
    check_array(image, (torch.float64,), None, image.device, "image")
    views = []
    for name, m in (("region", region), *masks.items()):
        if m is not None:
            check_array(m, (torch.uint8, torch.bool), tuple(image.shape), image.device, name)
            m = m.view(torch.uint8)
        views.append(m)
    return views


def device_image_select(image: "torch.Tensor", rank: int, *, region: Optional["torch.Tensor"] = None):
    """
    The sample of 0-based `rank` among the sorted finite pixels of the device
    float64 image `image` (nx, ny) inside `region` ((nx, ny) uint8 / bool,
    nonzero where a pixel counts; None: everywhere): `np.sort(v)[rank]`, bit for
    bit. Returns (value, count), `count` the number of samples. A `rank`
    outside 0 .. count - 1 raises ValueError.
    """
    require_gpu()
    (region,) = _check_image(image, region)
    count, value = ctypes.c_int64(0), ctypes.c_double(0.0)
    call(image.device, "cip_image_select", image, int(image.shape[0]), int(image.shape[1]), region, int(rank), STREAM,
         ctypes.byref(count), ctypes.byref(value))
    return float(value.value), int(count.value)


def device_image_noise(image: "torch.Tensor", *, region: Optional["torch.Tensor"] = None) -> dict:
    """
    The robust noise of the device float64 image `image` (nx, ny) over its
    finite pixels inside `region`: a dict of `count`, `median` (the lower
    median), `mad` (the lower median of |x - median|) and `sigma` =
    `MAD_TO_SIGMA` * mad. Without a sample `count` is 0 and the rest NaN.
    Nothing image-sized is allocated or copied: two selects read the image a
    few times each and a few scalars come back.
    """
    require_gpu()
    (region,) = _check_image(image, region)
    out = _lib.NoiseResult()
    call(image.device, "cip_image_noise", image, int(image.shape[0]), int(image.shape[1]), region, STREAM,
         ctypes.byref(out))
    return out.as_dict()


def device_auto_mask(
    image: "torch.Tensor",
    seed: float,
    grow: Optional[float] = None,
    *,
    region: Optional["torch.Tensor"] = None,
    base: Optional["torch.Tensor"] = None,
    out: Optional["torch.Tensor"] = None,
    positive: bool = False,
    connectivity: int = 8,
):
    """
    The island mask of the device float64 image `image` (nx, ny): 1 on every
    pixel with |image| >= `grow` (None: `seed`) that a path of such pixels
    joins to a pixel with |image| >= `seed`, and wherever `base` is nonzero.
    `positive=True` compares the signed value, `connectivity` is 8 or 4,
    `region` limits both thresholds to its nonzero pixels (a gap severs an
    island). `out` (uint8 / bool; None: a new uint8 image) may be `base`.
    Returns (mask, info), `info` holding `n_seed`, `n_island`, `n_out` and
    `rounds`. Thresholds that are not finite with seed >= grow > 0 raise
    ValueError.
    """
    require_gpu()
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    region, base_u8, out_u8 = _check_image(image, region, base=base, out=out)
    if out is None:
        out = out_u8 = torch.empty(tuple(image.shape), dtype=torch.uint8, device=image.device)
    flags = (_lib.MASK_POSITIVE if positive else 0) | (_lib.MASK_CONN4 if connectivity == 4 else 0)
    result = _lib.MaskResult()
    call(image.device, "cip_auto_mask", image, int(image.shape[0]), int(image.shape[1]), float(seed),
         float(seed if grow is None else grow), region, base_u8, flags, STREAM, out_u8, ctypes.byref(result))
    return out, result.as_dict()


def _host_mask(m, dev):
    """A host or device mask as a device bool image (a copy); None stays None."""
    if m is None:
        return None
    return to_device((np.asarray(m) if not torch.is_tensor(m) else m) != 0, torch.bool, dev)


def image_noise(image, *, region=None, device=None) -> dict:
    """`device_image_noise` for a host or device image (numpy or torch); the
    inputs are never modified."""
    require_gpu()
    dev = target_device(device)
    with torch.cuda.device(dev):
        return device_image_noise(to_device(image, torch.float64, dev), region=_host_mask(region, dev))


def auto_mask(image, seed, grow=None, *, region=None, base=None, positive=False, connectivity=8, device=None):
    """`device_auto_mask` for host or device arrays: numpy in -> numpy out,
    torch in -> torch out (on the GPU). The inputs are never modified. Returns
    (mask, info) as `device_auto_mask`, the mask uint8."""
    require_gpu()
    dev = target_device(device)
    with torch.cuda.device(dev):
        mask, info = device_auto_mask(to_device(image, torch.float64, dev), seed, grow, region=_host_mask(region, dev),
                                      base=_host_mask(base, dev), positive=positive, connectivity=connectivity)
    return (mask.cpu().numpy() if isinstance(image, np.ndarray) else mask), info
