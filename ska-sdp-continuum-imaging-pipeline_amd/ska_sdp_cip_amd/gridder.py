"""
`ms2dirty`: MI355X drop-in for `ducc0.wgridder.ms2dirty` as the reference
calls it (`/root/reference/src/ska_sdp_cip/invert.py:170-183`).

Host side only: moves arrays to HBM (torch tensors are used purely as device
buffers), calls `cip_ms2dirty` of libcip_hip.so on the current HIP stream and
returns the dirty image. Accepts numpy arrays (returns numpy) or CUDA/HIP
torch tensors (returns a torch tensor on the same device, no host round trip).

Definition computed (ducc0's documented ms2dirty):
    dirty[i, j] = (1/n) sum_{r,c} wgt[r,c] Re{ ms[r,c]
                  exp(2 pi i f_c/c (u_r l + v_r m - w_r (n - 1))) }
with l = (i - npix_x/2) pixsize_x, m = (j - npix_y/2) pixsize_y,
n = sqrt(1 - l^2 - m^2); in 2-D mode (do_wstacking=False) n := 1.

`dirty2ms` is its exact transpose (ducc0.wgridder.dirty2ms, `cip_dirty2ms`):
    vis[r,c] = wgt[r,c] sum_{i,j} dirty[i,j]/n
               exp(-2 pi i f_c/c (u_r l + v_r m - w_r (n - 1)))
"""

from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib
from ._call import (STREAM, VIS_DTYPES, WGT_DTYPES, call, check_array, check_rows, require_gpu, target_device,
                    to_device, vis_arg, wgt_arg)

try:  # torch is plumbing (device memory, streams); import lazily-safe
    import torch
except ModuleNotFoundError:  # pragma: no cover - torch is in the image
    torch = None


def device_ms2dirty(
    uvw: "torch.Tensor",
    freq: "torch.Tensor",
    vis: "torch.Tensor",
    wgt: Optional["torch.Tensor"],
    npix_x: int,
    npix_y: int,
    pixsize_x: float,
    pixsize_y: float,
    *,
    epsilon: float = 1e-4,
    support: Optional[int] = None,
    do_wstacking: bool = False,
    out: Optional["torch.Tensor"] = None,
    sum_weights: Optional["torch.Tensor"] = None,
    single_precision_accumulation: bool = False,
    psf: bool = False,
    normalise: bool = False,
    synchronize: bool = True,
    resident_inputs: bool = False,
    reuse_plan: bool = False,
    planes: Optional[tuple] = None,
) -> tuple["torch.Tensor", _lib.GridderParams]:
    """
    Device-resident ms2dirty: all tensors already in HBM on the current device.
    Returns (dirty fp64 tensor (npix_x, npix_y), params). `sum_weights`
    (fp64, 1 element) receives the sum of `wgt` when given.
    `single_precision_accumulation` (complex64 `vis` only) selects the packed
    single-precision class (CIP_ACC_SINGLE, include/cip.h): quantisation
    2^-19 of max|w V| per contribution, like ducc0's float gridding; the
    default accumulates every input in 64-bit fixed point (fp64 class).
    `psf=True` grids unit visibilities instead of `vis` (the point-spread
    function with the same weights; `vis` may then be None).
    `normalise=True` (CIP_NORMALISE) returns the image divided by the weight
    sum of this call (the reference's (1 / total_weight) * image,
    invert.py:119-149), fused into the FFT epilogue; not for partial images
    that are summed across ranks afterwards.
    `synchronize=False` (CIP_ASYNC) returns once the work is queued on the
    current stream: `out` / `sum_weights` are valid in stream order (the next
    kernel or copy on that stream sees them; the host must synchronise before
    reading them). The planner's two mid-call readbacks still wait.
    `resident_inputs=True` (CIP_PIPELINE, with `synchronize=False` only)
    promises that uvw / freq / vis / wgt were complete before the previous
    asynchronous call returned and stay unchanged (resident data, as in the
    benchmark): the planner of this call then runs beside the previous call's
    scatter and FFT instead of after all work queued on the stream.
    `reuse_plan=True` (CIP_REUSE_PLAN, not with `resident_inputs`) promises
    that uvw, freq and the row layout equal those of this thread's previous
    planned call (e.g. the Stokes parameters and PSF of one facet): if that
    call's geometry matches, its tile plan is used again and only the weight
    sum and max |w V| are computed (images identical to a planned call's).
    `planes=(begin, end)` (w-stacking only, cip_ms2dirty_wplanes): the partial
    image of w planes [begin, end) of the stack - the share of one GPU when the
    plane groups of ONE image are split over GPUs (SURVEY.md 8(e) option 2,
    `wplanes.py`); the partial images of a partition of [0, nplanes) sum to
    the whole image (the final w correction and `normalise` are linear and
    applied to each part; `sum_weights` is the whole call's weight sum).
    """
    if planes is not None and not do_wstacking:
        raise ValueError("planes=(begin, end) needs do_wstacking=True")
    if psf:
        vis = None  # never read
    elif vis is None:
        raise ValueError("vis dtype must be complex64/complex128, got None")
    vis_args, wgt_args = vis_arg(vis), wgt_arg(wgt)
    nrow, nchan = check_rows(uvw, freq, "device_ms2dirty inputs")
    if vis is not None:
        check_array(vis, VIS_DTYPES, (nrow, nchan), uvw.device, "ms")
    if wgt is not None:
        check_array(wgt, WGT_DTYPES, (nrow, nchan), uvw.device, "wgt")
    out = _invert_outputs(out, sum_weights, npix_x, npix_y, uvw.device, synchronize, resident_inputs, reuse_plan)
    params = _lib.GridderParams()
    call(uvw.device, "cip_ms2dirty" if planes is None else "cip_ms2dirty_wplanes",
         uvw, nrow, freq, nchan, *vis_args, *wgt_args, int(npix_x), int(npix_y), float(pixsize_x),
         float(pixsize_y), float(epsilon), int(support or 0),
         _invert_flags(do_wstacking, single_precision_accumulation, psf, normalise, synchronize, resident_inputs,
                       reuse_plan),
         *(() if planes is None else (int(planes[0]), int(planes[1]))), STREAM, out, sum_weights, params)
    return out, params


def _invert_outputs(out, sum_weights, npix_x, npix_y, device, synchronize, resident_inputs, reuse_plan):
    """The flag guards and the `out` / `sum_weights` checks of the device_ms2dirty* calls; returns `out`
    (allocated when None)."""
    if resident_inputs and synchronize:
        raise ValueError("resident_inputs=True needs synchronize=False")
    if reuse_plan and resident_inputs:
        raise ValueError("reuse_plan=True cannot be combined with resident_inputs=True")
    if out is None:
        out = torch.empty((npix_x, npix_y), dtype=torch.float64, device=device)
    else:  # the library writes npix_x * npix_y doubles through the raw pointer
        check_array(out, (torch.float64,), (int(npix_x), int(npix_y)), device, "out")
    if sum_weights is not None:
        if sum_weights.numel() != 1:
            raise ValueError("sum_weights must be a float64 tensor of one element")
        check_array(sum_weights, (torch.float64,), None, device, "sum_weights")
    return out


def _invert_flags(do_wstacking, single_precision_accumulation, psf, normalise, synchronize, resident_inputs,
                  reuse_plan):
    """The CIP_* flag word of a cip_ms2dirty* call, from device_ms2dirty's keywords."""
    return ((_lib.CIP_WSTACKING if do_wstacking else 0)
            | (_lib.CIP_ACC_SINGLE if single_precision_accumulation else 0)
            | (_lib.CIP_PSF if psf else 0)
            | (_lib.CIP_NORMALISE if normalise else 0)
            | (0 if synchronize else _lib.CIP_ASYNC)
            | (_lib.CIP_PIPELINE if resident_inputs else 0)
            | (_lib.CIP_REUSE_PLAN if reuse_plan else 0))


def device_ms2dirty_stokes_i(
    uvw: "torch.Tensor",
    freq: "torch.Tensor",
    vis4: Optional["torch.Tensor"],
    flags4: Optional["torch.Tensor"],
    wgt4: "torch.Tensor",
    npix_x: int,
    npix_y: int,
    pixsize_x: float,
    pixsize_y: float,
    *,
    epsilon: float = 1e-4,
    support: Optional[int] = None,
    do_wstacking: bool = False,
    out: Optional["torch.Tensor"] = None,
    sum_weights: Optional["torch.Tensor"] = None,
    single_precision_accumulation: bool = False,
    psf: bool = False,
    normalise: bool = False,
    synchronize: bool = True,
    resident_inputs: bool = False,
    reuse_plan: bool = False,
) -> tuple["torch.Tensor", _lib.GridderParams]:
    """
    device_ms2dirty on the raw linear-feed columns (cip_ms2dirty_stokes_i):
    vis4 (nrow, nchan, 4) complex64 XX, XY, YX, YY, flags4 (nrow, nchan, 4)
    bool/uint8 or None, wgt4 (nrow, nchan, 4) float32. Stokes I and the
    effective weights (reference invert.py:78-116) are formed inside the
    planner and scatter as each visibility is loaded - no intermediate
    columns; the image is bit-identical to device_stokes_i + device_ms2dirty.
    Keyword arguments as device_ms2dirty.
    """
    nrow, nchan = check_rows(uvw, freq, "device_ms2dirty_stokes_i inputs")
    dev, shape = uvw.device, (nrow, nchan, 4)
    if psf:
        vis4 = None
    elif vis4 is None:
        raise ValueError(f"vis4 must be complex64 of shape {shape}")
    else:
        check_array(vis4, (torch.complex64,), shape, dev, "vis4")
    if wgt4 is None:
        raise ValueError(f"wgt4 must be float32 of shape {shape}")
    check_array(wgt4, (torch.float32,), shape, dev, "wgt4")
    if flags4 is not None:
        check_array(flags4, (torch.bool, torch.uint8), shape, dev, "flags4")
        flags4 = flags4.view(torch.uint8)
    out = _invert_outputs(out, sum_weights, npix_x, npix_y, dev, synchronize, resident_inputs, reuse_plan)
    params = _lib.GridderParams()
    call(dev, "cip_ms2dirty_stokes_i", uvw, nrow, freq, nchan, vis4, flags4, wgt4, int(npix_x), int(npix_y),
         float(pixsize_x), float(pixsize_y), float(epsilon), int(support or 0),
         _invert_flags(do_wstacking, single_precision_accumulation, psf, normalise, synchronize, resident_inputs,
                       reuse_plan),
         STREAM, out, sum_weights, params)
    return out, params


def device_stokes(vis4: "torch.Tensor", flags4: "torch.Tensor", wgt4: "torch.Tensor", stokes: str = "I"):
    """
    Stokes parameter `stokes` ("I", "Q", "U", "V") on the device (cip_stokes;
    linear feeds XX, XY, YX, YY; I is the reference's invert.py:72-116,
    bit-exact): -> (visibilities complex64 (nrow, nchan), effective weights
    float32 (nrow, nchan)).
    """
    require_gpu()
    if stokes not in _lib.STOKES_CODES:
        raise ValueError(f"stokes must be one of I, Q, U, V, got {stokes!r}")
    return _stokes("cip_stokes", vis4, flags4, wgt4, _lib.STOKES_CODES[stokes])


def _stokes(name, vis4, flags4, wgt4, *code):
    """device_stokes / device_stokes_i: the checks, the outputs and the call (`code`: cip_stokes' parameter)."""
    if vis4.dim() != 3 or vis4.shape[-1] != 4:
        raise ValueError("vis4, flags4, wgt4 must all have shape (nrow, nchan, 4)")
    dev, shape = vis4.device, tuple(vis4.shape)
    fl = flags4.to(torch.uint8) if flags4.dtype != torch.uint8 else flags4
    check_array(vis4, (torch.complex64,), shape, dev, "vis4")
    check_array(fl, (torch.uint8,), shape, dev, "flags4")
    check_array(wgt4, (torch.float32,), shape, dev, "wgt4")
    vis_s = torch.empty(shape[:2], dtype=torch.complex64, device=dev)
    eff = torch.empty(shape[:2], dtype=torch.float32, device=dev)
    call(dev, name, vis4, fl, wgt4, shape[0] * shape[1], *code, STREAM, vis_s, None, None, eff)
    return vis_s, eff


def device_facet_rephase(uvw: "torch.Tensor", freq: "torch.Tensor", vis: Optional["torch.Tensor"],
                         l0: float, m0: float):
    """
    Facet data (cip_facet_rephase): visibilities rephased to the facet centre
    (l0, m0) of the image plane and baselines rotated into the facet's frame,
    so that device_ms2dirty of the result is the dirty image on the facet's own
    tangent plane centred on (l0, m0). Returns (uvw_f, vis_f); vis may be None
    (uvw only, for a facet PSF).
    """
    require_gpu()
    nrow, nchan = check_rows(uvw, freq, "device_facet_rephase inputs")
    if vis is not None:
        check_array(vis, VIS_DTYPES, (nrow, nchan), uvw.device, "vis")
    uvw_f = torch.empty_like(uvw)
    vis_f = torch.empty_like(vis) if vis is not None else None
    call(uvw.device, "cip_facet_rephase", uvw, nrow, freq, nchan, *vis_arg(vis), float(l0), float(m0), STREAM,
         uvw_f, vis_f)
    return uvw_f, vis_f


def device_stokes_i(vis4: "torch.Tensor", flags4: "torch.Tensor", wgt4: "torch.Tensor"):
    """
    Stokes I on the device (cip_stokes_i; reference invert.py:72-116, bit-exact
    with its numpy arithmetic): (nrow, nchan, 4) complex64 visibilities,
    bool/uint8 flags and float32 weights -> (vis_i complex64 (nrow, nchan),
    effective weights float32 (nrow, nchan)).
    """
    require_gpu()
    return _stokes("cip_stokes_i", vis4, flags4, wgt4)


def _stage(uvw, freq, wgt, mask, dev):
    """ms2dirty's / dirty2ms's uvw, freq (float64) and wgt (its own float32 / float64, zeroed where `mask`
    is 0; None without either) on `dev`."""
    uvw_d = to_device(uvw, torch.float64, dev)
    freq_d = to_device(np.asarray(freq, dtype=np.float64) if not torch.is_tensor(freq) else freq, torch.float64, dev)
    wgt_d = None
    if wgt is not None:
        wdt = torch.float32 if (wgt.dtype in (np.float32, torch.float32)) else torch.float64
        wgt_d = to_device(wgt, wdt, dev)
    if mask is not None:
        m = to_device(np.asarray(mask) if not torch.is_tensor(mask) else mask, torch.bool, dev)
        wgt_d = m.to(torch.float32) if wgt_d is None else wgt_d * m.to(wgt_d.dtype)
    return uvw_d, freq_d, wgt_d


def ms2dirty(  # pylint: disable=too-many-arguments,unused-argument
    uvw,
    freq,
    ms,
    wgt=None,
    npix_x: int = None,
    npix_y: int = None,
    pixsize_x: float = None,
    pixsize_y: float = None,
    nu: int = 0,
    nv: int = 0,
    epsilon: float = 1e-4,
    do_wstacking: bool = False,
    nthreads: int = 1,
    verbosity: int = 0,
    mask=None,
    double_precision_accumulation: Optional[bool] = None,
    *,
    support: Optional[int] = None,
    device=None,
    return_params: bool = False,
):
    """
    Drop-in for `ducc0.wgridder.ms2dirty` (same positional order as the call
    at reference invert.py:170-183). `nu`, `nv`, `nthreads` and `verbosity`
    are accepted for signature compatibility and ignored (the grid is chosen
    from epsilon / `support`). Accumulation is 64-bit fixed point unless
    `double_precision_accumulation=False` is passed explicitly with complex64
    `ms` (ducc0's float gridding class, CIP_ACC_SINGLE); left at None it is the
    fp64 class, at least as accurate as ducc0 in every mode. `mask` (uint8,
    shape of ms) zeroes the weights where 0. Output dtype follows ducc:
    float32 for complex64 `ms`, else float64.
    """
    require_gpu()
    if npix_x is None or npix_y is None or pixsize_x is None or pixsize_y is None:
        raise TypeError("npix_x, npix_y, pixsize_x and pixsize_y are required")
    dev = target_device(device)
    numpy_in = isinstance(ms, np.ndarray)
    ms_dtype = ms.dtype
    single = ms_dtype in (np.complex64, torch.complex64)
    with torch.cuda.device(dev):
        uvw_d, freq_d, wgt_d = _stage(uvw, freq, wgt, mask, dev)
        vis_d = to_device(ms, torch.complex64 if single else torch.complex128, dev)
        dirty, params = device_ms2dirty(
            uvw_d, freq_d, vis_d, wgt_d, int(npix_x), int(npix_y), float(pixsize_x),
            float(pixsize_y), epsilon=epsilon, support=support, do_wstacking=do_wstacking,
            single_precision_accumulation=single and double_precision_accumulation is False)
        dirty = dirty.to(torch.float32) if single else dirty
        result = dirty.cpu().numpy() if numpy_in else dirty
    if return_params:
        return result, params
    return result


def device_dirty2ms(
    uvw: "torch.Tensor",
    freq: "torch.Tensor",
    dirty: "torch.Tensor",
    wgt: Optional["torch.Tensor"],
    pixsize_x: float,
    pixsize_y: float,
    *,
    epsilon: float = 1e-4,
    support: Optional[int] = None,
    do_wstacking: bool = False,
    out: Optional["torch.Tensor"] = None,
    out_dtype=None,
    subtract: bool = False,
    reuse_plan: bool = False,
) -> tuple["torch.Tensor", _lib.GridderParams]:
    """
    Device-resident dirty2ms (cip_dirty2ms): model visibilities of the fp64
    image `dirty` (npix_x, npix_y) at (uvw, freq), all tensors already in HBM.
    Returns (vis (nrow, nchan), params). `out` (complex64 / complex128)
    receives the result, else a new tensor of `out_dtype` (default
    complex128); the arithmetic is fp64 either way. `subtract=True`
    (CIP_SUBTRACT, needs `out`): `out` holds data and receives
    out - wgt * model, the major cycle's residual. `reuse_plan=True`
    (CIP_REUSE_PLAN): as device_ms2dirty - a predict after an invert of the
    same uvw / freq / geometry on this thread runs through that invert's tile
    plan. Supports 4..16 only; `dirty` is not modified.
    """
    if out_dtype is None:
        out_dtype = torch.complex128
    nrow, nchan = check_rows(uvw, freq, "device_dirty2ms inputs")
    dev = uvw.device
    if dirty.dim() != 2:
        raise ValueError(f"dirty must be a float64 (npix_x, npix_y) image, got {dirty.dtype} "
                         f"{tuple(dirty.shape)}")
    check_array(dirty, (torch.float64,), None, dev, "dirty")
    wgt_args = wgt_arg(wgt)
    if wgt is not None:
        check_array(wgt, WGT_DTYPES, (nrow, nchan), dev, "wgt")
    if out is None:
        if subtract:
            raise ValueError("subtract=True needs `out` holding the visibilities to subtract from")
        if out_dtype not in VIS_DTYPES:
            raise ValueError(f"out_dtype must be complex64/complex128, got {out_dtype}")
        out = torch.empty((nrow, nchan), dtype=out_dtype, device=dev)
    else:  # the library writes nrow * nchan cells through the raw pointer
        check_array(out, VIS_DTYPES, (nrow, nchan), dev, "out")
    params = _lib.GridderParams()
    call(dev, "cip_dirty2ms", uvw, nrow, freq, nchan, dirty, int(dirty.shape[0]), int(dirty.shape[1]),
         float(pixsize_x), float(pixsize_y), float(epsilon), int(support or 0),
         (_lib.CIP_WSTACKING if do_wstacking else 0)
         | (_lib.CIP_SUBTRACT if subtract else 0)
         | (_lib.CIP_REUSE_PLAN if reuse_plan else 0),
         *wgt_args, STREAM, *vis_arg(out), params)
    return out, params


def dirty2ms(  # pylint: disable=too-many-arguments,unused-argument
    uvw,
    freq,
    dirty,
    wgt=None,
    pixsize_x: float = None,
    pixsize_y: float = None,
    nu: int = 0,
    nv: int = 0,
    epsilon: float = 1e-4,
    do_wstacking: bool = False,
    nthreads: int = 1,
    verbosity: int = 0,
    mask=None,
    *,
    support: Optional[int] = None,
    device=None,
    return_params: bool = False,
):
    """
    Drop-in for `ducc0.wgridder.dirty2ms` (same positional order). `nu`, `nv`,
    `nthreads` and `verbosity` are accepted for signature compatibility and
    ignored, as in `ms2dirty`. `mask` (uint8, shape of the visibilities)
    zeroes the weights where 0. numpy in -> numpy out, torch in -> torch out.
    Output dtype follows ducc: complex64 for a float32 `dirty`, else
    complex128; the arithmetic is fp64 either way.
    """
    require_gpu()
    if pixsize_x is None or pixsize_y is None:
        raise TypeError("pixsize_x and pixsize_y are required")
    dev = target_device(device)
    numpy_in = isinstance(dirty, np.ndarray)
    single = dirty.dtype in (np.float32, torch.float32)
    with torch.cuda.device(dev):
        uvw_d, freq_d, wgt_d = _stage(uvw, freq, wgt, mask, dev)
        dirty_d = to_device(dirty, torch.float64, dev)
        vis, params = device_dirty2ms(
            uvw_d, freq_d, dirty_d, wgt_d, float(pixsize_x), float(pixsize_y), epsilon=epsilon,
            support=support, do_wstacking=do_wstacking,
            out_dtype=torch.complex64 if single else torch.complex128)
        result = vis.cpu().numpy() if numpy_in else vis
    if return_params:
        return result, params
    return result
