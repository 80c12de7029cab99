"""
Predict: model visibilities of an image, and the major cycle's residual
`vis - dirty2ms(model)`, on the GPU (`cip_dirty2ms`, the exact transpose of
the invert's `cip_ms2dirty`). Argument style of `invert.ducc_invert`.
"""

from __future__ import annotations

from typing import Optional

from ._call import require_gpu
from .gridder import device_dirty2ms, dirty2ms
from .invert import DO_WSTACKING, EPSILON, pixel_size_lm


def ducc_predict(
    uvw,
    freq,
    image,
    pixel_size_asec: float,
    *,
    epsilon: float = EPSILON,
    do_wstacking: bool = DO_WSTACKING,
    support: Optional[int] = None,
):
    """
    Unweighted model visibilities (nrow, nchan) of `image` (num_pixels,
    num_pixels) with pixels of `pixel_size_asec` arcseconds, at the
    baselines `uvw` (nrow, 3) metres and `freq` (nchan) Hz: the call of
    `ducc0.wgridder.dirty2ms` that pairs with `ducc_invert`'s `ms2dirty`
    (same epsilon and w-stacking defaults). numpy in -> numpy out, torch in
    -> torch out; complex64 for a float32 image, else complex128.
    """
    pix = pixel_size_lm(pixel_size_asec)
    return dirty2ms(uvw, freq, image, None, pix, pix, epsilon=epsilon, do_wstacking=do_wstacking, support=support)


def device_residual(
    uvw,
    freq,
    vis,
    model_image,
    pixsize: float,
    wgt=None,
    *,
    epsilon: float = EPSILON,
    do_wstacking: bool = DO_WSTACKING,
    support: Optional[int] = None,
    inplace: bool = False,
    reuse_plan: bool = False,
):
    """
    The major cycle's residual `vis - wgt * dirty2ms(model_image)` on
    device-resident tensors (pixel size `pixsize` in radians, both axes),
    formed in the degridder's epilogue without a model column
    (CIP_SUBTRACT). Returns a new tensor, or `vis` itself updated in place
    with `inplace=True`. `wgt=None`: plain `vis - model`.
    """
    require_gpu()
    out = vis if inplace else vis.clone()
    device_dirty2ms(uvw, freq, model_image, wgt, pixsize, pixsize, epsilon=epsilon, support=support,
                    do_wstacking=do_wstacking, out=out, subtract=True, reuse_plan=reuse_plan)
    return out
