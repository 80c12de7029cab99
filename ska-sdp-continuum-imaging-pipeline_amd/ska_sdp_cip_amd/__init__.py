"""
ska_sdp_cip_amd - MI355X-native invert hot path of ska_sdp_cip.

Public API mirrors `/root/reference/src/ska_sdp_cip/__init__.py:1-10`
(`MeasurementSetReader`, `invert_measurement_set`,
`dask_invert_measurement_set`, `__version__`) plus the drop-in gridder
`ms2dirty` (replaces `ducc0.wgridder.ms2dirty`), its adjoint `dirty2ms`
(`ducc0.wgridder.dirty2ms`; `predict.py` wraps it), the minor and major cycle
built on the two (`deconvolve.py`: Hogbom CLEAN, `cip_hogbom_clean`), the
clean beam and the restored image (`restore.py`, `cip_beam_fit`,
`cip_restore`), uniform and Briggs imaging weights (`weighting.py`,
`cip_imaging_weights`), multi-term multi-frequency synthesis (`mfs.py`,
`cip_mfs_clean`), multiscale CLEAN (`multiscale.py`, `cip_ms_convolve`,
`cip_ms_clean`), antenna gain self-calibration (`calibrate.py`, `cip_gaincal`), the sky-model
predict (`skymodel.py`, `cip_dft_predict`), the image noise and the island
mask behind the major cycles' `auto_threshold` and `auto_mask` (`noise.py`,
`cip_image_noise`, `cip_auto_mask`), facet mosaicking onto one wide-field
plane (`mosaic.py`, `cip_mosaic_add`) and the `uvw_tiling` package.
"""

__version__ = "0.1.0"

from .gridder import dirty2ms, ms2dirty  # noqa: E402
from .invert import (  # noqa: E402
    StokesIGridderInput,
    dask_invert_measurement_set,
    ducc_invert,
    integrate_weighted_images,
    invert_measurement_set,
)
from .predict import device_residual, ducc_predict  # noqa: E402
from . import noise  # noqa: E402
from .noise import (  # noqa: E402
    MAD_TO_SIGMA,
    auto_mask,
    device_auto_mask,
    device_image_noise,
    device_image_select,
    image_noise,
)
from .deconvolve import device_hogbom_clean, device_major_cycles, hogbom_clean  # noqa: E402
# `restore.restore` (numpy in -> numpy out) stays in its module: exported here
# it would hide the module of the same name
from .restore import beam_from_fwhm, beam_taps, beam_to_sky, device_fit_beam, device_restore  # noqa: E402
from .weighting import WeightDensity, device_imaging_weights, imaging_weights  # noqa: E402
from . import mfs  # noqa: E402
from .mfs import (  # noqa: E402
    device_mfs_clean,
    device_mfs_invert,
    device_mfs_major_cycles,
    device_mfs_residual,
    mfs_clean,
    mfs_hessian,
    taylor_basis,
)
from . import multiscale  # noqa: E402
from .multiscale import (  # noqa: E402
    device_cross_psfs,
    device_ms_clean,
    device_ms_convolve,
    device_ms_major_cycles,
    device_ms_model,
    device_scale_residuals,
    ms_clean,
    scale_radius,
    scale_taps,
    scale_weights,
)
from . import calibrate  # noqa: E402
from .calibrate import (  # noqa: E402
    GainCorrelator,
    device_gain_apply,
    device_gain_correlate,
    device_gain_solve,
    device_gaincal,
    device_selfcal,
    gain_apply,
    gaincal,
    solution_intervals,
)
from . import skymodel  # noqa: E402
from .skymodel import SkyModel, device_dft_predict, dft_predict  # noqa: E402
from . import mosaic  # noqa: E402
from .mosaic import MosaicAccumulator, device_mosaic, facet_layout, mosaic_beta, mosaic_taps  # noqa: E402
from .measurement_set import (  # noqa: E402
    InMemoryMeasurementSet,
    MeasurementSetReader,
    UnsupportedMeasurementSetLayout,
)

# Load libcip_hip.so at import, on the importing thread, when it is built: the
# library records the thread that loads it as the main thread (whose workspaces
# are left to process teardown, cip_workspace.hip), so the first call from a worker
# thread must not be the one that loads it. A missing library raises at the
# first call instead (no CPU fallback).
try:
    from . import _lib as _cip_lib

    if _cip_lib.LIB_PATH.exists():
        _cip_lib.lib()
except OSError:  # pragma: no cover - a broken build raises again at first use
    pass

__all__ = [
    "__version__",
    "MeasurementSetReader",
    "InMemoryMeasurementSet",
    "UnsupportedMeasurementSetLayout",
    "StokesIGridderInput",
    "dask_invert_measurement_set",
    "ducc_invert",
    "integrate_weighted_images",
    "invert_measurement_set",
    "ms2dirty",
    "dirty2ms",
    "ducc_predict",
    "device_residual",
    "hogbom_clean",
    "device_hogbom_clean",
    "device_major_cycles",
    "imaging_weights",
    "device_imaging_weights",
    "WeightDensity",
    "device_restore",
    "device_fit_beam",
    "beam_from_fwhm",
    "beam_taps",
    "beam_to_sky",
    "mfs",
    "taylor_basis",
    "mfs_hessian",
    "mfs_clean",
    "device_mfs_clean",
    "device_mfs_invert",
    "device_mfs_residual",
    "device_mfs_major_cycles",
    "multiscale",
    "scale_radius",
    "scale_taps",
    "scale_weights",
    "ms_clean",
    "device_ms_convolve",
    "device_scale_residuals",
    "device_cross_psfs",
    "device_ms_clean",
    "device_ms_model",
    "device_ms_major_cycles",
    "calibrate",
    "solution_intervals",
    "GainCorrelator",
    "device_gain_correlate",
    "device_gain_solve",
    "device_gain_apply",
    "device_gaincal",
    "device_selfcal",
    "gaincal",
    "gain_apply",
    "skymodel",
    "SkyModel",
    "device_dft_predict",
    "dft_predict",
    "noise",
    "MAD_TO_SIGMA",
    "device_image_select",
    "device_image_noise",
    "device_auto_mask",
    "image_noise",
    "auto_mask",
    "mosaic",
    "MosaicAccumulator",
    "device_mosaic",
    "facet_layout",
    "mosaic_beta",
    "mosaic_taps",
]
