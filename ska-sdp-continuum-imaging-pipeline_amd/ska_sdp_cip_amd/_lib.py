"""
ctypes binding of libcip_hip.so (C ABI: include/cip.h, include/cip_restore.h,
include/cip_mfs.h, include/cip_cal.h, include/cip_dft.h, include/cip_ms.h,
include/cip_noise.h and include/cip_mosaic.h).

The library is the product: there is no CPU fallback. `lib()` raises when the
shared object is missing or cannot be loaded, and every call maps a negative
status to a Python exception carrying `cip_last_error()`:
CIP_EINVAL / CIP_ERANGE -> ValueError, CIP_EHIP -> RuntimeError,
CIP_ENOMEM -> MemoryError.
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "_lib" / "libcip_hip.so"

CIP_OK = 0
CIP_EINVAL = -1
CIP_ERANGE = -2
CIP_EHIP = -3
CIP_ENOMEM = -4

CIP_NONE = 0
CIP_C64 = 1
CIP_C128 = 2
CIP_F32 = 3
CIP_F64 = 4
CIP_WSTACKING = 1
CIP_ACC_SINGLE = 2
CIP_PSF = 4
CIP_NORMALISE = 8
CIP_ASYNC = 16
CIP_PIPELINE = 32
CIP_REUSE_PLAN = 64
CIP_GRID_ZEROED = 128
CIP_SUBTRACT = 256
CIP_CLEAN_NITER = 0
CIP_CLEAN_THRESHOLD = 1
CIP_CLEAN_EMPTY = 2
CIP_CLEAN_DEFAULT_BATCH = 64
CIP_WEIGHT_NATURAL = 0
CIP_WEIGHT_UNIFORM = 1
CIP_WEIGHT_BRIGGS = 2
WEIGHTING_MODES = {"natural": CIP_WEIGHT_NATURAL, "uniform": CIP_WEIGHT_UNIFORM, "briggs": CIP_WEIGHT_BRIGGS}
CLEAN_STOP_REASONS = {CIP_CLEAN_NITER: "niter", CIP_CLEAN_THRESHOLD: "threshold", CIP_CLEAN_EMPTY: "empty"}
STOKES_CODES = {"I": 0, "Q": 1, "U": 2, "V": 3}

PROFILE_PHASES = ("prep", "plan", "scatter", "fft", "correct", "total")
PROFILE_COUNTS = ("visibilities", "runs", "chunks", "planes", "scatter_launches", "reserved")


class GridderParams(ctypes.Structure):
    """Mirror of `cip_gridder_params` (include/cip.h)."""

    _fields_ = [
        ("nu", ctypes.c_int64),
        ("nv", ctypes.c_int64),
        ("support", ctypes.c_int32),
        ("degree", ctypes.c_int32),
        ("beta", ctypes.c_double),
        ("sigma", ctypes.c_double),
        ("do_wstacking", ctypes.c_int32),
        ("tile", ctypes.c_int32),
        ("nplanes", ctypes.c_int64),
        ("w0", ctypes.c_double),
        ("dw", ctypes.c_double),
        ("nmin", ctypes.c_double),
    ]

    def as_dict(self) -> dict:
        """Plain-dict view (for result files)."""
        return {name: getattr(self, name) for name, _ in self._fields_}


class CleanResult(ctypes.Structure):
    """Mirror of `cip_clean_result` (include/cip.h)."""

    _fields_ = [
        ("niter_done", ctypes.c_int64),
        ("stop_reason", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("peak", ctypes.c_double),
        ("peak_index", ctypes.c_int64),
    ]


class WeightGrid(ctypes.Structure):
    """Mirror of `cip_weight_grid` (include/cip.h)."""

    _fields_ = [
        ("npix_x", ctypes.c_int64),
        ("npix_y", ctypes.c_int64),
        ("pixsize_x", ctypes.c_double),
        ("pixsize_y", ctypes.c_double),
        ("SX", ctypes.c_double),
        ("SY", ctypes.c_double),
        ("wmax", ctypes.c_double),
        ("quantum", ctypes.c_double),
        ("shift", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]

    @property
    def density_shape(self) -> tuple:
        """Shape of the grid's int64 density array: (2 hx + 1, hy + 1)."""
        return (2 * (self.npix_x // 2) + 1, self.npix_y // 2 + 1)


class WeightInfo(ctypes.Structure):
    """Mirror of `cip_weight_info` (include/cip.h)."""

    _fields_ = [
        ("sum_w", ctypes.c_double),
        ("sum_d2", ctypes.c_double),
        ("f2", ctypes.c_double),
        ("quantum", ctypes.c_double),
        ("n_added", ctypes.c_int64),
        ("n_outside", ctypes.c_int64),
        ("n_cells", ctypes.c_int64),
    ]

    def as_dict(self) -> dict:
        """Plain-dict view."""
        return {name: getattr(self, name) for name, _ in self._fields_}


class Beam(ctypes.Structure):
    """Mirror of `cip_beam` (include/cip_restore.h)."""

    _fields_ = [
        ("a", ctypes.c_double),
        ("b", ctypes.c_double),
        ("c", ctypes.c_double),
        ("fwhm_major", ctypes.c_double),
        ("fwhm_minor", ctypes.c_double),
        ("pa", ctypes.c_double),
        ("n_fit", ctypes.c_int64),
    ]

    def as_dict(self) -> dict:
        """Plain-dict view."""
        return {name: getattr(self, name) for name, _ in self._fields_}


# CIP_RESTORE_MAX_RADIUS, CIP_BEAM_FIT_RADIUS and CIP_BEAM_FIT_CUT of include/cip_restore.h
RESTORE_MAX_RADIUS = 32
BEAM_FIT_RADIUS = 8
BEAM_FIT_CUT = 0.35

_LIB = None

_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_i32 = ctypes.c_int
_f64 = ctypes.c_double
_str = ctypes.c_char_p
_prm = ctypes.POINTER(GridderParams)
_wgrid = ctypes.POINTER(WeightGrid)
_pi64 = ctypes.POINTER(ctypes.c_int64)
_pf64 = ctypes.POINTER(ctypes.c_double)
_ROWS = [_vp, _i64, _vp, _i64]  # uvw, nrow, freq, nchan
_VIS_WGT = [_vp, _i32, _vp, _i32]  # vis, vis_dtype, wgt, wgt_dtype
_IMAGE = [_i64, _i64, _f64, _f64]  # npix_x, npix_y, pixsize_x, pixsize_y
_SLICES = [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _i32]  # cip_grid_tiles' slices .. wgt_dtype
_STRIP = [_vp, _prm, _i64, _i64]  # a buffer, params, npix_x, npix_y

# The prototype of every symbol declared in include/cip.h, in its order:
# name -> (restype, argtypes). A new entry point is one line here.
PROTOTYPES = {
    "cip_choose_params": (_i32, [*_IMAGE, _f64, _i32, _i32, _f64, _f64, _prm]),
    "cip_ms2dirty": (_i32, [*_ROWS, *_VIS_WGT, *_IMAGE, _f64, _i32, _i32, _vp, _vp, _vp, _prm]),
    "cip_dirty2ms": (_i32, [*_ROWS, _vp, *_IMAGE, _f64, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _prm]),
    "cip_hogbom_clean": (_i32, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _f64, _f64, _i64, _i64, _vp,
                                _vp, _vp, _vp, ctypes.POINTER(CleanResult)]),
    "cip_weight_grid_init": (_i32, [*_IMAGE, _f64, _i64, _wgrid]),
    "cip_weight_density": (_i32, [*_ROWS, _vp, _i32, _wgrid, _vp, _vp, _pi64]),
    "cip_weight_stats": (_i32, [_vp, _wgrid, _vp, _pf64]),
    "cip_weight_apply": (_i32, [*_ROWS, _vp, _i32, _vp, _wgrid, _i32, _f64, _vp, _vp, _i32]),
    "cip_imaging_weights": (_i32, [*_ROWS, _vp, _i32, *_IMAGE, _i32, _f64, _vp, _vp, _i32,
                                   ctypes.POINTER(WeightInfo)]),
    "cip_ms2dirty_wplanes": (_i32, [*_ROWS, *_VIS_WGT, *_IMAGE, _f64, _i32, _i32, _i64, _i64, _vp, _vp, _vp, _prm]),
    "cip_ms2dirty_stokes_i": (_i32, [*_ROWS, _vp, _vp, _vp, *_IMAGE, _f64, _i32, _i32, _vp, _vp, _vp, _prm]),
    "cip_grid_plane": (_i32, [*_ROWS, *_VIS_WGT, _prm, _f64, _f64, _i64, _i32, _vp, _vp]),
    "cip_grid_layout": (_i32, [_prm, _i64, _i64]),
    "cip_plane_group": (_i32, [_prm, _i32]),
    "cip_grid_ms": (_i32, [*_ROWS, *_VIS_WGT, _prm, _f64, _f64, _i64, _i64, _i32, _vp, _vp, _vp]),
    "cip_grid_ms_stokes_i": (_i32, [*_ROWS, _vp, _vp, _vp, _prm, _f64, _f64, _i64, _i64, _i32, _vp, _vp, _vp]),
    "cip_grid_tiles": (_i32, [*_SLICES, _prm, _f64, _f64, _i64, _i64, _i32, _vp, _vp, _vp]),
    "cip_grid_tiles_strip": (_i32, [*_SLICES, _prm, _f64, _f64, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp]),
    "cip_grid_tiles_strip_mask": (_i32, [*_SLICES, _prm, _f64, _f64, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp,
                                         _vp]),
    "cip_strip_histogram": (_i32, [*_ROWS, _prm, _f64, _f64, _vp, _vp]),
    "cip_strip_split": (_i32, [*_ROWS, *_VIS_WGT, _prm, _f64, _i64, _i64, _vp, _pi64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cip_grid_to_dirty": (_i32, [*_STRIP, _f64, _f64, _vp, _vp]),
    "cip_strip_rows": (_i32, [*_STRIP, _i64, _i64, _vp, _vp]),
    "cip_strip_cols": (_i32, [*_STRIP, _i64, _i64, _vp, _vp, _vp]),
    "cip_strip_rows_masked": (_i32, [*_STRIP, _i64, _i64, _i64, _vp, _vp, _vp]),
    "cip_strip_rows_packed": (_i32, [*_STRIP, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
    "cip_strip_pack_rows": (_i32, [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp]),
    "cip_strip_unpack_rows": (_i32, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "cip_strip_cols_wplane": (_i32, [*_STRIP, _f64, _f64, _i64, _i64, _i64, _i32, _vp, _vp]),
    "cip_strip_wfinal": (_i32, [*_STRIP, _f64, _f64, _i64, _i64, _vp, _vp]),
    "cip_tile_runs": (_i32, [*_ROWS, _pf64, _i64, _vp, _pi64, _vp, _vp, _vp, _vp]),
    "cip_stokes_i": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "cip_stokes": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "cip_facet_rephase": (_i32, [*_ROWS, _vp, _i32, _f64, _f64, _vp, _vp, _vp]),
    "cip_allreduce_grid": (_i32, [_vp, _vp, _i32, _i64, _i32, _vp]),
    "cip_release_collectives": (_i32, []),
    "cip_last_error": (_str, []),
    "cip_release_workspace": (_i32, []),
    "cip_profile_enable": (_i32, [_i32]),
    "cip_profile_last": (_i32, [_vp, _vp]),
    "cip_build_info": (_str, []),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

# The same for include/cip_restore.h, the second header of the C ABI.
_beam = ctypes.POINTER(Beam)
RESTORE_PROTOTYPES = {
    "cip_beam_from_fwhm": (_i32, [_f64, _f64, _f64, _beam]),
    "cip_beam_fit_window": (_i32, [_pf64, _i64, _f64, _beam]),
    "cip_beam_fit": (_i32, [_vp, _i64, _i64, _i64, _i64, _f64, _i64, _vp, _beam]),
    "cip_beam_radius": (_i32, [_beam, _f64]),
    "cip_beam_taps": (_i32, [_beam, _i64, _pf64]),
    "cip_restore": (_i32, [_vp, _vp, _i64, _i64, _beam, _i64, _vp, _vp]),
}

# And for include/cip_mfs.h, the third (hinv is a HOST array).
MFS_MAX_TERMS = 3  # CIP_MFS_MAX_TERMS
MFS_PROTOTYPES = {
    "cip_mfs_clean": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _pf64, _vp, _f64, _f64, _i64, _i64,
                             _vp, _vp, _vp, _vp, ctypes.POINTER(CleanResult)]),
}


class CalScale(ctypes.Structure):
    """Mirror of `cip_cal_scale` (include/cip_cal.h)."""

    _fields_ = [
        ("n_ant", ctypes.c_int64),
        ("n_int", ctypes.c_int64),
        ("amax", ctypes.c_double),
        ("wmax", ctypes.c_double),
        ("quantum", ctypes.c_double),
        ("shift", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]

    @property
    def corr_shape(self) -> tuple:
        """Shape of the int64 correlation array: (n_int, n_ant, n_ant, 3)."""
        return (self.n_int, self.n_ant, self.n_ant, 3)


class CalCounts(ctypes.Structure):
    """Mirror of `cip_cal_counts` (include/cip_cal.h)."""

    _fields_ = [(name, ctypes.c_int64) for name in ("n_added", "n_zero", "n_outside", "n_bad")]

    def as_dict(self) -> dict:
        """Plain-dict view."""
        return {name: getattr(self, name) for name, _ in self._fields_}


class CalSolveInfo(ctypes.Structure):
    """Mirror of `cip_cal_solve_info` (include/cip_cal.h)."""

    _fields_ = [
        ("n_converged", ctypes.c_int64),
        ("n_dead", ctypes.c_int64),
        ("max_iter_done", ctypes.c_int64),
        ("ref_missing", ctypes.c_int64),
        ("max_change", ctypes.c_double),
    ]

    def as_dict(self) -> dict:
        """Plain-dict view."""
        return {name: getattr(self, name) for name, _ in self._fields_}


# And for include/cip_cal.h, the fourth (the structs are HOST memory).
# (named without the CIP_ prefix, which is kept for the codes of cip.h)
CAL_MAX_ANT = 1024  # CIP_CAL_MAX_ANT
CAL_CORRECT = 0  # CIP_CAL_CORRECT
CAL_CORRUPT = 1  # CIP_CAL_CORRUPT
CAL_PHASE_ONLY = 1  # CIP_CAL_PHASE_ONLY (a flag)
CAL_MODES = {"correct": CAL_CORRECT, "corrupt": CAL_CORRUPT}
_scale = ctypes.POINTER(CalScale)
_counts = ctypes.POINTER(CalCounts)
_sinfo = ctypes.POINTER(CalSolveInfo)
_CAL_COLS = [_vp, _i32, _vp, _i32, _vp, _i32, _i64, _i64, _vp, _vp, _vp]  # vis .. wgt_dtype, nrow, nchan, ant1 ..
CAL_PROTOTYPES = {
    "cip_cal_scale_init": (_i32, [_i64, _i64, _f64, _f64, _i64, _scale]),
    "cip_cal_correlate": (_i32, [*_CAL_COLS, _scale, _vp, _vp, _counts]),
    "cip_cal_solve": (_i32, [_vp, _scale, _i64, _f64, _i64, _i32, _vp, _vp, _vp, _vp, _sinfo]),
    "cip_cal_apply": (_i32, [_vp, _i32, _vp, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp,
                             _vp]),
    "cip_gaincal": (_i32, [*_CAL_COLS, _i64, _i64, _i64, _f64, _i64, _i32, _vp, _vp, _vp, _vp, _scale, _counts,
                           _sinfo]),
}

# And for include/cip_dft.h, the fifth: the flags are a namespace of their own.
DFT_ADD = 1  # CIP_DFT_ADD
DFT_SUBTRACT = 2  # CIP_DFT_SUBTRACT
DFT_WTERM = 4  # CIP_DFT_WTERM
DFT_FAST = 8  # CIP_DFT_FAST
DFT_MODES = {"set": 0, "add": DFT_ADD, "subtract": DFT_SUBTRACT}
DFT_PROTOTYPES = {
    "cip_dft_predict": (_i32, [*_ROWS, _vp, _vp, _vp, _i64, _i64, _f64, _i32, _vp, _i32, _vp, _vp, _i32]),
}


class MsResult(ctypes.Structure):
    """Mirror of `cip_ms_result` (include/cip_ms.h)."""

    _fields_ = [
        ("niter_done", ctypes.c_int64),
        ("stop_reason", ctypes.c_int32),
        ("peak_scale", ctypes.c_int32),
        ("peak", ctypes.c_double),
        ("peak_index", ctypes.c_int64),
    ]


# And for include/cip_ms.h, the sixth (taps, select_weight and flux_scale are HOST arrays).
MS_MAX_SCALES = 6  # CIP_MS_MAX_SCALES
MS_MAX_RADIUS = 128  # CIP_MS_MAX_RADIUS
MS_PROTOTYPES = {
    "cip_ms_scale_radius": (_i32, [_f64, _f64]),
    "cip_ms_scale_taps": (_i32, [_f64, _i64, _pf64]),
    "cip_ms_convolve": (_i32, [_vp, _i64, _i64, _pf64, _i64, _vp, _vp]),
    "cip_ms_clean": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _pf64, _pf64, _vp, _f64, _f64, _i64,
                            _i64, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(MsResult)]),
}


class NoiseResult(ctypes.Structure):
    """Mirror of `cip_noise_result` (include/cip_noise.h)."""

    _fields_ = [
        ("count", ctypes.c_int64),
        ("median", ctypes.c_double),
        ("mad", ctypes.c_double),
        ("sigma", ctypes.c_double),
    ]

    def as_dict(self) -> dict:
        """Plain-dict view."""
        return {name: getattr(self, name) for name, _ in self._fields_}


class MaskResult(ctypes.Structure):
    """Mirror of `cip_mask_result` (include/cip_noise.h)."""

    _fields_ = [(name, ctypes.c_int64) for name in ("n_seed", "n_island", "n_out", "rounds")]

    def as_dict(self) -> dict:
        """Plain-dict view."""
        return {name: getattr(self, name) for name, _ in self._fields_}


# And for include/cip_noise.h, the seventh (the results and the two scalars of the select are HOST memory).
MAD_TO_SIGMA = 1.482602218505602  # CIP_MAD_TO_SIGMA
MASK_POSITIVE = 1  # CIP_MASK_POSITIVE
MASK_CONN4 = 2  # CIP_MASK_CONN4
NOISE_PROTOTYPES = {
    "cip_image_select": (_i32, [_vp, _i64, _i64, _vp, _i64, _vp, _pi64, _pf64]),
    "cip_image_noise": (_i32, [_vp, _i64, _i64, _vp, _vp, ctypes.POINTER(NoiseResult)]),
    "cip_auto_mask": (_i32, [_vp, _i64, _i64, _f64, _f64, _vp, _vp, _i32, _vp, _vp, ctypes.POINTER(MaskResult)]),
}


class MosaicGeom(ctypes.Structure):
    """Mirror of `cip_mosaic_geom` (include/cip_mosaic.h)."""

    _fields_ = [
        ("nx", ctypes.c_int64),
        ("ny", ctypes.c_int64),
        ("px", ctypes.c_double),
        ("py", ctypes.c_double),
        ("fnx", ctypes.c_int64),
        ("fny", ctypes.c_int64),
        ("fpx", ctypes.c_double),
        ("fpy", ctypes.c_double),
        ("half", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("beta", ctypes.c_double),
        ("trim", ctypes.c_int64),
        ("feather", ctypes.c_double),
    ]

    def as_dict(self) -> dict:
        """Plain-dict view."""
        return {name: getattr(self, name) for name, _ in self._fields_}


# And for include/cip_mosaic.h, the eighth (the geometry, beta_out, taps_out and n_uncovered_out are HOST memory).
MOSAIC_MAX_HALF = 8  # CIP_MOSAIC_MAX_HALF
MOSAIC_NSCALE = 1  # CIP_MOSAIC_NSCALE
MOSAIC_PROTOTYPES = {
    "cip_mosaic_beta": (_i32, [_i32, _f64, _pf64]),
    "cip_mosaic_taps": (_i32, [_i32, _f64, _f64, _pf64]),
    "cip_mosaic_add": (_i32, [ctypes.POINTER(MosaicGeom), _vp, _i64, _f64, _f64, _vp, _vp, _vp]),
    "cip_mosaic_finish": (_i32, [_vp, _vp, _i64, _i64, _i64, _f64, _vp, _pi64]),
}


def lib() -> ctypes.CDLL:
    """Load (once) and return the HIP library; raises if it is unavailable."""
    global _LIB  # pylint: disable=global-statement
    if _LIB is not None:
        return _LIB
    path = Path(os.environ.get("CIP_HIP_LIB", LIB_PATH))
    if not path.exists():
        raise RuntimeError(
            f"libcip_hip.so not found at {path}; build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C ska-sdp-continuum-imaging-pipeline_amd/csrc)"
        )
    so = ctypes.CDLL(str(path))
    for name, (restype, argtypes) in (*PROTOTYPES.items(), *RESTORE_PROTOTYPES.items(), *MFS_PROTOTYPES.items(),
                                      *CAL_PROTOTYPES.items(), *DFT_PROTOTYPES.items(), *MS_PROTOTYPES.items(),
                                      *NOISE_PROTOTYPES.items(), *MOSAIC_PROTOTYPES.items()):
        fn = getattr(so, name)
        fn.restype, fn.argtypes = restype, argtypes
    _LIB = so
    return so


def check(rc: int) -> None:
    """Raise the Python exception matching a CIP status code."""
    if rc == CIP_OK:
        return
    msg = lib().cip_last_error().decode(errors="replace")
    if rc in (CIP_EINVAL, CIP_ERANGE):
        raise ValueError(msg)
    if rc == CIP_ENOMEM:
        raise MemoryError(msg)
    raise RuntimeError(f"libcip_hip error {rc}: {msg}")


def choose_params(npix_x: int, npix_y: int, pixsize_x: float, pixsize_y: float,
                  epsilon: float, support: int = 0, do_wstacking: bool = False,
                  wmin: float = 0.0, wmax: float = 0.0) -> GridderParams:
    """Host-only parameter choice (no GPU needed)."""
    out = GridderParams()
    check(lib().cip_choose_params(int(npix_x), int(npix_y), float(pixsize_x), float(pixsize_y),
                                  float(epsilon), int(support or 0), int(bool(do_wstacking)),
                                  float(wmin), float(wmax), ctypes.byref(out)))
    return out


def weight_grid(npix_x: int, npix_y: int, pixsize_x: float, pixsize_y: float, wmax: float,
                nvis_max: int) -> WeightGrid:
    """The weighting grid and fixed-point scale of `cip_weight_grid_init` (host-only)."""
    out = WeightGrid()
    check(lib().cip_weight_grid_init(int(npix_x), int(npix_y), float(pixsize_x), float(pixsize_y), float(wmax),
                                     int(nvis_max), ctypes.byref(out)))
    return out


def cal_scale(n_ant: int, n_int: int, amax: float, wmax: float, nsamp_max: int) -> CalScale:
    """The fixed-point scale of `cip_cal_scale_init` (host-only)."""
    out = CalScale()
    check(lib().cip_cal_scale_init(int(n_ant), int(n_int), float(amax), float(wmax), int(nsamp_max),
                                   ctypes.byref(out)))
    return out


def plane_group(params: GridderParams, packed: bool = False) -> int:
    """w planes one w-stacking scatter pass grids together (host-only)."""
    g = int(lib().cip_plane_group(ctypes.byref(params), int(bool(packed))))
    if g < 0:
        check(g)
    return g


def profile_enable(on: bool = True) -> None:
    """Record per-phase hipEvents in subsequent calls on this thread."""
    check(lib().cip_profile_enable(int(bool(on))))


def profile_last() -> dict:
    """Per-phase milliseconds and counters of the last call on this thread."""
    import numpy as np  # pylint: disable=import-outside-toplevel

    ms = np.zeros(len(PROFILE_PHASES), dtype=np.float64)
    counts = np.zeros(len(PROFILE_COUNTS), dtype=np.int64)
    check(lib().cip_profile_last(ms.ctypes.data, counts.ctypes.data))
    out = {f"{k}_ms": float(v) for k, v in zip(PROFILE_PHASES, ms)}
    out.update({k: int(v) for k, v in zip(PROFILE_COUNTS, counts)})
    return out
