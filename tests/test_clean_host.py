"""
Host-side checks of the CLEAN interface (no GPU): the built library exports
`cip_hogbom_clean`, the header declares it and its stop codes, the result
struct has the C layout, the Python entry points exist and refuse to run
without a GPU, and the numpy statement of the algorithm (`_clean_np`, the GPU
tests' reference) does what include/cip.h says on hand-checkable cases.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _clean_np
from ska_sdp_cip_amd import _lib

HEADER = (Path(__file__).resolve().parents[1] / "include" / "cip.h").read_text()


def test_library_exports_cip_hogbom_clean():
    so = _lib.lib()
    assert "cip_hogbom_clean" in _lib.EXPORTED_SYMBOLS
    assert hasattr(so, "cip_hogbom_clean")
    # one argtype per parameter of the header's prototype (18: residual_io, nx,
    # ny, psf, psf_nx, psf_ny, psf_cx, psf_cy, mask, gain, threshold, niter,
    # batch, hip_stream, model_io, comp_index, comp_flux, result_out)
    proto = re.search(r"^int cip_hogbom_clean\((.*?)\);", HEADER, flags=re.M | re.S).group(1)
    assert len(proto.split(",")) == 18
    assert len(so.cip_hogbom_clean.argtypes) == 18
    assert so.cip_hogbom_clean.restype is ctypes.c_int


def test_header_declares_the_entry_point_and_stop_codes():
    assert "int cip_hogbom_clean(" in HEADER
    assert "typedef struct cip_clean_result" in HEADER
    for name, value in (("CIP_CLEAN_NITER", 0), ("CIP_CLEAN_THRESHOLD", 1), ("CIP_CLEAN_EMPTY", 2)):
        assert f"#define {name} {value}" in HEADER
        assert getattr(_lib, name) == value
    assert (_clean_np.NITER, _clean_np.THRESHOLD, _clean_np.EMPTY) == (0, 1, 2)


def test_result_struct_layout():
    assert ctypes.sizeof(_lib.CleanResult) == 32
    assert [(n, getattr(_lib.CleanResult, n).offset) for n, _ in _lib.CleanResult._fields_] == [
        ("niter_done", 0), ("stop_reason", 8), ("reserved", 12), ("peak", 16), ("peak_index", 24)]


def test_entry_points_need_a_gpu():
    import torch

    import ska_sdp_cip_amd as pkg
    from ska_sdp_cip_amd import deconvolve

    assert pkg.hogbom_clean is deconvolve.hogbom_clean
    assert pkg.device_hogbom_clean is deconvolve.device_hogbom_clean
    assert pkg.device_major_cycles is deconvolve.device_major_cycles
    if torch.cuda.is_available():
        return  # the refusal shows only without a GPU
    img, psf = np.zeros((8, 8)), np.ones((3, 3))
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        deconvolve.hogbom_clean(img, psf)
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        deconvolve.device_hogbom_clean(torch.zeros((8, 8), dtype=torch.float64),
                                       torch.ones((3, 3), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        deconvolve.device_major_cycles(torch.zeros((2, 3)), torch.ones(1), torch.zeros((2, 1), dtype=torch.complex128),
                                       None, 8, 1e-4, n_major=1, niter=1)


# ---- the numpy reference on hand-checkable cases ---------------------------

def test_reference_delta_image_delta_psf_empties_in_one_iteration():
    img = np.zeros((5, 7))
    img[2, 3] = 4.0
    model, res, info = _clean_np.hogbom_clean(img, np.ones((1, 1)), gain=1.0, niter=10)
    assert not res.any()
    assert model[2, 3] == 4.0 and np.count_nonzero(model) == 1
    assert info["niter_done"] == 1 and info["stop_reason"] == _clean_np.THRESHOLD  # a zero peak is <= 0
    assert info["comp_index"].tolist() == [2 * 7 + 3] and info["comp_flux"].tolist() == [4.0]
    assert info["peak"] == 0.0 and info["peak_index"] == 0
    assert img[2, 3] == 4.0  # the input is not modified


def test_reference_ties_go_to_the_lower_flat_index():
    img = np.zeros((4, 4))
    img[3, 0] = img[1, 2] = 2.0
    _, _, info = _clean_np.hogbom_clean(img, np.ones((1, 1)), gain=0.5, niter=1)
    assert info["comp_index"].tolist() == [1 * 4 + 2]
    img[1, 2] = -2.0  # |.| ties too
    _, _, info = _clean_np.hogbom_clean(img, np.ones((1, 1)), gain=0.5, niter=1)
    assert info["comp_index"].tolist() == [1 * 4 + 2] and info["comp_flux"].tolist() == [-1.0]


def test_reference_negative_peak_gives_a_negative_component():
    img = np.zeros((3, 3))
    img[1, 1], img[0, 2] = -5.0, 3.0
    model, res, info = _clean_np.hogbom_clean(img, np.ones((1, 1)), gain=0.1, niter=1)
    assert info["comp_flux"].tolist() == [0.1 * -5.0] and model[1, 1] == 0.1 * -5.0
    assert res[1, 1] == -5.0 - (0.1 * -5.0)
    assert info["stop_reason"] == _clean_np.NITER and info["peak"] == res[1, 1] and info["peak_index"] == 4


def test_reference_window_clips_at_both_corners():
    psf = np.arange(1.0, 10.0).reshape(3, 3)  # centre (1, 1) holds 5
    img = np.zeros((4, 5))
    img[0, 0] = 1.0
    _, res, _ = _clean_np.hogbom_clean(img, psf, gain=1.0, niter=1)
    want = np.zeros((4, 5))
    want[0, 0] = 1.0
    want[0:2, 0:2] -= psf[1:3, 1:3]
    assert np.array_equal(res, want)
    img = np.zeros((4, 5))
    img[3, 4] = 1.0
    _, res, _ = _clean_np.hogbom_clean(img, psf, gain=1.0, niter=1)
    want = np.zeros((4, 5))
    want[3, 4] = 1.0
    want[2:4, 3:5] -= psf[0:2, 0:2]
    assert np.array_equal(res, want)


def test_reference_mask_nan_and_stop_order():
    img = np.array([[1.0, np.nan], [3.0, -2.0]])
    one = np.ones((1, 1))
    # the NaN is never chosen; the mask keeps (1, 0) out but it is still subtracted from
    _, res, info = _clean_np.hogbom_clean(img, np.full((3, 3), 0.5), gain=1.0, niter=1,
                                          mask=np.array([[1, 1], [0, 1]], dtype=np.uint8))
    assert info["comp_index"].tolist() == [3]
    assert res[1, 0] == 3.0 - (-2.0 * 0.5) and np.isnan(res[0, 1])
    # no allowed pixel: EMPTY before anything else, nothing changed
    _, res, info = _clean_np.hogbom_clean(img, one, niter=5, mask=np.zeros((2, 2), dtype=np.uint8))
    assert info["stop_reason"] == _clean_np.EMPTY and info["peak_index"] == -1 and info["peak"] == 0.0
    assert np.array_equal(res, img, equal_nan=True)
    # threshold is checked before the iteration cap, with <=
    _, _, info = _clean_np.hogbom_clean(img, one, threshold=3.0, niter=0)
    assert info["stop_reason"] == _clean_np.THRESHOLD and info["peak"] == 3.0 and info["peak_index"] == 2
    _, _, info = _clean_np.hogbom_clean(img, one, threshold=2.5, niter=0)
    assert info["stop_reason"] == _clean_np.NITER and info["niter_done"] == 0
