"""
Host-side checks of the imaging-weights interface (no GPU): the numpy
statement of the operator (`_weights_np`, the GPU tests' yardstick) does what
include/cip.h says on hand-checkable cases, `cip_weight_grid_init` (host-only)
gives the fixed-point shift of the definition and refuses bad arguments, the
structs have the C layout and the header states the definition.
"""

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

import _weights_np as wnp
from ska_sdp_cip_amd import _lib

HEADER = (Path(__file__).resolve().parents[1] / "include" / "cip.h").read_text()
C = 299792458.0


def _grid(npix_x=8, npix_y=6, wmax=1.0, nvis_max=16):
    # SX = SY = 1: x = u f / c, y = v f / c, so with freq = c the uv are the cell coordinates
    return wnp.Grid(npix_x, npix_y, 1.0 / npix_x, 1.0 / npix_y, wmax, nvis_max)


# ---- the numpy statement on hand-checkable cases ----------------------------

def test_reference_one_visibility():
    g = _grid()
    assert g.shape == (9, 4) and (g.hx, g.hy) == (4, 3) and g.SX == 1.0 and g.SY == 1.0
    uvw = np.array([[2.0, 1.0, 0.0]])
    dens, counts = wnp.density(uvw, [C], np.array([[0.75]], dtype=np.float32), g)
    assert counts.tolist() == [1, 0, 0]
    assert np.count_nonzero(dens) == 1 and dens[2 + 4, 1] == int(0.75 * 2.0 ** g.shift)
    sum_w, sum_d2, n_cells = wnp.stats(dens, g)
    assert (sum_w, sum_d2, n_cells) == (0.75, 0.75 * 0.75, 1)
    # uniform: w / D = 1; Briggs with f2 = 4: 0.75 / (1 + 0.75 * 4)
    assert wnp.apply(uvw, [C], np.array([[0.75]]), dens, g, wnp.UNIFORM, 0.0, np.float64)[0, 0] == 1.0
    assert wnp.apply(uvw, [C], np.array([[0.75]]), dens, g, wnp.BRIGGS, 4.0, np.float64)[0, 0] == 0.75 / 4.0


def test_reference_conjugate_pair_lands_in_one_cell():
    g = _grid()
    uvw = np.array([[2.0, 1.0, 0.0], [-2.0, -1.0, 5.0]])
    iu, iv, inside = wnp.cells(uvw, [C], g)
    assert inside.all() and iu.ravel().tolist() == [2, 2] and iv.ravel().tolist() == [1, 1]
    dens, counts = wnp.density(uvw, [C], None, g)
    assert counts.tolist() == [2, 0, 0] and dens[6, 1] == 2 << g.shift and np.count_nonzero(dens) == 1
    out = wnp.apply(uvw, [C], None, dens, g, wnp.UNIFORM, 0.0, np.float32)
    assert out.dtype == np.float32 and out.ravel().tolist() == [0.5, 0.5]


def test_reference_fold_on_the_u_axis():
    # y == 0 and x < 0 folds to +x; y == 0, x > 0 stays
    g = _grid()
    iu, iv, inside = wnp.cells(np.array([[-3.0, 0.0, 0.0], [3.0, 0.0, 0.0], [-3.0, -0.0, 0.0]]), [C], g)
    assert inside.all() and iu.ravel().tolist() == [3, 3, 3] and iv.ravel().tolist() == [0, 0, 0]
    # y > 0 keeps a negative x
    iu, iv, _ = wnp.cells(np.array([[-3.0, 1.0, 0.0]]), [C], g)
    assert (iu[0, 0], iv[0, 0]) == (-3, 1)


def test_reference_half_cell_boundaries_round_up():
    # floor(x + 0.5): n + 0.5 goes to n + 1, -(n + 0.5) to -n
    g = _grid()
    iu, iv, inside = wnp.cells(np.array([[1.5, 0.5, 0.0], [-1.5, 2.5, 0.0], [-2.5, -0.5, 0.0]]), [C], g)
    assert inside.all()
    assert iu.ravel().tolist() == [2, -1, 3]  # the last one is folded: x = 2.5 -> 3
    assert iv.ravel().tolist() == [1, 3, 1]


def test_reference_grid_edge():
    g = _grid()  # hx = 4, hy = 3
    uvw = np.array([[4.0, 0.0, 0.0], [-4.0, 3.0, 0.0], [4.25, 3.25, 0.0],  # |iu| = hx, iv = hy: inside
                    [4.5, 0.0, 0.0], [0.0, 3.5, 0.0], [-4.75, 1.0, 0.0],    # just outside
                    [np.inf, 0.0, 0.0], [np.nan, 1.0, 0.0]])
    _, _, inside = wnp.cells(uvw, [C], g)
    assert inside.ravel().tolist() == [True, True, True, False, False, False, False, False]
    w = np.ones((8, 1), dtype=np.float32)
    dens, counts = wnp.density(uvw, [C], w, g)
    assert counts.tolist() == [3, 5, 0]
    assert dens[8, 0] == dens[0, 3] == dens[8, 3] == 1 << g.shift
    out = wnp.apply(uvw, [C], w, dens, g, wnp.BRIGGS, 1.0, np.float64)
    assert out.ravel().tolist() == [0.5, 0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0]


def test_reference_zero_and_bad_weights_and_rounding():
    g = _grid(wmax=2.0, nvis_max=4)
    uvw = np.zeros((1, 3))
    w = np.array([[0.0, -1.0, np.nan, 2.5, 2.0]])
    dens, counts = wnp.density(uvw, [C] * 5, w, g)
    assert counts.tolist() == [1, 0, 3] and dens[4, 0] == 2 << g.shift
    # round-half-even of w 2^shift: shift = 62 - 2 - 1 = 59
    assert g.shift == 59
    tiny = np.array([0.5, 1.5, 2.5]) * 2.0 ** -59
    assert wnp.quantise(tiny, g).tolist() == [0, 2, 2]


# ---- cip_weight_grid_init (host-only) ---------------------------------------

@pytest.mark.parametrize("wmax, nvis_max, shift", [
    (1.0, 1, 62),              # B = 0, E = 0
    (1.0, 2, 61),
    (1.0, 3, 60),              # B = 2
    (1.0, 1 << 20, 42),        # an exact power of two: B = 20
    ((1 << 20) + 1, 1 << 20, 21),  # E = 21
    (0.5, 1024, 53),           # E = -1
    (0.75, 1025, 51),          # E = 0, B = 11
    (4.0, 100_000_000, 33),    # B = 27, E = 2
    (2.0 ** -140, 7, 199),     # a tiny float32 bound
    (3.0e38, 1 << 40, -106),   # E = 128
])
def test_grid_init_shift(wmax, nvis_max, shift):
    assert wnp.grid_shift(wmax, nvis_max) == shift
    g = _lib.weight_grid(64, 48, 1e-4, 2e-4, wmax, nvis_max)
    assert g.shift == shift and g.quantum == math.ldexp(1.0, -shift) and g.wmax == wmax
    assert (g.npix_x, g.npix_y, g.pixsize_x, g.pixsize_y) == (64, 48, 1e-4, 2e-4)
    assert g.SX == 64 * 1e-4 and g.SY == 48 * 2e-4 and g.density_shape == (65, 25)
    # no sum of nvis_max weights <= wmax reaches 2^62
    assert nvis_max * int(np.rint(np.ldexp(np.float64(wmax), shift))) <= 1 << 62


def test_grid_init_odd_npix_shape():
    assert _lib.weight_grid(33, 17, 1e-3, 1e-3, 1.0, 10).density_shape == (33, 9)
    assert wnp.Grid(33, 17, 1e-3, 1e-3, 1.0, 10).shape == (33, 9)


@pytest.mark.parametrize("args", [
    (64, 64, 1e-4, 1e-4, 0.0, 10), (64, 64, 1e-4, 1e-4, -1.0, 10), (64, 64, 1e-4, 1e-4, math.inf, 10),
    (64, 64, 1e-4, 1e-4, math.nan, 10),
    (64, 64, 1e-4, 1e-4, 1.0, 0), (64, 64, 1e-4, 1e-4, 1.0, -5),
    (0, 64, 1e-4, 1e-4, 1.0, 10), (64, 0, 1e-4, 1e-4, 1.0, 10), (-3, 64, 1e-4, 1e-4, 1.0, 10),
    (64, 64, 0.0, 1e-4, 1.0, 10), (64, 64, 1e-4, -1e-4, 1.0, 10), (64, 64, math.nan, 1e-4, 1.0, 10),
    (64, 64, 1e-4, math.inf, 1.0, 10),
])
def test_grid_init_einval(args):
    out = _lib.WeightGrid()
    assert _lib.lib().cip_weight_grid_init(*args, ctypes.byref(out)) == _lib.CIP_EINVAL
    assert b"cip_weight_grid_init" in _lib.lib().cip_last_error()
    with pytest.raises(ValueError, match="cip_weight_grid_init"):
        _lib.weight_grid(*args)


def test_argument_checks_come_before_the_device():
    # refused on their arguments alone, so these run without a GPU
    L = _lib.lib()
    g = _lib.weight_grid(8, 8, 1e-3, 1e-3, 1.0, 8)
    stats = (ctypes.c_double * 3)()
    assert L.cip_weight_stats(None, ctypes.byref(g), None, stats) == _lib.CIP_EINVAL
    assert L.cip_weight_density(None, -1, None, 4, None, _lib.CIP_NONE, ctypes.byref(g), None, None, None) \
        == _lib.CIP_EINVAL
    assert L.cip_weight_density(None, 0, None, 70000, None, _lib.CIP_NONE, ctypes.byref(g), None, None, None) \
        == _lib.CIP_EINVAL
    assert L.cip_weight_density(None, 0, None, 4, None, _lib.CIP_NONE, None, None, None, None) == _lib.CIP_EINVAL
    blank = _lib.WeightGrid()  # never initialised
    assert L.cip_weight_density(None, 0, None, 4, None, _lib.CIP_NONE, ctypes.byref(blank), None, None, None) \
        == _lib.CIP_EINVAL
    assert L.cip_weight_apply(None, 0, None, 4, None, _lib.CIP_NONE, None, ctypes.byref(g), 7, 0.0, None, None,
                              _lib.CIP_F32) == _lib.CIP_EINVAL
    assert L.cip_weight_apply(None, 0, None, 4, None, _lib.CIP_NONE, None, ctypes.byref(g), _lib.CIP_WEIGHT_BRIGGS,
                              0.0, None, None, _lib.CIP_C64) == _lib.CIP_EINVAL
    assert L.cip_imaging_weights(None, 0, None, 4, None, _lib.CIP_NONE, 8, 8, 1e-3, 1e-3, _lib.CIP_WEIGHT_BRIGGS,
                                 math.nan, None, None, _lib.CIP_F32, None) == _lib.CIP_EINVAL
    assert b"robust" in L.cip_last_error()
    # nrow == 0 is a no-op that needs no device
    counts = (ctypes.c_int64 * 3)(9, 9, 9)
    assert L.cip_weight_density(None, 0, None, 4, None, _lib.CIP_NONE, ctypes.byref(g), None, None, counts) \
        == _lib.CIP_OK
    assert list(counts) == [0, 0, 0]
    info = _lib.WeightInfo()
    assert L.cip_imaging_weights(None, 0, None, 4, None, _lib.CIP_NONE, 8, 8, 1e-3, 1e-3, _lib.CIP_WEIGHT_UNIFORM,
                                 0.0, None, None, _lib.CIP_F32, ctypes.byref(info)) == _lib.CIP_OK
    assert (info.sum_w, info.n_added, info.n_cells) == (0.0, 0, 0)


# ---- the interface -----------------------------------------------------------

def test_library_exports_the_entry_points():
    so = _lib.lib()
    for name, nargs in (("cip_weight_grid_init", 7), ("cip_weight_density", 10), ("cip_weight_stats", 4),
                        ("cip_weight_apply", 13), ("cip_imaging_weights", 16)):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(so, name)
        proto = re.search(rf"^int {name}\((.*?)\);", HEADER, flags=re.M | re.S).group(1)
        assert len(proto.split(",")) == nargs, name
        assert len(getattr(so, name).argtypes) == nargs, name
        assert getattr(so, name).restype is ctypes.c_int


def test_struct_layouts():
    assert ctypes.sizeof(_lib.WeightGrid) == 72
    assert [(n, getattr(_lib.WeightGrid, n).offset) for n, _ in _lib.WeightGrid._fields_] == [
        ("npix_x", 0), ("npix_y", 8), ("pixsize_x", 16), ("pixsize_y", 24), ("SX", 32), ("SY", 40), ("wmax", 48),
        ("quantum", 56), ("shift", 64), ("reserved", 68)]
    assert ctypes.sizeof(_lib.WeightInfo) == 56
    assert [n for n, _ in _lib.WeightInfo._fields_] == ["sum_w", "sum_d2", "f2", "quantum", "n_added", "n_outside",
                                                        "n_cells"]
    for field in [n for n, _ in _lib.WeightGrid._fields_ if n != "reserved"] + [n for n, _ in _lib.WeightInfo._fields_]:
        assert re.search(rf"\b{field}\b", HEADER), field


def test_header_states_the_definition():
    for name, value in (("CIP_WEIGHT_NATURAL", 0), ("CIP_WEIGHT_UNIFORM", 1), ("CIP_WEIGHT_BRIGGS", 2)):
        assert f"#define {name} {value}" in HEADER
        assert getattr(_lib, name) == value
    assert (wnp.UNIFORM, wnp.BRIGGS) == (_lib.CIP_WEIGHT_UNIFORM, _lib.CIP_WEIGHT_BRIGGS)
    flat = " ".join(HEADER.replace("*", " ").split())
    for phrase in (
        "(2 hx + 1, hy + 1)",
        "cell (iu, iv) stored at [iu + hx][iv]",
        "wi = freq[c] / 299792458.0",
        "if (y < 0 || (y == 0 && x < 0)) { x = -x; y = -y; }",
        "iu = floor(x + 0.5) iv = floor(y + 0.5)",
        "|iu| <= hx and iv <= hy",
        "shift = 62 - B - E",
        "q(w) = llrint(ldexp((double)w, shift))",
        "64-bit integer atomic adds",
        "No floating-point atomics",
        "D > 0 ? w64 / D : 0",
        "w64 / (1.0 + D f2)",
        "f2 = (t t) / (sum_d2 / sum_w)",
    ):
        assert phrase in flat, phrase


def test_python_entry_points():
    import torch

    import ska_sdp_cip_amd as pkg
    from ska_sdp_cip_amd import weighting

    assert pkg.imaging_weights is weighting.imaging_weights
    assert pkg.device_imaging_weights is weighting.device_imaging_weights
    assert pkg.WeightDensity is weighting.WeightDensity
    # natural weighting: the weights themselves, no library call, no GPU
    w = np.ones((2, 3), dtype=np.float32)
    out, info = weighting.imaging_weights(np.zeros((2, 3)), np.ones(3), w, 8, 8, 1e-3, 1e-3, weighting="natural")
    assert out is w and info == {}
    with pytest.raises(ValueError, match="weighting must be one of"):
        weighting.imaging_weights(np.zeros((2, 3)), np.ones(3), w, 8, 8, 1e-3, 1e-3, weighting="superuniform")
    assert weighting.briggs_f2(0.5, 3.0, 7.0) == wnp.briggs_f2(0.5, 3.0, 7.0)
    if torch.cuda.is_available():
        return  # the refusal shows only without a GPU
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        weighting.imaging_weights(np.zeros((2, 3)), np.ones(3), w, 8, 8, 1e-3, 1e-3)
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        weighting.WeightDensity(8, 8, 1e-3, 1e-3, 1.0, 6, "cpu")
