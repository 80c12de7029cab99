"""
Host-side checks of facet mosaicking (no GPU): include/cip_mosaic.h against
`_lib.MOSAIC_PROTOTYPES` and `_lib.MosaicGeom` (the method of
test_noise_host.py on the eighth header), the closed form of the rotation
against `oracle.facet_rotation`, the host-only entry points cip_mosaic_beta and
cip_mosaic_taps against the numpy statement `_mosaic_np`, every argument check
that needs no device, `facet_layout`'s coverage, and the method's error on the
scene of `_mosaic_scene`: the numpy statement over the oracle's w-stacked
facets against the direct DFT of the whole field.

Measured on that scene (max |mosaic - DFT| over the weight sum): 5.4e-4 at
half = 3, 3.6e-5 at 4, 5.1e-7 at 6, 2.7e-9 at 8; 3.0e-3 at 6 without n' / n.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _mosaic_np as mnp
import _mosaic_scene as sc
import oracle
from ska_sdp_cip_amd import _lib, mosaic
from ska_sdp_cip_amd.mosaic import MosaicAccumulator, device_mosaic, facet_layout, mosaic_beta, mosaic_taps

HEADER = Path(__file__).resolve().parents[1] / "include" / "cip_mosaic.h"
SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "double": ctypes.c_double}
HOST_POINTERS = {"beta_out": ctypes.POINTER(ctypes.c_double), "taps_out": ctypes.POINTER(ctypes.c_double),
                 "n_uncovered_out": ctypes.POINTER(ctypes.c_int64)}
NAMES = ("cip_mosaic_beta", "cip_mosaic_taps", "cip_mosaic_add", "cip_mosaic_finish")


@pytest.fixture(scope="module")
def header():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


# ---- header against table ----------------------------------------------------
def test_every_prototype_matches_the_table(header):
    protos = {}
    for ret, name, params in re.findall(r"\b(int|const\s+char\s*\*)\s*(cip_\w+)\s*\(([^)]*)\)\s*;", header):
        protos[name] = (ret, [" ".join(p.split()) for p in params.split(",")])
    assert tuple(protos) == tuple(_lib.MOSAIC_PROTOTYPES) == NAMES
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.MOSAIC_PROTOTYPES[name]
        assert ret == "int" and restype is ctypes.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            if "*" in decl:
                base = decl.replace("const", " ").split("*")[0].strip()
                if base == "cip_mosaic_geom":
                    assert argtype is ctypes.POINTER(_lib.MosaicGeom), (name, k, decl)
                elif decl.split()[-1] in HOST_POINTERS:
                    assert argtype is HOST_POINTERS[decl.split()[-1]], (name, k, decl)
                else:
                    assert argtype is ctypes.c_void_p, (name, k, decl)
            else:
                assert argtype is SCALARS[decl.replace("const", " ").split()[0]], (name, k, decl)
    defines = dict(re.findall(r"#define\s+(CIP_\w+)\s+([0-9.]+)", header))
    assert int(defines["CIP_MOSAIC_MAX_HALF"]) == _lib.MOSAIC_MAX_HALF == mosaic.MAX_HALF == 8
    assert int(defines["CIP_MOSAIC_NSCALE"]) == _lib.MOSAIC_NSCALE == mnp.NSCALE == 1
    assert '#include "cip.h"' in header


def test_geometry_struct_matches_the_mirror(header):
    structs = dict(re.findall(r"typedef\s+struct\s+(cip_\w+)\s*\{(.*?)\}\s*\1\s*;", header, flags=re.S))
    assert tuple(structs) == ("cip_mosaic_geom",)
    fields = [(m[1], SCALARS[m[0]]) for m in re.findall(r"(\w+)\s+(\w+)\s*;", structs["cip_mosaic_geom"])]
    assert fields == list(_lib.MosaicGeom._fields_)
    assert ctypes.sizeof(_lib.MosaicGeom) == 96
    assert [f for f, _ in fields] == ["nx", "ny", "px", "py", "fnx", "fny", "fpx", "fpy", "half", "flags", "beta",
                                     "trim", "feather"]


def test_library_exports_and_other_tables_unchanged():
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in _lib.MOSAIC_PROTOTYPES:
        assert hasattr(so, name), name
        for table in (_lib.PROTOTYPES, _lib.RESTORE_PROTOTYPES, _lib.MFS_PROTOTYPES, _lib.CAL_PROTOTYPES,
                      _lib.DFT_PROTOTYPES, _lib.MS_PROTOTYPES, _lib.NOISE_PROTOTYPES):
            assert name not in table
    loaded = _lib.lib()  # lib() applies all eight tables
    for name, (restype, argtypes) in _lib.MOSAIC_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---- the definition ------------------------------------------------------------
@pytest.mark.parametrize("centre", [(0.0, 0.0), (0.3, 0.0), (0.0, -0.45), (0.5, 0.1), (-0.082, 0.077), (0.6, -0.7)])
def test_rotation_closed_form_is_the_oracles(centre):
    qt = mnp.rotation_t(*centre)
    assert np.abs(qt - oracle.facet_rotation(*centre).T).max() <= 1e-15
    assert np.abs(qt @ qt.T - np.eye(3)).max() <= 1e-15


def test_beta_rule():
    for half in range(2, 9):
        for nu in (0.0, 0.125, 0.25, 0.49):
            assert mosaic_beta(half, nu) == pytest.approx(np.pi * half * (1.0 - 2.0 * nu), rel=1e-15)
            assert mosaic_beta(half, nu) == pytest.approx(mnp.beta_rule(half, nu), rel=1e-15)
    assert mosaic_beta(6, 0.0) == pytest.approx(6 * np.pi, rel=1e-15)


@pytest.mark.parametrize("half", range(2, 9))
def test_taps_sum_to_one_and_are_a_delta_at_zero(half):
    beta = mosaic_beta(half, 0.125)
    delta = np.zeros(2 * half)
    delta[half - 1] = 1.0  # k = 0
    assert np.array_equal(mosaic_taps(half, beta, 0.0), delta)
    assert np.array_equal(mnp.taps(half, beta, 0.0), delta)
    fracs = np.concatenate([np.random.default_rng(half).uniform(size=200), [0.5, 1e-300, 1e-17, 1.0 - 2.0**-53]])
    ref = mnp.taps(half, beta, fracs)
    for f, r in zip(fracs, ref):
        t = mosaic_taps(half, beta, float(f))
        assert abs(t.sum() - 1.0) <= 4 * np.spacing(1.0), (f, t.sum())
        # the C taps and the numpy statement differ by the two libraries' exp and sin
        assert np.abs(t - r).max() <= 1e-15, (f, np.abs(t - r).max())
    # the taps are those of the kernel: symmetric about the sample point
    assert np.allclose(mosaic_taps(half, beta, 0.25), mosaic_taps(half, beta, 0.75)[::-1], rtol=0, atol=1e-15)
    # beta = 0 is the bare sinc, cut off at +-half
    bare = mosaic_taps(half, 0.0, 0.5)
    k = np.arange(-half + 1, half + 1)
    assert np.allclose(bare, np.sinc(0.5 - k) / np.sinc(0.5 - k).sum(), rtol=0, atol=1e-15)


# ---- argument checks: all before any device work -------------------------------
FAKE, OTHER, THIRD = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)  # never dereferenced
BIG = 1 << 62


def test_beta_and_taps_argument_checks():
    so = _lib.lib()
    out = ctypes.c_double(-7.0)
    taps = (ctypes.c_double * 16)()
    for args in ((1, 0.1, ctypes.byref(out)), (9, 0.1, ctypes.byref(out)), (6, -0.1, ctypes.byref(out)),
                 (6, 0.5, ctypes.byref(out)), (6, float("nan"), ctypes.byref(out)), (6, 0.1, None)):
        assert so.cip_mosaic_beta(*args) == _lib.CIP_EINVAL, args
        assert b"cip_mosaic_beta" in so.cip_last_error(), args
    assert out.value == -7.0
    for args in ((1, 1.0, 0.5, taps), (9, 1.0, 0.5, taps), (6, -1.0, 0.5, taps), (6, float("inf"), 0.5, taps),
                 (6, 1.0, 1.0, taps), (6, 1.0, -0.1, taps), (6, 1.0, float("nan"), taps), (6, 1.0, 0.5, None)):
        assert so.cip_mosaic_taps(*args) == _lib.CIP_EINVAL, args
        assert b"cip_mosaic_taps" in so.cip_last_error(), args
    for fn, args in ((mosaic_beta, (6, 0.5)), (mosaic_beta, (1, 0.1)), (mosaic_taps, (6, 1.0, 1.0)),
                     (mosaic_taps, (0, 1.0, 0.5)), (mosaic_taps, (6, -1.0, 0.5))):
        with pytest.raises(ValueError, match="cip_mosaic_"):
            fn(*args)


def _geom(**kw):
    base = dict(nx=64, ny=48, px=2e-3, py=2.3e-3, fnx=40, fny=36, fpx=1.6e-3, fpy=1.6e-3, half=6, flags=0, beta=10.0,
                trim=0, feather=0.0)
    base.update(kw)
    return _lib.MosaicGeom(**base)


ADD_REFUSED = [dict(nx=0), dict(ny=-1), dict(fnx=0), dict(fny=0), dict(nx=BIG, ny=4), dict(fnx=BIG), dict(px=0.0),
               dict(py=-1e-3), dict(fpx=float("nan")), dict(fpy=float("inf")), dict(half=1), dict(half=9),
               dict(beta=-1.0), dict(beta=float("nan")), dict(trim=-1), dict(feather=-0.5),
               dict(feather=float("inf")), dict(flags=2), dict(flags=-1), dict(px=0.03, py=0.03),  # a corner at 1.2
               dict(fnx=11), dict(fny=11), dict(trim=13), dict(fnx=24, trim=7, half=6), dict(trim=BIG)]


@pytest.mark.parametrize("kw", ADD_REFUSED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_add_geometry_checks_come_before_the_device(kw):
    so = _lib.lib()
    assert so.cip_mosaic_add(ctypes.byref(_geom(**kw)), FAKE, 1, 0.01, 0.02, None, OTHER, THIRD) == _lib.CIP_EINVAL
    assert b"cip_mosaic_add" in so.cip_last_error()


def test_add_and_finish_argument_checks_come_before_the_device():
    so = _lib.lib()
    g = ctypes.byref(_geom())

    def add(geom=g, facet=FAKE, nplane=1, l0=0.01, m0=0.02, num=OTHER, wsum=THIRD):
        return so.cip_mosaic_add(geom, facet, nplane, l0, m0, None, num, wsum)

    for kw in (dict(geom=None), dict(facet=None), dict(num=None), dict(wsum=None), dict(nplane=0), dict(nplane=BIG),
               dict(l0=0.8, m0=0.6), dict(l0=1.5), dict(m0=float("nan")), dict(l0=float("inf"))):
        assert add(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_mosaic_add" in so.cip_last_error(), kw
    missed = ctypes.c_int64(-7)

    def finish(num=FAKE, wsum=OTHER, nplane=1, nx=8, ny=8, out=ctypes.byref(missed)):
        return so.cip_mosaic_finish(num, wsum, nplane, nx, ny, float("nan"), None, out)

    for kw in (dict(num=None), dict(wsum=None), dict(out=None), dict(nplane=0), dict(nx=0), dict(ny=-3),
               dict(nx=BIG, ny=4), dict(nx=1 << 31, ny=1 << 31, nplane=4)):
        assert finish(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_mosaic_finish" in so.cip_last_error(), kw
    assert missed.value == -7


ACC_REFUSED = [dict(nx=0), dict(ny=-2), dict(nx=6.5), dict(px=0.0), dict(py=float("nan")), dict(nplane=0),
               dict(half=1), dict(half=9), dict(half=6.5), dict(trim=-1), dict(trim=1.5), dict(feather=-1.0),
               dict(feather=float("nan")), dict(nu_max=0.5), dict(nu_max=-0.1), dict(nu_max=None),
               dict(beta=3.0), dict(nu_max=None, beta=-1.0), dict(nu_max=None, beta=float("inf")),
               dict(px=0.03, py=0.03)]


@pytest.mark.parametrize("kw", ACC_REFUSED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_python_arguments_are_validated_without_a_gpu(kw):
    # `nu_max=None` alone gives neither nu_max nor beta, `beta=3.0` alone both
    args = dict(nx=64, ny=48, px=2e-3, py=2.3e-3, nplane=1, half=6, nu_max=0.125, trim=0, feather=0.0)
    args.update(kw)
    with pytest.raises(ValueError):
        MosaicAccumulator(**args)


def test_layout_and_one_shot_arguments_are_validated_without_a_gpu():
    for kw in (dict(nx=0), dict(px=-1.0), dict(facet_pixels=11), dict(facet_pixels=20, trim=5), dict(half=9),
               dict(trim=-1), dict(px=0.03), dict(facet_pixel_size=0.0), dict(py=float("nan"))):
        args = dict(nx=64, ny=48, px=2e-3, facet_pixels=40)
        args.update(kw)
        with pytest.raises(ValueError):
            facet_layout(**args)
    with pytest.raises(ValueError, match="one centre per facet"):
        device_mosaic([], [], 64, 48, 2e-3, nu_max=0.1)
    with pytest.raises(ValueError, match="one centre per facet"):
        device_mosaic([np.zeros((4, 4))], [(0.0, 0.0), (0.1, 0.1)], 64, 48, 2e-3, nu_max=0.1)


# ---- layout --------------------------------------------------------------------
@pytest.mark.parametrize("width", [0.05, 0.3, 0.6])
@pytest.mark.parametrize("shape,facet,half,trim", [((96, 80), 48, 6, 0), ((75, 130), 40, 8, 3), ((64, 64), 64, 2, 0)])
def test_facet_layout_leaves_no_pixel_uncovered(width, shape, facet, half, trim):
    nx, ny = shape
    py = width / max(nx, ny)
    px = py / 1.1
    cen = facet_layout(nx, ny, px, facet, half=half, trim=trim, py=py, facet_pixel_size=0.9 * px)
    assert all(isinstance(v, float) for c in cen for v in c)
    g = mnp.Geom(nx, ny, px, py, facet, facet, 0.9 * px, 0.9 * px, half, 1.0, trim, 0.0)
    wsum = np.zeros((nx, ny))
    for c in cen:
        x, y, q2, _ = mnp.coords(g, *c)
        wsum += mnp.weight(g, x, y, q2)
    assert int((wsum <= 0).sum()) == 0, (len(cen), int((wsum <= 0).sum()))
    # the smallest regular grid: no fewer facets than the valid spans allow
    span = (facet - 2 * (trim + half)) * 0.9 + 1  # output pixels of px a facet's valid region spans at the centre
    fewest = int(np.ceil(nx / span)) * int(np.ceil(ny * 1.1 / span))
    print(f"{len(cen)} facets, at least {fewest}")
    assert fewest <= len(cen) <= (int(np.ceil(nx / span)) + 1) * (int(np.ceil(ny * 1.1 / span)) + 1)


# ---- the method ----------------------------------------------------------------
def test_method_error_on_the_scene():
    """The numpy statement over oracle.ms2dirty facets against
    oracle.dft_dirty(apply_w=True): exponential convergence in `half`, orders
    of magnitude below a short Lanczos (8.9e-4 at a = 6), and n' / n needed."""
    assert len(sc.centres(6)) == 4
    err = {}
    for half in (4, 6, 8):
        err[half], missed = sc.method_error(half)
        assert missed == 0
    plain, _ = sc.method_error(6, nscale=False)
    print("max |mosaic - DFT| / sum w:", {k: f"{v:.2e}" for k, v in err.items()}, f"without n'/n at 6: {plain:.2e}")
    assert err[8] < err[6] < err[4]
    assert err[6] < 1e-5
    assert plain > err[6]
