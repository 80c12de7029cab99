"""
Host-side checks of multiscale CLEAN (no GPU): include/cip_ms.h against
`_lib.MS_PROTOTYPES` and `_lib.MsResult` (the method of test_mfs_host.py on the
sixth header), every argument check of the four entry points through the
shared object, the scale taps and the radius rule against the numpy formula,
and the numpy statement `_ms_np` itself: against `_clean_np` where the two
operators coincide (S = 1, both host arrays [1.0]), the packed index, and a
planted blob that one scale-2 component removes.
"""
import ctypes
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest

import _clean_np
import _ms_np
from ska_sdp_cip_amd import _lib, multiscale

HEADER = Path(__file__).resolve().parents[1] / "include" / "cip_ms.h"
SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "double": ctypes.c_double}
PF64 = ctypes.POINTER(ctypes.c_double)
HOST_ARRAYS = {"taps", "taps_out", "select_weight", "flux_scale"}


@pytest.fixture(scope="module")
def header():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


# ---- header against table ----------------------------------------------------
def test_every_prototype_matches_the_table(header):
    protos = {}
    for ret, name, params in re.findall(r"\b(int|const\s+char\s*\*)\s*(cip_\w+)\s*\(([^)]*)\)\s*;", header):
        protos[name] = (ret, [" ".join(p.split()) for p in params.split(",")])
    assert tuple(protos) == tuple(_lib.MS_PROTOTYPES) == ("cip_ms_scale_radius", "cip_ms_scale_taps",
                                                          "cip_ms_convolve", "cip_ms_clean")
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.MS_PROTOTYPES[name]
        assert ret == "int" and restype is ctypes.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            if "*" in decl:
                base = decl.replace("const", " ").split("*")[0].strip()
                if base == "cip_ms_result":
                    assert argtype is ctypes.POINTER(_lib.MsResult), (name, k, decl)
                elif decl.split()[-1] in HOST_ARRAYS:
                    assert base == "double" and argtype is PF64, (name, k, decl)
                else:
                    assert argtype is ctypes.c_void_p, (name, k, decl)
            else:
                assert argtype is SCALARS[decl.replace("const", " ").split()[0]], (name, k, decl)
    defines = dict(re.findall(r"#define\s+(CIP_\w+)\s+(\d+)", header))
    assert int(defines["CIP_MS_MAX_SCALES"]) == _lib.MS_MAX_SCALES == 6
    assert int(defines["CIP_MS_MAX_RADIUS"]) == _lib.MS_MAX_RADIUS == 128
    assert '#include "cip.h"' in header


def test_result_struct_matches_the_mirror(header):
    structs = dict(re.findall(r"typedef\s+struct\s+(cip_\w+)\s*\{(.*?)\}\s*\1\s*;", header, flags=re.S))
    assert tuple(structs) == ("cip_ms_result",)
    fields = [(m[1], SCALARS[m[0]]) for m in re.findall(r"(\w+)\s+(\w+)\s*;", structs["cip_ms_result"])]
    assert fields == list(_lib.MsResult._fields_)
    assert ctypes.sizeof(_lib.MsResult) == 32 == ctypes.sizeof(_lib.CleanResult)


def test_library_exports_and_other_tables_unchanged():
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in _lib.MS_PROTOTYPES:
        assert hasattr(so, name), name
        for table in (_lib.PROTOTYPES, _lib.RESTORE_PROTOTYPES, _lib.MFS_PROTOTYPES, _lib.CAL_PROTOTYPES,
                      _lib.DFT_PROTOTYPES):
            assert name not in table
    assert len(_lib.PROTOTYPES) == 41 and len(_lib.RESTORE_PROTOTYPES) == 6 and len(_lib.MFS_PROTOTYPES) == 1
    loaded = _lib.lib()  # lib() applies all six tables
    for name, (restype, argtypes) in _lib.MS_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---- argument checks: all before a launch -------------------------------------
def _arr(*values):
    return (ctypes.c_double * len(values))(*values)


def test_clean_argument_checks_come_before_the_device():
    so = _lib.lib()
    out = _lib.MsResult()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)  # never dereferenced: every call below is refused
    good = _arr(1.0, 0.5, 0.25, 0.1, 0.1, 0.1)

    def call(res=fake, nscales=2, nx=8, ny=8, psf=other, px=5, py=5, cx=-1, cy=-1, sw=good, fs=good, gain=0.1,
             threshold=0.0, niter=4, batch=0, ci=None, cs=None, cf=None):
        return so.cip_ms_clean(res, nscales, nx, ny, psf, px, py, cx, cy, sw, fs, None, gain, threshold, niter, batch,
                               None, None, ci, cs, cf, ctypes.byref(out))

    nan, inf = _arr(1.0, float("nan")), _arr(float("inf"), 1.0)
    big = 1 << 31
    for kw in (dict(nscales=0), dict(nscales=7), dict(nscales=-1), dict(sw=None), dict(fs=None), dict(sw=nan),
               dict(fs=nan), dict(sw=inf), dict(fs=inf),
               # some but not all of the three component arrays
               dict(ci=fake), dict(cs=fake), dict(cf=fake), dict(ci=fake, cf=fake), dict(ci=fake, cs=fake),
               dict(cs=fake, cf=fake),
               # everything cip_hogbom_clean refuses
               dict(res=None), dict(psf=None), dict(nx=0), dict(ny=-1), dict(px=0), dict(py=-3), dict(cx=5),
               dict(cy=-2), dict(gain=0.0), dict(gain=-0.1), dict(gain=float("nan")), dict(gain=float("inf")),
               dict(threshold=-1.0), dict(threshold=float("nan")), dict(niter=-1), dict(batch=-1),
               # S nx ny, and the PSF stack, beyond int64
               dict(nscales=6, nx=big * big // 4, ny=4), dict(nscales=6, px=big * big // 16, py=4, cx=0, cy=0)):
        assert call(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_ms_clean" in so.cip_last_error(), kw
    # a NaN beyond the S entries that are read is not the arrays'
    tail = _arr(1.0, 0.5, float("nan"))
    assert call(nscales=0, sw=tail) == _lib.CIP_EINVAL and b"nscales" in so.cip_last_error()


def test_convolve_and_taps_argument_checks_come_before_the_device():
    so = _lib.lib()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    taps = _arr(*([1.0 / 257.0] * 257))

    def conv(src=fake, nx=8, ny=8, t=taps, radius=1, dst=other):
        return so.cip_ms_convolve(src, nx, ny, t, radius, None, dst)

    for kw in (dict(src=None), dict(t=None), dict(dst=None), dict(nx=0), dict(ny=-2), dict(radius=-1),
               dict(radius=129), dict(t=_arr(0.5, float("nan"), 0.5)), dict(t=_arr(0.5, 0.5, float("inf"))),
               dict(nx=1 << 62, ny=4)):
        assert conv(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_ms_convolve" in so.cip_last_error(), kw
    out = _arr(*([0.0] * 257))
    for width, radius, t in ((0.5, 1, out), (-1.0, 1, out), (float("nan"), 1, out), (float("inf"), 1, out),
                             (2.0, -1, out), (2.0, 129, out), (2.0, 3, None), (0.0, 1, out)):
        assert so.cip_ms_scale_taps(width, radius, t) == _lib.CIP_EINVAL, (width, radius)
        assert b"cip_ms_scale_taps" in so.cip_last_error()
    for width, tol in ((0.5, 1e-8), (-2.0, 1e-8), (float("nan"), 1e-8), (3.0, 0.0), (3.0, 1.0), (3.0, -1.0),
                       (3.0, float("nan"))):
        assert so.cip_ms_scale_radius(width, tol) == _lib.CIP_EINVAL, (width, tol)
        assert b"cip_ms_scale_radius" in so.cip_last_error()


# ---- taps and radius ----------------------------------------------------------
@pytest.mark.parametrize("width, radius", [(1.0, None), (2.5, None), (10.0, None), (10.0, 7), (49.0, None),
                                           (300.0, 128)])
def test_scale_taps_against_the_numpy_formula(width, radius):
    taps = multiscale.scale_taps(width, radius)
    want = _ms_np.scale_taps(width, radius)
    assert taps.dtype == np.float64 and taps.shape == want.shape
    assert taps.size == 2 * (multiscale.scale_radius(width) if radius is None else radius) + 1
    assert np.abs(taps - want).max() <= 4 * np.spacing(want).max()
    assert (np.abs(taps - want) <= 4 * np.spacing(want)).all()  # 4 ulp, tap by tap
    # the taps' own sum (fsum adds exactly: 257 rounded adds would measure the adding, up to 256 * 2^-53)
    assert abs(math.fsum(taps) - 1.0) <= 1e-15
    assert np.array_equal(taps.view(np.int64), taps[::-1].view(np.int64))  # symmetric to the bit
    assert taps.argmax() == taps.size // 2 and (taps > 0).all()


def test_width_zero_is_the_single_tap_one():
    assert multiscale.scale_radius(0.0) == 0
    assert multiscale.scale_taps(0.0).tolist() == [1.0] and multiscale.scale_taps(0.0, 0).tolist() == [1.0]


def test_radius_rule():
    for width in (0.0, 1.0, 10.0):
        assert multiscale.scale_radius(width) == _ms_np.scale_radius(width), width
    assert (multiscale.scale_radius(1.0), multiscale.scale_radius(10.0)) == (3, 26)
    assert multiscale.scale_radius(10.0, 1e-4) == _ms_np.scale_radius(10.0, 1e-4) < 26
    # the first width (in steps of 1/8 pixel) whose radius exceeds CIP_MS_MAX_RADIUS
    first = next(w for w in np.arange(8, 8 * 200) / 8.0 if _ms_np.scale_radius(w) > _lib.MS_MAX_RADIUS)
    assert _ms_np.scale_radius(first - 0.125) == multiscale.scale_radius(first - 0.125) == _lib.MS_MAX_RADIUS
    assert _lib.lib().cip_ms_scale_radius(float(first), 1e-8) == _lib.CIP_ERANGE
    assert b"CIP_MS_MAX_RADIUS" in _lib.lib().cip_last_error()
    with pytest.raises(ValueError, match="CIP_MS_MAX_RADIUS"):
        multiscale.scale_radius(first)
    assert multiscale.scale_radius(first, 1e-4) <= _lib.MS_MAX_RADIUS  # a looser tol still fits


# ---- the numpy statement --------------------------------------------------------
def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("kw", [dict(gain=0.2, niter=40), dict(gain=0.3, niter=500, threshold=0.9),
                                dict(gain=0.2, niter=30, psf_centre=(5, 20)), dict(niter=0)])
def test_one_scale_identity_is_hogbom(kw):
    rng = np.random.default_rng(3)
    img = rng.standard_normal((70, 45))
    img[0, 0], img[69, 44], img[35, 22], img[10, 10] = 9.0, -8.0, 7.0, np.nan
    cx, cy = kw.get("psf_centre", (16, 10))
    r = np.hypot(np.arange(33)[:, None] - cx, np.arange(21)[None, :] - cy)
    psf = np.exp(-r * r / 8.0) * np.cos(0.7 * r)
    mask = (rng.random((70, 45)) < 0.7).astype(np.uint8)
    model0 = rng.standard_normal((70, 45))
    for extra in (dict(), dict(mask=mask, model=model0)):
        ref_model, ref_res, ref_info = _clean_np.hogbom_clean(img, psf, **kw, **extra)
        mkw = dict(kw, **extra)
        if "model" in mkw:
            mkw["model"] = mkw["model"][None]
        model, res, info = _ms_np.ms_clean(img[None], psf[None], np.ones(1), np.ones(1), **mkw)
        assert _same(model[0], ref_model) and _same(res[0], ref_res)
        assert _same(info["comp_index"], ref_info["comp_index"]) and _same(info["comp_flux"], ref_info["comp_flux"])
        assert (info["comp_scale"] == 0).all() and info["peak_scale"] == 0
        for key in ("niter_done", "stop_reason", "peak_index"):
            assert info[key] == ref_info[key], key
        assert _same(np.float64(info["peak"]), np.float64(ref_info["peak"]))


def test_packed_index():
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert [_ms_np.tri(s, q, 3) for s, q in pairs] == [0, 1, 2, 3, 4, 5]
    assert [multiscale.tri(s, q, 3) for s, q in pairs] == [0, 1, 2, 3, 4, 5]
    for n in range(1, 7):  # a bijection onto 0 .. S (S + 1) / 2 - 1, in row order
        assert [_ms_np.tri(s, q, n) for s in range(n) for q in range(s, n)] == list(range(n * (n + 1) // 2))
    # cross_psfs fills the planes in that order: scale s first, then scale q
    psf = np.zeros((41, 41))
    psf[20, 20] = 1.0
    widths = [0, 3, 6]
    cross = _ms_np.cross_psfs(psf, widths)
    assert cross.shape == (6, 41, 41) and _same(cross[0], psf)
    assert _same(cross[4], _ms_np.smooth(_ms_np.smooth(psf, 3), 6))


def test_planted_blob_is_one_component_of_the_widest_scale():
    widths, amp, n = [0, 5, 10], 3.0, 96
    taps = _ms_np.scale_taps(10)
    rad = taps.size // 2
    img = np.zeros((n, n))
    img[n // 2 - rad:n // 2 + rad + 1, n // 2 - rad:n // 2 + rad + 1] = amp * np.outer(taps, taps)
    # a delta PSF in a patch that holds the widest cross term (two radii of the width-10 scale)
    psf = np.zeros((4 * rad + 1, 4 * rad + 1))
    psf[2 * rad, 2 * rad] = 1.0
    cross = _ms_np.cross_psfs(psf, widths)
    select_weight, flux_scale = _ms_np.scale_weights(cross, widths)
    lib_weights = multiscale.scale_weights(cross, widths)
    assert _same(lib_weights[0], select_weight) and _same(lib_weights[1], flux_scale)
    res = _ms_np.scale_residuals(img, widths)
    centre = (n // 2) * n + n // 2
    scores = [np.abs(select_weight[s] * res[s]).max() / amp for s in range(3)]
    print("selection scores / A:", scores)
    assert scores[2] == pytest.approx(0.40, abs=0.01) and scores[1] == pytest.approx(0.28, abs=0.01)
    assert scores[0] == pytest.approx(0.009, abs=0.001)
    probe = _ms_np.ms_clean(res, cross, select_weight, flux_scale, niter=0)[2]
    assert (probe["peak_scale"], probe["peak_index"]) == (2, centre)
    model, out, info = _ms_np.ms_clean(res, cross, select_weight, flux_scale, gain=1.0, niter=1)
    assert info["comp_scale"].tolist() == [2] and info["comp_index"].tolist() == [centre]
    assert info["comp_flux"][0] == pytest.approx(amp, rel=1e-12)
    print("largest |residual| / A after one component:", np.abs(out).max() / amp)
    assert np.abs(out).max() < 1e-12 * amp
    assert np.count_nonzero(model) == 1 and model[2, n // 2, n // 2] == info["comp_flux"][0]
    # and the model image is the blob again
    assert np.abs(_ms_np.ms_model(model, widths) - img).max() < 1e-12 * amp


def test_scale_weights_values_and_refusals():
    cross = np.zeros((3, 9, 9))
    cross[:, 4, 4] = [1.0, 0.5, 0.25]
    sw, fs = multiscale.scale_weights(cross, [0, 8])
    assert fs.tolist() == [1.0, 4.0] and sw.tolist() == [1.0, (1.0 - 0.6) * 4.0]
    assert multiscale.scale_weights(cross, [0, 8], scale_bias=0.0)[0].tolist() == [1.0, 4.0]
    one = multiscale.scale_weights(cross[:1], [0])
    assert one[0].tolist() == [1.0] and one[1].tolist() == [1.0]  # width_max 0: the bias is 1
    off = np.zeros((1, 9, 9))
    off[0, 1, 2] = 2.0
    assert multiscale.scale_weights(off, [3], centre=(1, 2))[1].tolist() == [0.5]
    for bad in (0.0, -1.0, np.nan, np.inf):
        broken = cross.copy()
        broken[2, 4, 4] = bad
        with pytest.raises(ValueError, match="finite and > 0"):
            multiscale.scale_weights(broken, [0, 8])
    with pytest.raises(ValueError, match="cross_psfs"):
        multiscale.scale_weights(cross, [0, 4, 8])
    with pytest.raises(ValueError, match="centre"):
        multiscale.scale_weights(cross, [0, 8], centre=(9, 0))
    for bad in ([], [0, 0.5], [4, 2], [2, 2], [0, 1, 2, 3, 4, 5, 6], [np.nan]):
        with pytest.raises(ValueError, match="widths"):
            multiscale.scale_weights(cross, bad)


# ---- the package ------------------------------------------------------------------
def test_python_entry_points(monkeypatch):
    import torch

    import ska_sdp_cip_amd as pkg
    from ska_sdp_cip_amd import _call

    assert pkg.multiscale is multiscale and "multiscale" in pkg.__all__
    for name in ("scale_radius", "scale_taps", "scale_weights", "ms_clean", "device_ms_convolve",
                 "device_scale_residuals", "device_cross_psfs", "device_ms_clean", "device_ms_model",
                 "device_ms_major_cycles"):
        assert getattr(pkg, name) is getattr(multiscale, name) and name in pkg.__all__, name
    params = inspect.signature(multiscale.device_ms_major_cycles).parameters
    from ska_sdp_cip_amd import deconvolve

    assert set(inspect.signature(deconvolve.device_major_cycles).parameters) <= set(params)
    assert params["widths"].kind is inspect.Parameter.KEYWORD_ONLY and params["restore"].default is False
    conv = inspect.signature(multiscale.device_ms_convolve).parameters
    assert conv["tol"].default == 1e-8 and conv["out"].default is None
    assert inspect.signature(multiscale.scale_weights).parameters["scale_bias"].default == 0.6
    monkeypatch.setattr(_call.torch.cuda, "is_available", lambda: False)
    img = torch.zeros((2, 4, 4), dtype=torch.float64)
    psfs = torch.zeros((3, 4, 4), dtype=torch.float64)
    for fn, args in ((multiscale.device_ms_clean, (img, psfs, np.ones(2), np.ones(2))),
                     (multiscale.ms_clean, (np.zeros((2, 4, 4)), np.zeros((3, 4, 4)), np.ones(2), np.ones(2))),
                     (multiscale.device_ms_convolve, (img[0], 2.0)),
                     (multiscale.device_ms_model, (img, [0, 2]))):
        with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
            fn(*args)
