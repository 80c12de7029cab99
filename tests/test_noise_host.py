"""
Host-side checks of the image noise and the island mask (no GPU):
include/cip_noise.h against `_lib.NOISE_PROTOTYPES`, `_lib.NoiseResult` and
`_lib.MaskResult` (the method of test_ms_host.py on the seventh header), every
argument check of the three entry points through the shared object, the numpy
statement `_noise_np` against scipy's labelling and numpy's median, and the
premises of test_gpu_auto_major.py on its scene, in numpy.
"""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import _auto_scene as au
import _clean_np
import _ms_scene as sc
import _noise_np
import oracle
from ska_sdp_cip_amd import _lib, noise

HEADER = Path(__file__).resolve().parents[1] / "include" / "cip_noise.h"
SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "double": ctypes.c_double}
HOST_POINTERS = {"count_out": ctypes.POINTER(ctypes.c_int64), "value_out": ctypes.POINTER(ctypes.c_double)}
STRUCTS = {"cip_noise_result": _lib.NoiseResult, "cip_mask_result": _lib.MaskResult}
NAMES = ("cip_image_select", "cip_image_noise", "cip_auto_mask")


@pytest.fixture(scope="module")
def header():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


# ---- header against table ----------------------------------------------------
def test_every_prototype_matches_the_table(header):
    protos = {}
    for ret, name, params in re.findall(r"\b(int|const\s+char\s*\*)\s*(cip_\w+)\s*\(([^)]*)\)\s*;", header):
        protos[name] = (ret, [" ".join(p.split()) for p in params.split(",")])
    assert tuple(protos) == tuple(_lib.NOISE_PROTOTYPES) == NAMES
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.NOISE_PROTOTYPES[name]
        assert ret == "int" and restype is ctypes.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            if "*" in decl:
                base = decl.replace("const", " ").split("*")[0].strip()
                if base in STRUCTS:
                    assert argtype is ctypes.POINTER(STRUCTS[base]), (name, k, decl)
                elif decl.split()[-1] in HOST_POINTERS:
                    assert argtype is HOST_POINTERS[decl.split()[-1]], (name, k, decl)
                else:
                    assert argtype is ctypes.c_void_p, (name, k, decl)
            else:
                assert argtype is SCALARS[decl.replace("const", " ").split()[0]], (name, k, decl)
    defines = dict(re.findall(r"#define\s+(CIP_\w+)\s+([0-9.]+)", header))
    assert float(defines["CIP_MAD_TO_SIGMA"]) == _lib.MAD_TO_SIGMA == noise.MAD_TO_SIGMA == 1.482602218505602
    assert int(defines["CIP_MASK_POSITIVE"]) == _lib.MASK_POSITIVE == 1
    assert int(defines["CIP_MASK_CONN4"]) == _lib.MASK_CONN4 == 2
    assert '#include "cip.h"' in header


def test_result_structs_match_the_mirrors(header):
    structs = dict(re.findall(r"typedef\s+struct\s+(cip_\w+)\s*\{(.*?)\}\s*\1\s*;", header, flags=re.S))
    assert tuple(structs) == tuple(STRUCTS)
    for name, mirror in STRUCTS.items():
        fields = [(m[1], SCALARS[m[0]]) for m in re.findall(r"(\w+)\s+(\w+)\s*;", structs[name])]
        assert fields == list(mirror._fields_), name
        assert ctypes.sizeof(mirror) == 32, name
    assert [f for f, _ in _lib.NoiseResult._fields_] == ["count", "median", "mad", "sigma"]
    assert [f for f, _ in _lib.MaskResult._fields_] == ["n_seed", "n_island", "n_out", "rounds"]


def test_library_exports_and_other_tables_unchanged():
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in _lib.NOISE_PROTOTYPES:
        assert hasattr(so, name), name
        for table in (_lib.PROTOTYPES, _lib.RESTORE_PROTOTYPES, _lib.MFS_PROTOTYPES, _lib.CAL_PROTOTYPES,
                      _lib.DFT_PROTOTYPES, _lib.MS_PROTOTYPES):
            assert name not in table
    loaded = _lib.lib()  # lib() applies all seven tables
    for name, (restype, argtypes) in _lib.NOISE_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---- argument checks: all before any device work -------------------------------
FAKE, OTHER = ctypes.c_void_p(4096), ctypes.c_void_p(8192)  # never dereferenced: every call below is refused
BIG = 1 << 62


def test_select_argument_checks_come_before_the_device():
    so = _lib.lib()
    count, value = ctypes.c_int64(-7), ctypes.c_double(0.0)

    def call(img=FAKE, nx=8, ny=8, rank=0, count_out=ctypes.byref(count), value_out=ctypes.byref(value)):
        return so.cip_image_select(img, nx, ny, None, rank, None, count_out, value_out)

    for kw in (dict(img=None), dict(nx=0), dict(ny=-1), dict(nx=BIG, ny=4), dict(rank=-1), dict(count_out=None),
               dict(value_out=None)):
        assert call(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_image_select" in so.cip_last_error(), kw
    assert count.value == -7


def test_noise_argument_checks_come_before_the_device():
    so = _lib.lib()
    out = _lib.NoiseResult()

    def call(img=FAKE, nx=8, ny=8, res=ctypes.byref(out)):
        return so.cip_image_noise(img, nx, ny, None, None, res)

    for kw in (dict(img=None), dict(nx=0), dict(ny=-3), dict(nx=4, ny=BIG), dict(res=None)):
        assert call(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_image_noise" in so.cip_last_error(), kw


def test_auto_mask_argument_checks_come_before_the_device():
    so = _lib.lib()
    out = _lib.MaskResult()
    nan, inf = float("nan"), float("inf")

    def call(img=FAKE, nx=8, ny=8, seed=5.0, grow=3.0, flags=0, mask=OTHER, res=ctypes.byref(out)):
        return so.cip_auto_mask(img, nx, ny, seed, grow, None, None, flags, None, mask, res)

    for kw in (dict(img=None), dict(mask=None), dict(res=None), dict(nx=0), dict(ny=-1), dict(nx=BIG, ny=4),
               dict(seed=2.0, grow=3.0), dict(grow=0.0), dict(grow=-1.0), dict(seed=nan), dict(grow=nan),
               dict(seed=inf), dict(seed=inf, grow=inf), dict(seed=0.0, grow=0.0), dict(flags=4), dict(flags=-1),
               dict(flags=8 | 1)):
        assert call(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_auto_mask" in so.cip_last_error(), kw


# ---- the numpy statement ---------------------------------------------------------
def _smooth_field(seed, n=120):
    rng = np.random.default_rng(seed)
    f = np.fft.rfft2(rng.standard_normal((n, n)))
    k = np.hypot(np.fft.fftfreq(n)[:, None], np.fft.rfftfreq(n)[None, :])
    return np.fft.irfft2(f * np.exp(-(k / 0.05) ** 2), s=(n, n))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_numpy_auto_mask_against_scipy_label(seed, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    img = _smooth_field(seed)
    hi_t, lo_t = np.percentile(np.abs(img), [99, 90])
    mask, info = _noise_np.auto_mask(img, hi_t, lo_t, connectivity=connectivity)
    lo = np.abs(img) >= lo_t
    labels, _ = ndimage.label(lo, structure=np.ones((3, 3)) if connectivity == 8 else None)
    keep = np.unique(labels[np.abs(img) >= hi_t])
    want = np.isin(labels, keep[keep > 0])
    assert np.array_equal(mask != 0, want) and 0 < info["n_seed"] < info["n_island"] == want.sum() < lo.sum()
    assert info["n_out"] == info["n_island"]


def test_numpy_auto_mask_on_a_serpentine():
    img = _noise_np.serpentine(9)
    img[0, 0] = 2.0
    mask, info = _noise_np.auto_mask(img, 2.0, 1.0, connectivity=4)
    assert np.array_equal(mask, (img > 0).astype(np.uint8)) and info["n_seed"] == 1
    assert info["n_island"] == 5 * 9 + 4
    img[4, 3] = np.nan  # severs the path half way
    cut, _ = _noise_np.auto_mask(img, 2.0, 1.0, connectivity=4)
    # the path enters row 4 at column 0: it keeps columns 0 .. 2 and nothing behind the NaN
    assert cut[:4].sum() == 2 * 9 + 2 and cut[4, :3].sum() == 3 and cut[4, 3:].sum() == 0 and cut[5:].sum() == 0


def test_numpy_noise_against_numpy_median_on_odd_counts():
    rng = np.random.default_rng(4)
    for n in (1, 3, 101, 4097):
        x = rng.standard_normal(n) * 3.0 + 1.0
        got = _noise_np.noise(x.reshape(1, n))
        assert got["count"] == n and got["median"] == np.median(x)
        assert got["mad"] == np.median(np.abs(x - np.median(x)))
        assert got["sigma"] == 1.482602218505602 * got["mad"]
    # the lower median of an even count, NaN and inf excluded, the region, the overflow of d
    x = np.array([[4.0, np.nan, 1.0, np.inf, 3.0, 2.0, -np.inf]])
    got = _noise_np.noise(x)
    assert (got["count"], got["median"], got["mad"]) == (4, 2.0, 1.0)
    assert _noise_np.noise(x, region=np.array([[1, 1, 0, 1, 1, 1, 1]]))["median"] == 3.0
    assert _noise_np.noise(np.full((2, 2), np.nan))["count"] == 0
    big = _noise_np.noise(np.array([[1e308, -1e308, -1e308, 1e308]]))
    assert big["median"] == -1e308 and big["mad"] == 0.0
    big = _noise_np.noise(np.array([[1e308, -1e308, 1e308, 1e308, -1e308]]))
    assert big["median"] == 1e308 and big["mad"] == 0.0
    big = _noise_np.noise(np.array([[1e308, -1e308, 0.5e308]]))
    assert big["median"] == 0.5e308 and big["mad"] == 0.5e308  # d = [0.5e308, inf, 0]
    assert _noise_np.select(x, 3) == (4.0, 4) and _noise_np.select(x, 4) == (None, 4)
    assert 0.6744 < 1.0 / 1.482602218505602 < 0.6745  # Phi^-1(3/4)


# ---- the premises of the major-cycle test, in numpy --------------------------------
def test_noisy_scene_keeps_the_faint_source_above_ten_sigma():
    uvw, freq, pix = sc.tracks()
    vis = au.noisy_visibilities(uvw, freq, pix)
    wgt = np.ones(vis.shape)
    n = au.NPIX

    def invert(v):
        return oracle.ms2dirty(uvw, freq, v, wgt, n, n, pix, pix) / wgt.sum()

    psf = invert(np.ones_like(vis))
    residual = invert(vis)
    model = np.zeros((n, n))
    grown = np.zeros((n, n), dtype=np.uint8)
    faint = min(flux for _, flux in au.POINTS)
    sigmas = []
    for cycle in range(au.MAJOR["n_major"]):
        sigma = _noise_np.noise(residual)["sigma"]
        sigmas.append(sigma)
        assert np.isfinite(sigma) and sigma > 0.0
        if cycle == 0:
            print("first residual: sigma", sigma, "faint source / sigma", faint / sigma)
            assert faint >= 10.0 * sigma
        seed_s, grow_s = au.AUTO["auto_mask"]
        grown, info = _noise_np.auto_mask(residual, seed_s * sigma, grow_s * sigma, base=grown)
        for pos, _ in au.POINTS:
            assert grown[pos] == 1
        floor = au.AUTO["auto_threshold"] * sigma
        peak = np.abs(residual[grown != 0]).max()
        if peak <= floor:
            break
        model, _, cinfo = _clean_np.hogbom_clean(residual, psf, gain=au.MAJOR["gain"], threshold=floor,
                                                 niter=au.MAJOR["niter"], mask=grown, model=model)
        print("cycle", cycle, "sigma", sigma, "mask", info, "peak", peak, "components", cinfo["niter_done"])
        residual = invert(vis - au.model_visibilities(uvw, freq, pix, model))
    assert len(sigmas) >= 2 and sigmas[-1] < sigmas[0]  # the sources' sidelobes leave the residual
    assert (grown[model != 0.0] == 1).all()


# ---- the package ------------------------------------------------------------------
def test_python_entry_points(monkeypatch):
    import torch

    import ska_sdp_cip_amd as pkg
    from ska_sdp_cip_amd import _call, deconvolve, mfs, multiscale

    assert pkg.noise is noise and "noise" in pkg.__all__
    for name in ("MAD_TO_SIGMA", "device_image_select", "device_image_noise", "device_auto_mask", "image_noise",
                 "auto_mask"):
        assert getattr(pkg, name) is getattr(noise, name) and name in pkg.__all__, name
    for fn in (deconvolve.device_major_cycles, mfs.device_mfs_major_cycles, multiscale.device_ms_major_cycles):
        params = inspect.signature(fn).parameters
        for name in ("auto_threshold", "auto_mask"):
            assert params[name].default is None and params[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn, name)
    mask = inspect.signature(noise.device_auto_mask).parameters
    assert mask["grow"].default is None and mask["connectivity"].default == 8 and mask["positive"].default is False
    monkeypatch.setattr(_call.torch.cuda, "is_available", lambda: False)
    img = torch.zeros((4, 4), dtype=torch.float64)
    for fn, args in ((noise.device_image_select, (img, 0)), (noise.device_image_noise, (img,)),
                     (noise.device_auto_mask, (img, 1.0)), (noise.image_noise, (np.zeros((4, 4)),)),
                     (noise.auto_mask, (np.zeros((4, 4)), 1.0))):
        with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
            fn(*args)
