"""
Host-side checks of multi-term MFS (no GPU): include/cip_mfs.h against
`_lib.MFS_PROTOTYPES` (the method of test_restore_host.py on the third
header), `taylor_basis`, `mfs_hessian`, and the numpy statement `_mfs_np`
against `_clean_np` where the two operators coincide (T = 1, hinv = [[1]]).
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _clean_np
import _mfs_np
from ska_sdp_cip_amd import _lib, mfs

HEADER = Path(__file__).resolve().parents[1] / "include" / "cip_mfs.h"
SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "double": ctypes.c_double}
PF64 = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def header():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


# ---- header against table ----------------------------------------------------
def test_every_prototype_matches_the_table(header):
    protos = {}
    for ret, name, params in re.findall(r"\b(int|const\s+char\s*\*)\s*(cip_\w+)\s*\(([^)]*)\)\s*;", header):
        protos[name] = (ret, [" ".join(p.split()) for p in params.split(",")])
    assert tuple(protos) == tuple(_lib.MFS_PROTOTYPES) == ("cip_mfs_clean",)
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.MFS_PROTOTYPES[name]
        assert ret == "int" and restype is ctypes.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            if "*" in decl:
                base = decl.replace("const", " ").split("*")[0].strip()
                if base == "cip_clean_result":
                    assert argtype is ctypes.POINTER(_lib.CleanResult), (name, k, decl)
                elif decl.split()[-1] == "hinv":  # the one HOST array
                    assert base == "double" and argtype is PF64, (name, k, decl)
                else:
                    assert argtype is ctypes.c_void_p, (name, k, decl)
            else:
                assert argtype is SCALARS[decl.replace("const", " ").split()[0]], (name, k, decl)
    defines = dict(re.findall(r"#define\s+(CIP_\w+)\s+(\d+)", header))
    assert int(defines["CIP_MFS_MAX_TERMS"]) == _lib.MFS_MAX_TERMS == 3
    assert '#include "cip.h"' in header and "typedef" not in header  # cip_clean_result and CIP_CLEAN_* are cip.h's


def test_library_exports_and_other_tables_unchanged():
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in _lib.MFS_PROTOTYPES:
        assert hasattr(so, name), name
        assert name not in _lib.PROTOTYPES and name not in _lib.RESTORE_PROTOTYPES
    assert len(_lib.PROTOTYPES) == 41 and len(_lib.RESTORE_PROTOTYPES) == 6
    loaded = _lib.lib()  # lib() applies all three tables
    for name, (restype, argtypes) in _lib.MFS_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_argument_checks_come_before_the_device():
    so = _lib.lib()
    out = _lib.CleanResult()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)  # never dereferenced: every call below is refused
    good = (ctypes.c_double * 9)(1.0, 0.1, 0.0, 0.1, 2.0, 0.0, 0.0, 0.0, 1.0)

    def call(res=fake, nterms=2, nx=8, ny=8, psf=other, px=5, py=5, cx=-1, cy=-1, hinv=good, gain=0.1, threshold=0.0,
             niter=4, batch=0, ci=None, cf=None):
        return so.cip_mfs_clean(res, nterms, nx, ny, psf, px, py, cx, cy, hinv, None, gain, threshold, niter, batch,
                                None, None, ci, cf, ctypes.byref(out))

    nan = (ctypes.c_double * 4)(1.0, 0.0, float("nan"), 1.0)
    inf = (ctypes.c_double * 4)(1.0, float("inf"), 0.0, 1.0)
    for kw in (dict(nterms=0), dict(nterms=4), dict(nterms=-1), dict(hinv=None), dict(hinv=nan), dict(hinv=inf),
               dict(ci=fake), dict(cf=fake), dict(res=None), dict(psf=None), dict(nx=0), dict(py=-3), dict(cx=5),
               dict(cy=-2), dict(gain=0.0), dict(gain=float("nan")), dict(threshold=-1.0), dict(niter=-1),
               dict(batch=-1)):
        assert call(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_mfs_clean" in so.cip_last_error(), kw
    # a NaN beyond the T x T entries that are read is not hinv's
    tail = (ctypes.c_double * 9)(1.0, 0.1, 0.1, 2.0, *([float("nan")] * 5))
    assert call(nterms=0, hinv=tail) == _lib.CIP_EINVAL and b"nterms" in so.cip_last_error()


# ---- taylor_basis ----------------------------------------------------------------
def test_taylor_basis_values():
    freq = np.array([1.0e9, 1.1e9, 1.3e9])
    basis = mfs.taylor_basis(freq, 1.1e9, 3)
    assert basis.shape == (3, 3) and basis.dtype == np.float64
    x = (freq - 1.1e9) / 1.1e9
    assert np.array_equal(basis[0], np.ones(3))  # x^0 = 1 at x = 0 too
    assert np.array_equal(basis[1], x) and basis[1, 1] == 0.0
    assert np.allclose(basis[2], x * x, rtol=1e-15, atol=0.0)
    assert basis[1, 0] == pytest.approx(-1.0 / 11.0, rel=1e-15) and basis[1, 2] == pytest.approx(2.0 / 11.0, rel=1e-15)
    assert np.array_equal(mfs.taylor_basis(freq, 1.1e9, 1), np.ones((1, 3)))
    import torch

    t = mfs.taylor_basis(torch.from_numpy(freq), 1.1e9, 3)
    assert torch.is_tensor(t) and t.dtype == torch.float64 and np.allclose(t.numpy(), basis, rtol=1e-15, atol=0.0)
    for bad in (0, 4):
        with pytest.raises(ValueError, match="nterms"):
            mfs.taylor_basis(freq, 1.1e9, bad)
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="ref_freq"):
            mfs.taylor_basis(freq, bad, 2)


# ---- mfs_hessian -------------------------------------------------------------------
def _stack(peaks, shape=(7, 9), centre=None):
    cx, cy = (shape[0] // 2, shape[1] // 2) if centre is None else centre
    psfs = np.random.default_rng(4).standard_normal((len(peaks), *shape)) * 0.01
    psfs[:, cx, cy] = peaks
    return psfs


def test_mfs_hessian_hand_made():
    peaks = [1.0, 0.05, 0.0125, 0.002, 0.0006]
    hessian, hinv = mfs.mfs_hessian(_stack(peaks))
    assert hessian.dtype == hinv.dtype == np.float64
    assert np.array_equal(hessian, [[1.0, 0.05, 0.0125], [0.05, 0.0125, 0.002], [0.0125, 0.002, 0.0006]])
    assert np.array_equal(hessian, hessian.T) and np.array_equal(hinv, np.linalg.inv(hessian))
    assert np.allclose(hinv @ hessian, np.eye(3), atol=1e-9)
    h2, hinv2 = mfs.mfs_hessian(_stack(peaks[:3]))
    assert np.array_equal(h2, [[1.0, 0.05], [0.05, 0.0125]])
    det = 1.0 * 0.0125 - 0.05 * 0.05
    assert np.allclose(hinv2, np.array([[0.0125, -0.05], [-0.05, 1.0]]) / det, rtol=1e-13)
    h1, hinv1 = mfs.mfs_hessian(_stack([0.5]))
    assert h1.tolist() == [[0.5]] and hinv1.tolist() == [[2.0]]
    # another centre, and a torch stack
    import torch

    off = _stack(peaks[:3], centre=(0, 8))
    assert np.array_equal(mfs.mfs_hessian(off, centre=(0, 8))[0], h2)
    assert not np.array_equal(mfs.mfs_hessian(off)[0], h2)
    assert np.array_equal(mfs.mfs_hessian(torch.from_numpy(_stack(peaks[:3])))[1], hinv2)


def test_mfs_hessian_refusals():
    with pytest.raises(ValueError, match="singular"):  # one channel at the reference frequency: x = 0
        mfs.mfs_hessian(_stack([1.0, 0.0, 0.0]))
    with pytest.raises(ValueError, match="singular"):  # rank one
        mfs.mfs_hessian(_stack([1.0, 0.5, 0.25]))
    with pytest.raises(ValueError, match="singular"):
        mfs.mfs_hessian(_stack([1.0, 1e-7, 1e-14 + 1e-27]))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="not finite"):
            mfs.mfs_hessian(_stack([1.0, bad, 0.0125]))
    with pytest.raises(ValueError, match="2 nterms - 1"):
        mfs.mfs_hessian(_stack([1.0, 0.1]))  # an even number of PSFs
    with pytest.raises(ValueError, match="2 nterms - 1"):
        mfs.mfs_hessian(_stack([1.0] * 7))  # nterms = 4
    with pytest.raises(ValueError, match="2 nterms - 1"):
        mfs.mfs_hessian(np.ones((7, 9)))
    with pytest.raises(ValueError, match="centre"):
        mfs.mfs_hessian(_stack([1.0]), centre=(7, 0))


# ---- the numpy statement ------------------------------------------------------------
def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("kw", [dict(gain=0.2, niter=40), dict(gain=0.3, niter=500, threshold=0.9),
                                dict(gain=0.2, niter=30, psf_centre=(5, 20)), dict(niter=0)])
def test_one_term_identity_is_hogbom(kw):
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
        model, res, info = _mfs_np.mfs_clean(img[None], psf[None], np.ones((1, 1)), **mkw)
        assert _same(model[0], ref_model) and _same(res[0], ref_res)
        assert _same(info["comp_index"], ref_info["comp_index"])
        assert _same(info["comp_flux"][:, 0], ref_info["comp_flux"])
        for key in ("niter_done", "stop_reason", "peak_index"):
            assert info[key] == ref_info[key], key
        assert _same(np.float64(info["peak"]), np.float64(ref_info["peak"]))


def test_two_terms_on_a_noiseless_source_solve_for_both_coefficients():
    # r_t = I0 psf_t + I1 psf_{t+1}: gain 1 takes (I0, I1) in one component and leaves zero
    r = np.hypot(np.arange(15)[:, None] - 7, np.arange(15)[None, :] - 7)
    shape = np.exp(-r * r / 6.0)
    psfs = np.stack([1.0 * shape, 0.05 * shape, 0.0125 * shape])
    hessian, hinv = mfs.mfs_hessian(psfs)
    i0, i1 = 2.0, -1.4
    res = np.zeros((2, 15, 15))
    for t in range(2):
        res[t] = i0 * psfs[t] + i1 * psfs[t + 1]
    model, out, info = _mfs_np.mfs_clean(res, psfs, hinv, gain=1.0, niter=1)
    assert info["comp_index"].tolist() == [7 * 15 + 7] and info["niter_done"] == 1
    assert info["comp_flux"][0] == pytest.approx([i0, i1], rel=1e-12)
    assert np.abs(out).max() <= 1e-13 and model[:, 7, 7] == pytest.approx([i0, i1], rel=1e-12)


def test_python_entry_points(monkeypatch):
    import torch

    import ska_sdp_cip_amd as pkg
    from ska_sdp_cip_amd import _call

    assert pkg.mfs is mfs and "mfs" in pkg.__all__
    for name in ("taylor_basis", "mfs_hessian", "mfs_clean", "device_mfs_clean", "device_mfs_invert",
                 "device_mfs_residual", "device_mfs_major_cycles"):
        assert getattr(pkg, name) is getattr(mfs, name) and name in pkg.__all__, name
    import inspect

    params = inspect.signature(mfs.device_mfs_major_cycles).parameters
    assert params["nterms"].default == 2 and params["ref_freq"].default is None and params["restore"].default is False
    monkeypatch.setattr(_call.torch.cuda, "is_available", lambda: False)
    img = torch.zeros((2, 4, 4), dtype=torch.float64)
    for fn, args in ((mfs.device_mfs_clean, (img, torch.zeros((3, 4, 4), dtype=torch.float64), np.eye(2))),
                     (mfs.mfs_clean, (np.zeros((2, 4, 4)), np.zeros((3, 4, 4)), np.eye(2)))):
        with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
            fn(*args)
