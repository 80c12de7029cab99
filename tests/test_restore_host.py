"""
Host-side checks of the restoring step (no GPU): include/cip_restore.h against
`_lib.RESTORE_PROTOTYPES` and the `Beam` mirror (the method of
test_binding_host.py on the second header), and the host-only entry points
(`cip_beam_from_fwhm`, `cip_beam_fit_window`, `cip_beam_radius`,
`cip_beam_taps`) against the numpy statement `_restore_np`.
"""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

import _restore_np as rnp
from ska_sdp_cip_amd import _lib
from ska_sdp_cip_amd import restore as rst  # the module (the package exports its functions one by one)
from test_gpu_clean import major_scene

HEADER = Path(__file__).resolve().parents[1] / "include" / "cip_restore.h"
SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "double": ctypes.c_double}
PF64 = ctypes.POINTER(ctypes.c_double)
PAS = (0.0, 0.3, -0.3, 1.2, -1.2, 1.5, math.pi / 2)
FORMS = ((0.11, 0.03, 0.2), (0.02, -0.005, 0.03), (0.3, 0.0, 0.3), (0.0632, -0.0378, 0.0926))


@pytest.fixture(scope="module")
def header():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _fit(window, cut):
    """(status, Beam) of cip_beam_fit_window on a host window."""
    win = np.ascontiguousarray(window, dtype=np.float64)
    out = _lib.Beam()
    rc = _lib.lib().cip_beam_fit_window(win.ctypes.data_as(PF64), win.shape[0] // 2, cut, ctypes.byref(out))
    return rc, out


# ---- header against table ----------------------------------------------------
def test_every_prototype_matches_the_table(header):
    protos = {}
    for ret, name, params in re.findall(r"\b(int|const\s+char\s*\*)\s*(cip_\w+)\s*\(([^)]*)\)\s*;", header):
        protos[name] = (ret, [" ".join(p.split()) for p in params.split(",")])
    assert tuple(protos) == tuple(_lib.RESTORE_PROTOTYPES) and len(protos) == 6
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.RESTORE_PROTOTYPES[name]
        assert ret == "int" and restype is ctypes.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            if "*" in decl:
                base = decl.replace("const", " ").split("*")[0].strip()
                if base == "cip_beam":
                    assert argtype is ctypes.POINTER(_lib.Beam), (name, k, decl)
                elif base == "double" and argtype is not ctypes.c_void_p:
                    assert argtype is PF64, (name, k, decl)
                else:
                    assert argtype is ctypes.c_void_p, (name, k, decl)
            else:
                assert argtype is SCALARS[decl.replace("const", " ").split()[0]], (name, k, decl)


def test_beam_mirror_matches_the_header(header):
    structs = dict(re.findall(r"typedef\s+struct\s+(cip_\w+)\s*\{(.*?)\}\s*\1\s*;", header, flags=re.S))
    assert set(structs) == {"cip_beam"}
    fields = []
    for decl in filter(None, (" ".join(d.split()) for d in structs["cip_beam"].split(";"))):
        ctype, names = decl.split(" ", 1)
        fields += [(n.strip(), SCALARS[ctype]) for n in names.split(",")]
    assert fields == list(_lib.Beam._fields_)  # pylint: disable=protected-access
    assert ctypes.sizeof(_lib.Beam) == 56
    defines = dict(re.findall(r"#define\s+(CIP_\w+)\s+([\d.]+)", header))
    assert int(defines["CIP_RESTORE_MAX_RADIUS"]) == _lib.RESTORE_MAX_RADIUS == rnp.MAX_RADIUS == 32
    assert int(defines["CIP_BEAM_FIT_RADIUS"]) == _lib.BEAM_FIT_RADIUS == 8
    assert float(defines["CIP_BEAM_FIT_CUT"]) == _lib.BEAM_FIT_CUT == 0.35


def test_library_exports_and_first_table_unchanged():
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in _lib.RESTORE_PROTOTYPES:
        assert hasattr(so, name), name
        assert name not in _lib.PROTOTYPES and name not in _lib.EXPORTED_SYMBOLS
    assert len(_lib.PROTOTYPES) == 41 and _lib.EXPORTED_SYMBOLS == tuple(_lib.PROTOTYPES)
    loaded = _lib.lib()  # lib() applies both tables
    for name, (restype, argtypes) in _lib.RESTORE_PROTOTYPES.items():
        fn = getattr(loaded, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---- shape formulas -----------------------------------------------------------
@pytest.mark.parametrize("pa", PAS)
def test_shape_round_trip(pa):
    beam = rst.beam_from_fwhm(7.5, 3.25, pa)
    a, b, c = rnp.from_fwhm(7.5, 3.25, pa)
    for got, want in ((beam["a"], a), (beam["b"], b), (beam["c"], c)):
        assert abs(got - want) <= 1e-14 * max(a, c)
    assert beam["n_fit"] == 0
    assert beam["fwhm_major"] == pytest.approx(7.5, rel=1e-14) and beam["fwhm_minor"] == pytest.approx(3.25, rel=1e-14)
    assert beam["pa"] == pytest.approx(pa, rel=1e-14, abs=1e-14)
    major, minor, pa_np = rnp.shape(beam["a"], beam["b"], beam["c"])
    assert (beam["fwhm_major"], beam["fwhm_minor"]) == pytest.approx((major, minor), rel=1e-14)
    assert beam["pa"] == pytest.approx(pa_np, rel=1e-14, abs=1e-14)
    # G is 0.5 at half the major FWHM along the major axis (pa from +axis 1 towards +axis 0)
    da, db = 3.75 * math.sin(pa), 3.75 * math.cos(pa)
    assert math.exp(-(a * da * da + 2 * b * da * db + c * db * db)) == pytest.approx(0.5, rel=1e-12)


def test_shape_edge_cases():
    beam = rst.beam_from_fwhm(4.0, 4.0, 0.7)
    assert beam["pa"] == 0.0 and beam["b"] == 0.0 and beam["a"] == beam["c"]  # circular: pa = 0
    assert rst.beam_from_fwhm(5.0, 2.0, -math.pi / 2)["pa"] == pytest.approx(math.pi / 2, rel=1e-14)  # (-pi/2, pi/2]
    sky = rst.beam_to_sky(rst.beam_from_fwhm(6.0, 3.0, 0.0), 2e-5, 2e-5)
    assert sky["fwhm_major"] == pytest.approx(6.0 * 2e-5, rel=1e-13) and sky["pa"] == pytest.approx(0.0, abs=1e-13)
    # a pixel three times as long along axis 0 turns this round beam into one elongated along axis 0
    sky = rst.beam_to_sky(rst.beam_from_fwhm(4.0, 4.0, 0.0), 3e-5, 1e-5)
    assert sky["fwhm_major"] == pytest.approx(12e-5, rel=1e-13) and sky["fwhm_minor"] == pytest.approx(4e-5, rel=1e-13)
    assert sky["pa"] == pytest.approx(math.pi / 2, rel=1e-13)
    out = _lib.Beam()
    for args in ((3.0, 4.0, 0.0), (3.0, 0.0, 0.0), (3.0, -1.0, 0.0), (math.inf, 1.0, 0.0), (3.0, math.nan, 0.0),
                 (3.0, 2.0, math.nan), (3.0, 2.0, math.inf)):
        assert _lib.lib().cip_beam_from_fwhm(*args, ctypes.byref(out)) == _lib.CIP_EINVAL, args
        with pytest.raises(ValueError, match="cip_beam_from_fwhm"):
            rst.beam_from_fwhm(*args)
    assert _lib.lib().cip_beam_from_fwhm(3.0, 2.0, 0.0, None) == _lib.CIP_EINVAL


# ---- the fit -------------------------------------------------------------------
@pytest.mark.parametrize("cut", [0.5, 0.35])
@pytest.mark.parametrize("form", FORMS)
def test_fit_recovers_exact_gaussians(form, cut):
    a, b, c = form
    window = 1.7 * rnp.gaussian(a, b, c, 8)  # the centre value divides out
    rc, out = _fit(window, cut)
    assert rc == 0, _lib.lib().cip_last_error()
    tol = 1e-10 * max(a, c)
    print(form, cut, out.n_fit, out.a - a, out.b - b, out.c - c)
    assert abs(out.a - a) <= tol and abs(out.b - b) <= tol and abs(out.c - c) <= tol
    assert out.n_fit == len(rnp.fit_set(window, cut)[2]) >= 5
    assert (out.fwhm_major, out.fwhm_minor, out.pa) == pytest.approx(rnp.shape(out.a, out.b, out.c), rel=1e-13,
                                                                        abs=1e-13)
    assert rst.beam_fit_window(window, cut=cut) == out.as_dict()


@pytest.fixture(scope="module")
def psf_windows():
    """17 x 17 patches of the PSFs of `major_scene` (test_gpu_clean.py) by direct
    DFT: the scene as it is and with u scaled by 0.45 and v by 0.8."""
    uvw, freq, _, wgt, pix = major_scene()
    return {"iso": rnp.dft_psf(uvw, freq, wgt, pix, 8), "aniso": rnp.dft_psf(uvw, freq, wgt, pix, 8, 0.45, 0.8)}


@pytest.mark.parametrize("cut", [0.5, 0.35])
@pytest.mark.parametrize("which", ["iso", "aniso"])
def test_fit_on_real_psf_windows(psf_windows, which, cut):
    window = psf_windows[which]
    assert window[8, 8] == pytest.approx(1.0, abs=1e-12)
    rc, out = _fit(window, cut)
    assert rc == 0, _lib.lib().cip_last_error()
    a, b, c, n = rnp.fit_window(window, cut)
    print(which, cut, n, (a, b, c), (out.fwhm_major, out.fwhm_minor, out.pa))
    tol = 1e-10 * max(a, c)
    assert out.n_fit == n
    assert abs(out.a - a) <= tol and abs(out.b - b) <= tol and abs(out.c - c) <= tol
    if which == "iso":  # the values of the scene, computed by DFT
        want = {0.5: (0.184105, 0.184104, 8), 0.35: (0.185989, None, 20)}[cut]
        assert out.a == pytest.approx(want[0], abs=2e-6) and out.n_fit == want[2]
        if want[1] is not None:
            assert out.c == pytest.approx(want[1], abs=2e-6)
            assert (out.fwhm_major, out.fwhm_minor) == pytest.approx((3.8809, 3.8805), abs=1e-4)
    else:  # narrower uv coverage along u: the beam is longer along axis 0
        assert out.a < out.c and abs(out.pa) > 1.5


def test_fit_edge_cases():
    so = _lib.lib()
    # only the four axis neighbours reach the cut: an exactly singular matrix
    rc, _ = _fit(rnp.gaussian(0.6, 0.2, 0.5, 8), 0.5)
    assert rc == _lib.CIP_ERANGE
    msg = so.cip_last_error().decode()
    assert "lower cut" in msg and "pass a beam" in msg
    with pytest.raises(ValueError, match="lower cut"):
        rst.beam_fit_window(rnp.gaussian(0.6, 0.2, 0.5, 8), cut=0.5)
    assert _fit(rnp.gaussian(0.6, 0.2, 0.5, 8), 0.2)[0] == 0  # a lower cut does fit
    # NaN on one whole side (the PSF ends there): the other side still fits
    a, b, c = FORMS[0]
    window = rnp.gaussian(a, b, c, 8)
    window[:, :8] = np.nan
    rc, out = _fit(window, 0.35)
    assert rc == 0 and abs(out.a - a) <= 1e-10 * c and abs(out.b - b) <= 1e-10 * c and abs(out.c - c) <= 1e-10 * c
    assert out.n_fit == len(rnp.fit_set(window, 0.35)[2]) < len(rnp.fit_set(rnp.gaussian(a, b, c, 8), 0.35)[2])
    # a form that is not positive definite (a saddle through the neighbours)
    d = np.arange(-2, 3, dtype=np.float64)
    saddle = np.exp(-(0.05 * d[:, None] ** 2 + 2 * 0.2 * d[:, None] * d[None, :] + 0.05 * d[None, :] ** 2))
    saddle[saddle > 1.0] = np.nan  # keeps the centre the largest value
    assert _fit(saddle, 0.3)[0] == _lib.CIP_ERANGE and "positive definite" in so.cip_last_error().decode()
    # the centre pixel must be finite and > 0
    for centre in (0.0, -1.0, np.nan, np.inf):
        window = rnp.gaussian(a, b, c, 8)
        window[8, 8] = centre
        assert _fit(window, 0.35)[0] == _lib.CIP_EINVAL, centre
        assert b"centre pixel" in so.cip_last_error()
    # cut and radius
    good = rnp.gaussian(a, b, c, 8)
    for cut in (0.0, 1.0, -0.5, 1.5, math.nan):
        assert _fit(good, cut)[0] == _lib.CIP_EINVAL, cut
    out = _lib.Beam()
    big = np.ones((131, 131))
    for radius in (0, -1, 65):
        assert so.cip_beam_fit_window(big.ctypes.data_as(PF64), radius, 0.35, ctypes.byref(out)) == _lib.CIP_EINVAL
    assert so.cip_beam_fit_window(None, 8, 0.35, ctypes.byref(out)) == _lib.CIP_EINVAL
    assert so.cip_beam_fit_window(good.ctypes.data_as(PF64), 8, 0.35, None) == _lib.CIP_EINVAL
    # radius 64 is allowed (a 129 x 129 window)
    wide = rnp.gaussian(0.02, -0.005, 0.03, 64)
    rc, out = _fit(wide, 0.35)
    assert rc == 0 and abs(out.a - 0.02) <= 1e-10 * 0.03


# ---- radius and taps -------------------------------------------------------------
def test_beam_radius():
    so = _lib.lib()
    for tol, want in ((1e-8, (6, 8, 13, 21, 31)), (1e-4, (4, 6, 10, 15, 22))):
        for fwhm, r in zip((2, 3, 5, 8, 12), want):
            beam = rst.beam_from_fwhm(fwhm, fwhm, 0.0)
            assert rst.beam_radius(beam, tol) == r == rnp.radius(beam["a"], beam["b"], beam["c"], tol), (fwhm, tol)
    assert rst.beam_radius(rst.beam_from_fwhm(12, 2, 0.4), 1e-8) == 31  # the major axis sets it
    b13 = _lib.Beam(**{k: v for k, v in rst.beam_from_fwhm(13, 13, 0.0).items()})
    assert so.cip_beam_radius(ctypes.byref(b13), 1e-8) == _lib.CIP_ERANGE
    assert b"CIP_RESTORE_MAX_RADIUS" in so.cip_last_error()
    with pytest.raises(ValueError, match="CIP_RESTORE_MAX_RADIUS"):
        rst.beam_radius(rst.beam_from_fwhm(13, 13, 0.0))
    assert so.cip_beam_radius(ctypes.byref(b13), 1e-4) == 24
    for tol in (0.0, 1.0, -1.0, math.nan):
        assert so.cip_beam_radius(ctypes.byref(b13), tol) == _lib.CIP_EINVAL, tol
    assert so.cip_beam_radius(None, 1e-8) == _lib.CIP_EINVAL
    for form in ((0.1, 0.2, 0.1), (0.0, 0.0, 0.1), (-0.1, 0.0, 0.1), (math.nan, 0.0, 0.1)):
        bad = _lib.Beam(a=form[0], b=form[1], c=form[2])
        assert so.cip_beam_radius(ctypes.byref(bad), 1e-8) == _lib.CIP_EINVAL, form


@pytest.mark.parametrize("radius", [0, 1, 5, 13, 32, None])
def test_beam_taps(radius):
    beam = rst.beam_from_fwhm(6, 3, 0.3)
    taps = rst.beam_taps(beam, radius)
    R = radius
    if radius is None:  # the default: where the beam has fallen to 1e-8, ceil(sqrt(log(1e8) / (4 ln 2 / 36))) = 16
        R = rst.beam_radius(beam, 1e-8)
        assert R == rnp.radius(beam["a"], beam["b"], beam["c"], 1e-8) == 16
    assert taps.shape == (2 * R + 1, 2 * R + 1) and taps.dtype == np.float64
    assert taps[R, R] == 1.0
    assert np.array_equal(taps.view(np.int64), taps[::-1, ::-1].view(np.int64))  # taps[R+da][R+db] == taps[R-da][R-db]
    if R:
        assert not np.array_equal(taps, taps.T) and not np.array_equal(taps, taps[::-1])  # b != 0 shows in the table
    want = rnp.taps(beam["a"], beam["b"], beam["c"], R)
    ulp = np.spacing(want)
    assert np.abs(taps - want).max() <= 0 or (np.abs(taps - want) / ulp).max() <= 4.0


def test_beam_taps_refusals():
    so = _lib.lib()
    beam = _lib.Beam(a=0.1, b=0.0, c=0.1)
    buf = np.zeros(65 * 65)
    assert so.cip_beam_taps(ctypes.byref(beam), 33, buf.ctypes.data_as(PF64)) == _lib.CIP_EINVAL
    assert so.cip_beam_taps(ctypes.byref(beam), -1, buf.ctypes.data_as(PF64)) == _lib.CIP_EINVAL
    assert so.cip_beam_taps(ctypes.byref(beam), 3, None) == _lib.CIP_EINVAL
    assert so.cip_beam_taps(None, 3, buf.ctypes.data_as(PF64)) == _lib.CIP_EINVAL
    bad = _lib.Beam(a=0.1, b=0.2, c=0.1)
    assert so.cip_beam_taps(ctypes.byref(bad), 3, buf.ctypes.data_as(PF64)) == _lib.CIP_EINVAL
    assert not buf.any()
    with pytest.raises(ValueError, match="a, b and c"):
        rst.beam_taps({"fwhm_major": 3.0})


# ---- the argument checks of the device entry points come before the device -------
def test_argument_checks_come_before_the_device():
    so = _lib.lib()
    beam, out = _lib.Beam(a=0.1, b=0.0, c=0.1), _lib.Beam()
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused on its arguments
    other = ctypes.c_void_p(8192)
    for args in ((None, None, 4, 4, ctypes.byref(beam), 2, None, other), (fake, None, 4, 4, ctypes.byref(beam), 2, None, None),
                 (fake, None, 4, 4, None, 2, None, other), (fake, None, 4, 4, ctypes.byref(beam), 2, None, fake),
                 (fake, None, 0, 4, ctypes.byref(beam), 2, None, other), (fake, None, 4, -1, ctypes.byref(beam), 2, None, other),
                 (fake, None, 4, 4, ctypes.byref(beam), 33, None, other),
                 (fake, None, 4, 4, ctypes.byref(_lib.Beam(a=0.1, b=0.2, c=0.1)), 2, None, other)):
        assert so.cip_restore(*args) == _lib.CIP_EINVAL, args
        assert b"cip_restore" in so.cip_last_error()
    wide = _lib.Beam(a=1e-3, b=0.0, c=1e-3)  # radius < 0: from the beam, which needs more than 32 pixels
    assert so.cip_restore(fake, None, 4, 4, ctypes.byref(wide), -1, None, other) == _lib.CIP_ERANGE
    for args in ((None, 9, 9, -1, -1, 0.35, 8, None, ctypes.byref(out)), (fake, 9, 9, -1, -1, 0.35, 8, None, None),
                 (fake, 0, 9, -1, -1, 0.35, 8, None, ctypes.byref(out)), (fake, 9, 9, 9, 0, 0.35, 8, None, ctypes.byref(out)),
                 (fake, 9, 9, 0, -2, 0.35, 8, None, ctypes.byref(out)), (fake, 9, 9, -1, -1, 1.0, 8, None, ctypes.byref(out)),
                 (fake, 9, 9, -1, -1, 0.35, 0, None, ctypes.byref(out)), (fake, 9, 9, -1, -1, 0.35, 65, None, ctypes.byref(out))):
        assert so.cip_beam_fit(*args) == _lib.CIP_EINVAL, args
        assert b"cip_beam_fit" in so.cip_last_error()


def test_python_entry_points(monkeypatch):
    import torch

    import ska_sdp_cip_amd as pkg
    from ska_sdp_cip_amd import _call, deconvolve

    for name in ("device_restore", "device_fit_beam", "beam_from_fwhm", "beam_taps", "beam_to_sky"):
        assert getattr(pkg, name) is getattr(rst, name) and name in pkg.__all__, name
    assert callable(rst.restore) and callable(rst.beam_radius) and callable(rst.beam_fit_window)
    import inspect

    params = inspect.signature(deconvolve.device_major_cycles).parameters
    assert params["restore"].default is False and params["beam"].default is None
    monkeypatch.setattr(_call.torch.cuda, "is_available", lambda: False)
    beam = rst.beam_from_fwhm(3.0, 2.0, 0.1)  # the host-only ones need no GPU
    assert rst.beam_taps(beam, 2).shape == (5, 5)
    img = torch.zeros((4, 4), dtype=torch.float64)
    for fn, args in ((rst.device_restore, (img, None, beam)), (rst.restore, (np.zeros((4, 4)), None, beam)),
                     (rst.device_fit_beam, (img,))):
        with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
            fn(*args)
