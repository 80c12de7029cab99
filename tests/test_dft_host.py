"""
Host-side checks of the sky-model predict (no GPU): include/cip_dft.h against
`_lib.DFT_PROTOTYPES` and the `DFT_*` constants (the method of test_cal_host.py
on the fifth header), every CIP_EINVAL refused before the device, the numpy
statement `_dft_np` against `synthetic.predict_visibilities` and against its
own limits, and `skymodel.SkyModel` on CPU tensors.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _dft_np as dnp
from ska_sdp_cip_amd import _lib, mfs, skymodel, synthetic

HEADER = Path(__file__).resolve().parents[1] / "include" / "cip_dft.h"
SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "double": ctypes.c_double}
C = 299792458.0


@pytest.fixture(scope="module")
def header():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


@pytest.fixture(scope="module")
def rows():
    uvw = synthetic.uvw_tracks(120, 6, array_radius_m=3000.0, seed=5)
    return uvw, np.array([0.9e9, 1.0e9, 1.1e9, 1.25e9])


# ---- header against table ----------------------------------------------------
def test_every_prototype_matches_the_table(header):
    protos = {}
    for ret, name, params in re.findall(r"\b(int|const\s+char\s*\*)\s*(cip_\w+)\s*\(([^)]*)\)\s*;", header):
        protos[name] = (ret, [" ".join(p.split()) for p in params.split(",")])
    assert tuple(protos) == tuple(_lib.DFT_PROTOTYPES) == ("cip_dft_predict",)
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.DFT_PROTOTYPES[name]
        assert ret == "int" and restype is ctypes.c_int, name
        assert len(argtypes) == len(params) == 16, (name, len(argtypes), len(params))
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            if "*" in decl:
                assert argtype is ctypes.c_void_p, (name, k, decl)
            else:
                assert argtype is SCALARS[decl.replace("const", " ").split()[0]], (name, k, decl)
    assert '#include "cip.h"' in header and 'extern "C"' in header


def test_defines_match_the_binding(header):
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(CIP_\w+)\s+(\d+)", header)}
    assert defines == {"CIP_DFT_ADD": 1, "CIP_DFT_SUBTRACT": 2, "CIP_DFT_WTERM": 4, "CIP_DFT_FAST": 8}
    assert (_lib.DFT_ADD, _lib.DFT_SUBTRACT, _lib.DFT_WTERM, _lib.DFT_FAST) == (1, 2, 4, 8)
    assert _lib.DFT_MODES == {"set": 0, "add": 1, "subtract": 2}
    assert (dnp.FLAG_ADD, dnp.FLAG_SUBTRACT, dnp.FLAG_WTERM, dnp.FLAG_FAST) == (1, 2, 4, 8)
    assert dnp.MAX_TERMS == _lib.MFS_MAX_TERMS == 3 and dnp.C0 == synthetic.SPEED_OF_LIGHT


def test_library_exports_and_other_tables_unchanged():
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(so, "cip_dft_predict")
    for table in (_lib.PROTOTYPES, _lib.RESTORE_PROTOTYPES, _lib.MFS_PROTOTYPES, _lib.CAL_PROTOTYPES):
        assert "cip_dft_predict" not in table
    counts = [len(t) for t in (_lib.PROTOTYPES, _lib.RESTORE_PROTOTYPES, _lib.MFS_PROTOTYPES, _lib.CAL_PROTOTYPES)]
    assert counts == [41, 6, 1, 5]
    fn = _lib.lib().cip_dft_predict  # lib() applies all five tables
    restype, argtypes = _lib.DFT_PROTOTYPES["cip_dft_predict"]
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


# ---- every CIP_EINVAL comes before the device ----------------------------------
def test_argument_checks_come_before_the_device():
    so = _lib.lib()
    p = [ctypes.c_void_p(4096 * k) for k in range(1, 8)]  # never dereferenced: every call below is refused
    nan, inf = float("nan"), float("inf")

    def call(uvw=p[0], nrow=10, freq=p[1], nchan=4, lm=p[2], flux=p[3], shape=None, ncomp=3, nterms=1, ref=1e9,
             flags=0, wgt=p[4], wdt=_lib.CIP_F32, vis=p[5], vdt=_lib.CIP_C64):
        return so.cip_dft_predict(uvw, nrow, freq, nchan, lm, flux, shape, ncomp, nterms, ref, flags, wgt, wdt, None,
                                  vis, vdt)

    refused = [dict(nterms=0), dict(nterms=4), dict(nterms=-1), dict(nterms=2, ref=0.0), dict(nterms=2, ref=-1e9),
               dict(nterms=3, ref=nan), dict(nterms=2, ref=inf), dict(flags=_lib.DFT_ADD | _lib.DFT_SUBTRACT),
               dict(flags=16), dict(flags=1 << 20), dict(flags=-1), dict(vdt=_lib.CIP_F32), dict(vdt=_lib.CIP_NONE),
               dict(vdt=99), dict(wdt=_lib.CIP_C64), dict(wdt=99), dict(wgt=None), dict(wgt=p[4], wdt=_lib.CIP_NONE),
               dict(lm=None), dict(flux=None), dict(vis=None), dict(vis=None, ncomp=0, lm=None, flux=None),
               dict(uvw=None), dict(freq=None), dict(nrow=-1), dict(nchan=-1), dict(ncomp=-1)]
    for kw in refused:
        assert call(**kw) == _lib.CIP_EINVAL, kw
        assert b"cip_dft_predict" in so.cip_last_error(), kw
    # nothing to do: no device work, no error, whatever the pointers
    for kw in (dict(nrow=0, vis=None, uvw=None), dict(nchan=0, vis=None, freq=None),
               dict(ncomp=0, lm=None, flux=None, flags=_lib.DFT_ADD, vis=None),
               dict(ncomp=0, lm=None, flux=None, flags=_lib.DFT_SUBTRACT | _lib.DFT_WTERM),
               dict(nrow=0, ref=nan), dict(nrow=0, wgt=None)):
        assert call(**kw) == _lib.CIP_OK, kw


# ---- the numpy statement ---------------------------------------------------------
def test_statement_equals_predict_visibilities(rows):
    uvw, freq = rows
    rng = np.random.default_rng(2)
    srcs = synthetic.random_sources(7, 0.05, rng)
    ref = synthetic.predict_visibilities(uvw, freq, srcs)
    lm = [[s.l, s.m] for s in srcs]
    got, phi, sigma = dnp.predict(uvw, freq, lm, [[s.flux] for s in srcs], w_term=True)
    assert sigma == pytest.approx(sum(s.flux for s in srcs), rel=1e-14) and 1.0 < phi < 1e4
    # predict_visibilities takes the sine of the unreduced phase and forms n - 1 by subtraction
    assert np.abs(got - ref).max() <= sigma * (2 * np.pi * phi * 2.0 ** -49 + 1e-12)
    flat, _, _ = dnp.predict(uvw, freq, lm, [[s.flux] for s in srcs], w_term=False)
    assert np.abs(flat - ref).max() > 1e-6  # the w term is not a no-op on these rows


def test_zero_size_gaussian_is_a_point_and_a_gaussian_falls_off(rows):
    uvw, freq = rows
    lm, flux = [[0.01, -0.02], [0.0, 0.003]], [[1.5], [-0.5]]
    point, _, _ = dnp.predict(uvw, freq, lm, flux)
    zero, _, _ = dnp.predict(uvw, freq, lm, flux, shape=np.zeros((2, 3)))
    assert np.array_equal(point, zero)
    # one circular Gaussian at the centre: |V| = flux exp(-pi^2 theta^2 q^2 / (4 ln 2)), q = |uv| f / c
    theta = 2e-4
    got, _, _ = dnp.predict(uvw, freq, [[0.0, 0.0]], [[2.0]], shape=[[theta, theta, 0.7]])
    q2 = (uvw[:, 0] ** 2 + uvw[:, 1] ** 2)[:, None] * (freq / C)[None, :] ** 2
    assert np.allclose(got, 2.0 * np.exp(-np.pi ** 2 * theta ** 2 * q2 / (4 * np.log(2))), rtol=1e-12, atol=0)
    # position angle from +m towards +l: at pa = 0 the major axis lies along m, so a baseline along v resolves it
    line, _, _ = dnp.predict(np.array([[0.0, 1000.0, 0.0], [1000.0, 0.0, 0.0]]), freq[:1], [[0.0, 0.0]], [[1.0]],
                             shape=[[theta, 0.0, 0.0]])
    assert abs(line[0, 0]) < 0.9 and line[1, 0] == 1.0
    # left-out components
    skip, _, _ = dnp.predict(uvw, freq, [[0.01, -0.02], [0.8, 0.8], [np.nan, 0.0], [0.0, 0.003]],
                             [[1.5], [9.0], [9.0], [-0.5]])
    assert np.array_equal(skip, point)


def test_two_terms_are_the_first_order_expansion_of_a_power_law(rows):
    uvw, _ = rows
    ref_freq, alpha, s0 = 1.0e9, -0.7, 2.0
    freq = ref_freq * (1.0 + np.array([-0.04, -0.01, 0.0, 0.02, 0.05]))
    lm = [[0.004, 0.002]]
    two, _, sigma = dnp.predict(uvw, freq, lm, [[s0, s0 * alpha]], ref_freq=ref_freq)
    x = (freq - ref_freq) / ref_freq
    assert np.array_equal(dnp.spectra(np.array([[s0, s0 * alpha]]), freq, ref_freq)[0],
                          (mfs.taylor_basis(freq, ref_freq, 2) * np.array([[s0], [s0 * alpha]])).sum(axis=0))
    for c in range(len(freq)):  # channel by channel: a one-term source of flux s0 (1 + alpha x_c)
        one, _, _ = dnp.predict(uvw, freq[c:c + 1], lm, [[s0 * (1.0 + alpha * x[c])]])
        assert np.abs(two[:, c:c + 1] - one).max() <= 1e-15 * s0
    law, _, _ = dnp.predict(uvw, freq, lm, [[1.0]])
    law = law * (s0 * (freq / ref_freq) ** alpha)[None, :]
    # the remainder of the expansion: |alpha (alpha - 1) / 2| x^2 (1 + x)^(alpha - 2) at most
    bound = s0 * abs(alpha * (alpha - 1) / 2) * x ** 2 * (1.0 - 0.04) ** (alpha - 2)
    assert (np.abs(two - law).max(axis=0) <= bound + 1e-14).all() and np.abs(two - law).max() > 1e-4
    assert sigma == pytest.approx(s0 * (1 + abs(alpha) * 0.04))


def test_apply_rule():
    model = np.array([[1 + 2j, 3 - 1j, 0.5j]])
    wgt = np.array([[2.0, 0.0, 0.5]], dtype=np.float32)
    old = np.array([[1j, np.nan + 1j, 4.0]], dtype=np.complex64)
    assert np.array_equal(dnp.apply(model, old, wgt, "set"), np.array([[2 + 4j, 0, 0.25j]], dtype=np.complex64))
    add = dnp.apply(model, old, wgt, "add")
    assert add.dtype == np.complex64 and add[0, 0] == 2 + 5j and add[0, 2] == 4 + 0.25j
    assert add[0, 1:2].tobytes() == old[0, 1:2].tobytes()
    assert dnp.apply(model, old, None, "subtract")[0, 2] == 4 - 0.5j


# ---- SkyModel ----------------------------------------------------------------------
def test_skymodel_validation():
    lm, flux = torch.zeros((3, 2), dtype=torch.float64), torch.ones((3, 1), dtype=torch.float64)
    sky = skymodel.SkyModel(lm, flux)
    assert len(sky) == 3 and sky.nterms == 1 and sky.shape is None and sky.device == lm.device
    assert len(sky.to("cpu")) == 3
    two = skymodel.SkyModel(lm, torch.ones((3, 2), dtype=torch.float64), 1e9, torch.zeros((3, 3), dtype=torch.float64))
    assert two.nterms == 2 and two.ref_freq == 1e9 and two.to("cpu").ref_freq == 1e9
    bad = [
        lambda: skymodel.SkyModel(lm.numpy(), flux),
        lambda: skymodel.SkyModel(lm.float(), flux),
        lambda: skymodel.SkyModel(torch.zeros((3, 3), dtype=torch.float64), flux),
        lambda: skymodel.SkyModel(lm, torch.ones((2, 1), dtype=torch.float64)),
        lambda: skymodel.SkyModel(lm, torch.ones(3, dtype=torch.float64)),
        lambda: skymodel.SkyModel(lm, torch.ones((3, 4), dtype=torch.float64), 1e9),
        lambda: skymodel.SkyModel(lm, torch.ones((3, 0), dtype=torch.float64)),
        lambda: skymodel.SkyModel(lm, torch.ones((3, 2), dtype=torch.float64)),
        lambda: skymodel.SkyModel(lm, torch.ones((3, 2), dtype=torch.float64), 0.0),
        lambda: skymodel.SkyModel(lm, torch.ones((3, 2), dtype=torch.float64), float("nan")),
        lambda: skymodel.SkyModel(lm, flux, shape=torch.zeros((3, 2), dtype=torch.float64)),
        lambda: skymodel.SkyModel(lm, flux, shape=torch.zeros((3, 3), dtype=torch.float32)),
    ]
    for make in bad:
        with pytest.raises(ValueError):
            make()
    srcs = [synthetic.PointSource(0.01, -0.02, 1.5), synthetic.PointSource(0.0, 0.003, -0.5)]
    sky = skymodel.SkyModel.from_point_sources(srcs)
    assert np.array_equal(sky.lm.numpy(), [[0.01, -0.02], [0.0, 0.003]]) and sky.lm.dtype == torch.float64
    assert np.array_equal(sky.flux.numpy(), [[1.5], [-0.5]]) and sky.shape is None
    assert len(skymodel.SkyModel.from_point_sources([])) == 0
    taylor = skymodel.SkyModel.from_point_sources([synthetic.PointSource(0.0, 0.0, (1.0, -0.7))], ref_freq=1e9)
    assert taylor.nterms == 2 and np.array_equal(taylor.flux.numpy(), [[1.0, -0.7]])
    with pytest.raises(ValueError):
        skymodel.SkyModel.from_point_sources([synthetic.PointSource(0.0, 0.0, (1.0, -0.7))])


def test_skymodel_from_image_on_cpu_tensors():
    import dft_torch

    nx, ny, px, py = 10, 7, 2e-3, 3e-3
    img = torch.zeros((nx, ny), dtype=torch.float64)
    pixels = [(0, 0), (5, 3), (9, 6), (2, 5)]
    for n, (i, j) in enumerate(pixels):
        img[i, j] = (-1.0) ** n * (n + 1.0)
    img[7, 1] = 0.05  # below the threshold
    order = sorted(pixels)  # row-major
    l, m, nm1 = dft_torch._directions(order, nx, ny, px, py)  # pylint: disable=protected-access
    want = np.array([img[i, j].item() for i, j in order])
    flat = skymodel.SkyModel.from_image(img, px, py, False, threshold=0.1)
    assert len(flat) == 4 and flat.nterms == 1 and flat.shape is None
    assert np.array_equal(flat.lm.numpy(), np.stack([l, m], axis=1))
    assert np.array_equal(flat.flux.numpy()[:, 0], want)
    wide = skymodel.SkyModel.from_image(img, px, py, True, threshold=0.1)
    assert np.array_equal(wide.lm.numpy(), flat.lm.numpy())
    assert np.array_equal(wide.flux.numpy()[:, 0], want / (nm1 + 1.0))  # S = I / n
    off = [k for k, pix in enumerate(order) if pix != (nx // 2, ny // 2)]  # n < 1 everywhere but at the centre
    assert (np.abs(wide.flux.numpy()[off, 0]) > np.abs(want[off])).all() and len(off) == 3
    assert len(skymodel.SkyModel.from_image(img, px, py, False)) == 5  # threshold 0: every non-zero pixel
    assert len(skymodel.SkyModel.from_image(img, px, py, False, threshold=10.0)) == 0
    # Taylor terms: the union of the supports
    t1 = torch.zeros_like(img)
    t1[5, 3], t1[1, 1] = -0.7, 0.3
    sky = skymodel.SkyModel.from_image([img, t1], px, py, False, threshold=0.1, ref_freq=1.2e9)
    assert sky.nterms == 2 and len(sky) == 5 and sky.ref_freq == 1.2e9
    union = sorted(pixels + [(1, 1)])
    assert np.array_equal(sky.lm.numpy()[:, 0], [(i - nx // 2) * px for i, _ in union])
    assert np.array_equal(sky.flux.numpy(), [[img[i, j].item(), t1[i, j].item()] for i, j in union])
    with pytest.raises(ValueError):
        skymodel.SkyModel.from_image([img, t1], px, py, False)  # nterms > 1 needs ref_freq
    with pytest.raises(ValueError):
        skymodel.SkyModel.from_image(torch.zeros(4, dtype=torch.float64), px, py, False)
