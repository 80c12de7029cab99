"""
GPU tests of the sky-model predict (`cip_dft_predict` through
`skymodel.device_dft_predict`) against the numpy statement of include/cip_dft.h,
`_dft_np`, at every sample.

Shapes are the smallest that reach a boundary of the kernel: a group of L
lanes (the least power of two with 4 L >= nchan, 64 at most) owns a row and a
lane 4 channels per pass, so nchan 1, 3, 4, 7 (L = 1, 1, 1, 2), 64 (L = 16) and
130 (L = 32, a partial last lane) on 168 rows, 2017 x 5 (an odd row count over
several workgroups) and 2048 * 256 + 5 rows of one channel: one more row block
than the 2048 workgroups of the grid-stride launch. Components are read at a
uniform index, with no tile: ncomp 0, 1, 5, 300.

Tolerances. fp64 class: with PHI the largest |phase| in cycles of the case
and SIGMA = max_c sum_k |S_k(c)|, |delta| <= |w| SIGMA (32 pi PHI 2^-52 + 1e-13)
plus one rounding of the output (2^-23 |V| for complex64, 2^-52 |V| for
complex128): both sides round the path in fp64, and the margin is a small
multiple of that rounding. Fast class: FAST_TOL SIGMA, see FAST_TOL below.
"""

import numpy as np
import pytest

import _dft_np as dnp
from ska_sdp_cip_amd import _call, _lib, gridder, skymodel, synthetic as syn
from test_oracle_accuracy import EXPECTED

pytestmark = pytest.mark.gpu

GRID_BLOCKS, BLOCK_THREADS = 2048, 256  # kDftMaxBlocks, kDftThreads of cip_dft.hip

# The fast class (CIP_DFT_FAST): 4 x the largest |delta| / SIGMA measured on the MI355X over fast_cases() below,
# the large-phase case included (the 4 x covers other inputs and clocks). The kept trig variant is the hardware
# sine and cosine: measured maximum 1.052e-7, against 7.95e-8 and 8.10e-8 for two fp32 polynomial sincospi
# (DESIGN.md 17 has the three and the times that decided between them).
FAST_MEASURED = 1.052e-7
FAST_TOL = 4.0 * FAST_MEASURED  # 4.2e-7, far inside the 1e-5 beyond which the class would not be worth having


def _t(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def geometry(nrow, nchan, seed=1):
    """`nrow` rows of an 8-antenna array (28 baselines a dump) and `nchan` channels from 1 GHz over 300 MHz."""
    return (syn.uvw_tracks(nrow, 8, array_radius_m=3000.0, dump_s=120.0, seed=seed),
            syn.channel_frequencies(nchan, 1.0e9, 0.3e9))


def components(ncomp, kind="points", nterms=1, seed=3, fov=0.1):
    """lm, flux (ncomp, nterms), shape (None for points; 'mix': every other row a point) and ref_freq."""
    rng = np.random.default_rng(seed)
    lm = rng.uniform(-fov / 2, fov / 2, (ncomp, 2))
    flux = rng.uniform(0.1, 1.0, (ncomp, nterms)) * rng.choice([-1.0, 1.0], (ncomp, nterms))
    shape = None
    if kind != "points":
        major = rng.uniform(1e-4, 4e-4, ncomp)
        shape = np.stack([major, major * rng.uniform(0.2, 1.0, ncomp), rng.uniform(-np.pi, np.pi, ncomp)], axis=1)
        if kind == "mix":
            shape[::2, :2] = 0.0
    return dict(lm=lm, flux=flux, shape=shape, ref_freq=1.1e9)


def sky_of(comp):
    return skymodel.SkyModel(_t(comp["lm"].reshape(-1, 2)), _t(comp["flux"]), comp["ref_freq"], _t(comp["shape"]))


def reference(uvw, freq, comp, w_term=True):
    return dnp.predict(uvw, freq, comp["lm"], comp["flux"], comp["shape"], comp["ref_freq"], w_term)


def gpu(uvw, freq, comp, wgt=None, **kw):
    out = kw.pop("out", None)
    res = skymodel.device_dft_predict(_t(uvw), _t(freq), sky_of(comp), _t(wgt), out=_t(out), **kw)
    return res.cpu().numpy()


def out_rounding(v):
    return (2.0 ** -23 if v.dtype == np.complex64 else 2.0 ** -52) * np.abs(v).astype(np.float64)


def check_fp64(got, model, phi, sigma, wgt=None, old=None, mode="set", what=""):
    """Every sample within the fp64-class bound of the statement; prints the largest error over the bound."""
    want = dnp.apply(model, np.zeros(model.shape, dtype=got.dtype) if old is None else old, wgt, mode)
    w = 1.0 if wgt is None else np.abs(wgt.astype(np.float64))
    bound = w * dnp.fp64_bound(phi, sigma) + out_rounding(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.complex128) - want.astype(np.complex128))
    live = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), live), what
    ratio = float((err[live] / np.maximum(bound[live], 1e-300)).max(initial=0.0))
    print(f"{what}: phi {phi:.4g} sigma {sigma:.4g} max|delta| {float(err[live].max(initial=0.0)):.3e} "
          f"max delta/bound {ratio:.3f}")
    assert ratio <= 1.0, what
    return want


# -------------------------------------------------------------------- shapes ----
@pytest.mark.parametrize("nchan", [1, 3, 4, 7, 64, 130])
def test_channel_counts(gpu_device, nchan):
    uvw, freq = geometry(168, nchan)
    comp = components(5)
    model, phi, sigma = reference(uvw, freq, comp)
    check_fp64(gpu(uvw, freq, comp), model, phi, sigma, what=f"168 x {nchan}")


def test_odd_rows_across_workgroups(gpu_device):
    uvw, freq = geometry(2017, 5)
    comp = components(5, "mix", 2)
    model, phi, sigma = reference(uvw, freq, comp)
    check_fp64(gpu(uvw, freq, comp), model, phi, sigma, what="2017 x 5")


def test_more_row_blocks_than_workgroups(gpu_device):
    nrow = GRID_BLOCKS * BLOCK_THREADS + 5  # one channel: 256 rows a workgroup, so one block more than the grid
    uvw = np.random.default_rng(8).uniform(-3000.0, 3000.0, (nrow, 3))
    freq = np.array([1.2e9])
    comp = components(2)
    model, phi, sigma = reference(uvw, freq, comp, True)
    got = gpu(uvw, freq, comp)
    check_fp64(got, model, phi, sigma, what=f"{nrow} x 1")
    assert np.abs(got[-5:]).min() > 0.0  # the rows of the second sweep are written


@pytest.mark.parametrize("ncomp", [0, 1, 5, 300])
def test_component_counts(gpu_device, ncomp):
    uvw, freq = geometry(168, 7)
    comp = components(ncomp, "mix" if ncomp else "points", 2)
    model, phi, sigma = reference(uvw, freq, comp)
    old = np.full(model.shape, np.nan + 1j, dtype=np.complex64)
    got = gpu(uvw, freq, comp, out=old.copy())
    check_fp64(got, model, phi, sigma, what=f"ncomp {ncomp}")
    if ncomp == 0:  # zeros by default (whatever the column held), a no-op under add and subtract
        assert got.tobytes() == np.zeros_like(old).tobytes()
        for mode in ("add", "subtract"):
            kept = gpu(uvw, freq, comp, out=old.copy(), mode=mode)
            assert kept.tobytes() == old.tobytes()
        empty = skymodel.SkyModel.from_point_sources([], device="cuda")
        assert float(skymodel.device_dft_predict(_t(uvw), _t(freq), empty).abs().max()) == 0.0


# ------------------------------------------------------------------ variants ----
def _weights(shape, dtype, seed=4):
    rng = np.random.default_rng(seed)
    wgt = rng.uniform(0.5, 1.5, shape)
    wgt[rng.uniform(size=shape) < 0.05] = 0.0
    wgt[0, 0] = wgt[-1, -1] = 0.0
    return wgt.astype(dtype)


@pytest.mark.parametrize("mode", ["set", "add", "subtract"])
@pytest.mark.parametrize("wdtype", [None, np.float32, np.float64])
@pytest.mark.parametrize("vdtype", [np.complex64, np.complex128])
def test_dtypes_weights_and_modes(gpu_device, vdtype, wdtype, mode):
    uvw, freq = geometry(168, 7)
    comp = components(5, "mix", 2)
    model, phi, sigma = reference(uvw, freq, comp)
    rng = np.random.default_rng(6)
    old = (rng.standard_normal(model.shape) + 1j * rng.standard_normal(model.shape)).astype(vdtype)
    wgt = None if wdtype is None else _weights(model.shape, wdtype)
    if wgt is not None:  # NaN data under some of the zero weights, and under one live sample
        zr, zc = np.nonzero(wgt == 0.0)
        old[zr[::2], zc[::2]] = np.nan
        old[3, 3] = np.nan if wgt[3, 3] != 0.0 else old[3, 3]
    got = gpu(uvw, freq, comp, wgt, out=old.copy(), mode=mode)
    want = check_fp64(got, model, phi, sigma, wgt, old, mode, what=f"{np.dtype(vdtype).name} {wdtype} {mode}")
    assert got.dtype == vdtype
    if wgt is not None:
        zero = wgt == 0.0
        assert zero.sum() >= 2
        if mode == "set":  # an exact 0
            assert got[zero].tobytes() == np.zeros(int(zero.sum()), dtype=vdtype).tobytes()
        else:  # the input bits, NaN included
            assert got[zero].tobytes() == old[zero].tobytes() == want[zero].tobytes()
    if mode == "set":  # without `out`: a new column of `dtype`
        import torch

        fresh = skymodel.device_dft_predict(_t(uvw), _t(freq), sky_of(comp), _t(wgt),
                                            dtype=torch.complex64 if vdtype == np.complex64 else torch.complex128)
        assert fresh.cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize("kind", ["points", "gauss", "mix"])
@pytest.mark.parametrize("nterms", [1, 2, 3])
@pytest.mark.parametrize("w_term", [True, False])
def test_w_term_terms_and_shapes(gpu_device, w_term, nterms, kind):
    import torch

    uvw, freq = geometry(168, 7)
    comp = components(6, kind, nterms)
    comp["lm"][2] = (0.8, 0.8)  # l^2 + m^2 > 1: left out under the w term, a plain direction without it
    comp["flux"][4, 0] = np.inf  # a non-finite field: left out either way
    model, phi, sigma = reference(uvw, freq, comp, w_term)
    gone = [2, 4] if w_term else [4]
    rest = dict(comp, lm=np.delete(comp["lm"], gone, axis=0), flux=np.delete(comp["flux"], gone, axis=0),
                shape=None if comp["shape"] is None else np.delete(comp["shape"], gone, axis=0))
    assert np.array_equal(model, reference(uvw, freq, rest, w_term)[0])
    got = gpu(uvw, freq, comp, w_term=w_term, dtype=torch.complex128)
    check_fp64(got, model, phi, sigma, what=f"w_term {w_term} nterms {nterms} {kind}")
    if kind == "gauss":  # the envelope matters on these baselines
        pts, _, _ = reference(uvw, freq, dict(comp, shape=None), w_term)
        assert np.abs(pts - model).max() > 0.05


# -------------------------------------------------------------- large phases ----
def large_phase_case():
    """Baselines of up to 150 km at 1.4 GHz and |l| up to 0.2: |phase| of about 1e5 cycles."""
    rng = np.random.default_rng(12)
    uvw = rng.uniform(-1.5e5, 1.5e5, (300, 3))
    uvw[:, 2] *= 0.1
    freq = np.array([1.40e9, 1.41e9, 1.42e9])
    comp = components(5, "points", 1, seed=9, fov=0.4)
    comp["lm"][0] = (0.2, -0.2)
    return uvw, freq, comp


@pytest.mark.parametrize("vdtype", [np.complex64, np.complex128])
def test_large_phases(gpu_device, vdtype):
    import torch

    uvw, freq, comp = large_phase_case()
    model, phi, sigma = reference(uvw, freq, comp)
    assert 5e4 < phi < 5e5
    got = gpu(uvw, freq, comp, dtype=torch.complex64 if vdtype == np.complex64 else torch.complex128)
    check_fp64(got, model, phi, sigma, what=f"large phases {np.dtype(vdtype).name}")


# ---------------------------------------------------------------- fast class ----
def fast_cases():
    """(name, uvw, freq, components, w_term) of the fast class's error measurement and test."""
    cases = []
    for nchan in (1, 3, 4, 7, 64, 130):
        cases.append((f"168x{nchan}", *geometry(168, nchan), components(5), True))
    cases.append(("2017x5", *geometry(2017, 5), components(5, "mix", 2), True))
    for kind in ("points", "gauss", "mix"):
        for nterms in (1, 2, 3):
            cases.append((f"{kind}-T{nterms}", *geometry(168, 7), components(6, kind, nterms), nterms != 2))
    cases.append(("ncomp300", *geometry(168, 7), components(300, "mix", 2), True))
    cases.append(("large-phases", *large_phase_case(), True))
    return cases


def fast_error(name, uvw, freq, comp, w_term):
    """max |delta| / SIGMA of one case, complex128 output without weights."""
    import torch

    model, _, sigma = reference(uvw, freq, comp, w_term)
    sky = sky_of(comp)
    out = torch.empty(model.shape, dtype=torch.complex128, device="cuda")
    flags = _lib.DFT_FAST | (_lib.DFT_WTERM if w_term else 0)
    _call.call(out.device, "cip_dft_predict", _t(uvw), len(uvw), _t(freq), len(freq), sky.lm, sky.flux, sky.shape,
               len(sky), sky.nterms, float(sky.ref_freq), flags, None, _lib.CIP_NONE, _call.STREAM,
               *_call.vis_arg(out))
    return float(np.abs(out.cpu().numpy() - model).max() / sigma)


def test_fast_class_error(gpu_device):
    worst = 0.0
    for case in fast_cases():
        err = fast_error(*case)
        print(f"fast class {case[0]}: max|delta| / sigma = {err:.3e}")
        worst = max(worst, err)
    print(f"fast class: worst {worst:.3e}, bound {FAST_TOL}")
    assert FAST_TOL <= 1e-5 and worst <= FAST_TOL


def test_fast_class_through_the_wrapper(gpu_device):
    uvw, freq = geometry(168, 7)
    comp = components(5, "mix", 2)
    model, _, sigma = reference(uvw, freq, comp)
    wgt = _weights(model.shape, np.float32)
    got = gpu(uvw, freq, comp, wgt, fast=True)
    want = dnp.apply(model, np.zeros(model.shape, dtype=np.complex64), wgt, "set")
    assert got.dtype == np.complex64
    assert (np.abs(got - want) <= wgt * FAST_TOL * sigma + out_rounding(want)).all()
    assert got[wgt == 0.0].tobytes() == want[wgt == 0.0].tobytes()
    exact = gpu(uvw, freq, comp, wgt)
    assert got.tobytes() != exact.tobytes()  # the flag selects another kernel


# ---------------------------------------------------------------------- bits ----
@pytest.mark.parametrize("fast", [False, True])
def test_bits_repeat_and_row_splits(gpu_device, fast):
    uvw, freq = geometry(2017, 5)
    comp = components(7, "mix", 3)
    wgt = _weights((2017, 5), np.float32)
    rng = np.random.default_rng(2)
    old = (rng.standard_normal((2017, 5)) + 1j * rng.standard_normal((2017, 5))).astype(np.complex64)
    for mode in ("set", "add"):
        one = gpu(uvw, freq, comp, wgt, out=old.copy(), mode=mode, fast=fast)
        again = gpu(uvw, freq, comp, wgt, out=old.copy(), mode=mode, fast=fast)
        assert one.tobytes() == again.tobytes(), mode
        parts = [gpu(uvw[a:b], freq, comp, wgt[a:b], out=old[a:b].copy(), mode=mode, fast=fast)
                 for a, b in ((0, 33), (33, 1000), (1000, 2017))]  # odd boundaries
        assert np.concatenate(parts).tobytes() == one.tobytes(), mode


# ------------------------------------------------- against the degridder ----
@pytest.mark.parametrize("wstack", [False, True])
def test_image_components_against_the_degridder(gpu_device, wstack):
    import torch

    uvw = syn.uvw_tracks(3_000, 16, array_radius_m=1000.0, seed=1)
    freq = syn.channel_frequencies(2)
    npix, support = 64, 8
    px = syn.pixel_size_for_grid(uvw, freq, npix, fill=0.8)
    img = np.zeros((npix, npix))
    for (i, j), v in (((32, 32), 1.0), ((3, 60), -0.7), ((50, 9), 0.4), ((63, 63), 0.25), ((17, 40), 2.0)):
        img[i, j] = v
    sky = skymodel.SkyModel.from_image(_t(img), px, px, wstack)
    assert len(sky) == 5 and sky.lm.is_cuda
    got = skymodel.device_dft_predict(_t(uvw), _t(freq), sky, w_term=wstack, dtype=torch.complex128).cpu().numpy()
    deg, _ = gridder.device_dirty2ms(_t(uvw), _t(freq), _t(img), None, px, px, support=support, do_wstacking=wstack)
    err = float(np.abs(got - deg.cpu().numpy()).max() / np.abs(img).sum())
    print(f"dft predict vs dirty2ms W={support} wstack={wstack}: {err:.3e}")
    assert err < EXPECTED[support], err


# ---------------------------------------------------------------- validation ----
def test_every_einval_is_a_value_error_with_the_library_message(gpu_device):
    import torch

    uvw, freq = geometry(28, 3)
    comp = components(2, "mix", 2)
    sky, u, f = sky_of(comp), _t(uvw), _t(freq)
    out = torch.zeros((28, 3), dtype=torch.complex64, device="cuda")
    wgt = torch.ones((28, 3), dtype=torch.float32, device="cuda")
    nan = float("nan")

    def call(uvw=u, nrow=28, freq=f, nchan=3, lm=sky.lm, flux=sky.flux, shape=sky.shape, ncomp=2, nterms=2, ref=1.1e9,
             flags=0, wgt=wgt, wdt=_lib.CIP_F32, vis=out, vdt=_lib.CIP_C64):
        _call.call(out.device, "cip_dft_predict", uvw, nrow, freq, nchan, lm, flux, shape, ncomp, nterms, ref, flags,
                   wgt, wdt, _call.STREAM, vis, vdt)

    call()
    torch.cuda.synchronize()
    good = out.clone()
    assert float(good.abs().max()) > 0.0
    for kw in (dict(nterms=0), dict(nterms=4), dict(ref=0.0), dict(ref=-1.0), dict(ref=nan), dict(ref=float("inf")),
               dict(flags=_lib.DFT_ADD | _lib.DFT_SUBTRACT), dict(flags=16), dict(flags=1 << 12),
               dict(vdt=_lib.CIP_F64), dict(vdt=77), dict(wdt=_lib.CIP_C128), dict(wdt=77), dict(wgt=None),
               dict(wdt=_lib.CIP_NONE), dict(lm=None), dict(flux=None), dict(vis=None),
               dict(vis=None, ncomp=0, lm=None, flux=None), dict(nrow=-1), dict(ncomp=-1)):
        with pytest.raises(ValueError, match="cip_dft_predict"):
            call(**kw)
    torch.cuda.synchronize()
    assert torch.equal(out, good)  # a refused call writes nothing
    call(nterms=1, ref=nan, flux=sky.flux[:, :1].contiguous())  # ref_freq is not read with one term
    # the wrapper's own checks
    with pytest.raises(ValueError, match="mode"):
        skymodel.device_dft_predict(u, f, sky, mode="replace")
    with pytest.raises(ValueError, match="needs `out`"):
        skymodel.device_dft_predict(u, f, sky, mode="add")
    with pytest.raises(ValueError):
        skymodel.device_dft_predict(u, f, sky, wgt[:, :2].contiguous())
    with pytest.raises(ValueError):
        skymodel.device_dft_predict(u, f, sky.to("cpu"))


def test_numpy_front_end(gpu_device):
    import torch

    uvw, freq = geometry(168, 4)
    comp = components(3, "gauss", 1)
    model, phi, sigma = reference(uvw, freq, comp)
    sky = skymodel.SkyModel(torch.from_numpy(comp["lm"]), torch.from_numpy(comp["flux"]),
                            shape=torch.from_numpy(comp["shape"]))  # on the host: the front end moves it
    got = skymodel.dft_predict(uvw, freq, sky)
    assert isinstance(got, np.ndarray) and got.dtype == np.complex64
    check_fp64(got, model, phi, sigma, what="dft_predict")
    old = np.ones(model.shape, dtype=np.complex128)
    sub = skymodel.dft_predict(uvw, freq, sky, out=old, mode="subtract")
    assert (old == 1.0).all()
    check_fp64(sub, model, phi, sigma, old=old, mode="subtract", what="dft_predict subtract")
