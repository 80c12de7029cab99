"""
Facet mosaicking on the GPU (cip_mosaic_add, cip_mosaic_finish; mosaic.py and
continuum_invert(mosaic=...)) against the numpy statement `_mosaic_np`.

The kernel test resamples standard-normal facets (pure resampling: the values
do not matter, every pixel is independent). Its bounds are derived, not
measured: a facet coordinate of up to 256 pixels carries at most 2e-13 pixels
of rounding (the sqrt and a handful of rounded operations at 1.1e-16 each), an
interpolant of data bounded by max |facet| has a slope of at most pi max per
pixel, so the two sides differ by at most 7e-13 max |facet| from the
coordinates, and the tap arithmetic (exp, sinpi, fused multiply-adds) is of the
1e-14 class: 1e-11 max |facet| leaves more than a factor of 10. The weight is
a product of two ramps of slope <= 1 per pixel: 1e-13 on wsum.

Both paths of the kernel (the tile's facet window staged in LDS, and direct
loads; CIP_MOSAIC_LDS is read per call) are held to the same statement.
"""
import itertools

import numpy as np
import pytest

import _mosaic_np as mnp
import _mosaic_scene as sc
import oracle
from ska_sdp_cip_amd import _lib
from ska_sdp_cip_amd.continuum import continuum_invert, continuum_mosaic_invert
from ska_sdp_cip_amd.mosaic import MosaicAccumulator, device_mosaic, mosaic_beta

pytestmark = pytest.mark.gpu

NX, NY, FNX, FNY = 64, 48, 40, 36  # both non-square: a transposition shows
# (px, py, facet centres): a field of small angles with off-pixel centres, one of them hanging off the
# plane's corner; and a field of large pixels with a strongly rotated facet at l0 = 0.5
FIELDS = [
    (2.0e-3, 2.3e-3, [(0.01131, -0.00717), (-0.02049, 0.01333), (0.0551, 0.0443)]),
    (1.6e-2, 1.7e-2, [(0.5, 0.0931), (-0.2413, -0.3077)]),
]
OPTIONS = list(itertools.product((1, 3), (0, 3), (0.0, 5.0), (False, True)))  # nplane, trim, feather, nscale


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _geom(px, py, half, trim, feather, nscale, nx=NX, ny=NY, fnx=FNX, fny=FNY, ratio=0.8):
    return mnp.Geom(nx, ny, px, py, fnx, fny, ratio * px, ratio * px, half, mnp.beta_rule(half, 0.2), trim, feather,
                    mnp.NSCALE if nscale else 0)


def _accumulator(g, nplane):
    return MosaicAccumulator(g.nx, g.ny, g.px, g.py, nplane, half=g.half, beta=g.beta, trim=g.trim,
                             feather=g.feather, nscale=bool(g.flags & mnp.NSCALE))


@pytest.fixture(scope="module")
def facets():
    return np.random.default_rng(20).standard_normal((3, 3, FNX, FNY))  # (facet, plane, fnx, fny)


@pytest.mark.parametrize("nplane,trim,feather,nscale", OPTIONS)
@pytest.mark.parametrize("half", [2, 6, 8])
def test_kernel_equals_the_numpy_statement(gpu_device, facets, monkeypatch, half, nplane, trim, feather, nscale):
    worst = 0.0
    for px, py, centres in FIELDS:
        g = _geom(px, py, half, trim, feather, nscale)
        num, wsum = np.zeros((nplane, NX, NY)), np.zeros((NX, NY))
        for f, c in zip(facets, centres):
            x, y, _, _ = mnp.coords(g, *c)
            dx, dy = mnp.margins(g, x, y)
            assert min(np.abs(dx).min(), np.abs(dy).min()) >= 1e-9  # no pixel sits on the boundary
            mnp.add(g, f[:nplane], c[0], c[1], num, wsum)
        assert 0 < (wsum > 0).sum() < NX * NY
        ref, ref_missed = mnp.finish(num, wsum, fill=-7.0)
        for lds in ("1", "0"):
            monkeypatch.setenv("CIP_MOSAIC_LDS", lds)
            acc = _accumulator(g, nplane)
            for f, c in zip(facets, centres):
                acc.add(_dev(f[:nplane]), c[0], c[1], (g.fpx, g.fpy))
            got_wsum = acc.wsum.cpu().numpy()
            assert np.array_equal(got_wsum > 0, wsum > 0), (lds, "the covered sets differ")
            assert np.abs(got_wsum - wsum).max() <= 1e-13, lds
            got_num = acc.num.cpu().numpy()
            assert np.abs(got_num - num).max() <= 1e-11 * np.abs(facets).max() * len(centres), lds
            got, missed = acc.finish(fill=-7.0)
            err = float(np.abs(got.cpu().numpy() - ref).max())
            worst = max(worst, err)
            assert missed == ref_missed, lds
            assert err <= 1e-11 * np.abs(facets).max(), (lds, err)
    print(f"max |kernel - numpy| = {worst:.2e} (max |facet| = {np.abs(facets).max():.2f})")


def test_edge_shapes(gpu_device, facets):
    import torch

    px = 2.0e-3
    # (nx, ny, fnx, fny, centre): one pixel; not a multiple of the tile; a facet larger than the plane
    for nx, ny, fnx, fny, c in ((1, 1, FNX, FNY, (0.00031, -0.00047)), (17, 33, FNX, FNY, (0.00131, 0.00717)),
                                (9, 7, FNX, FNY, (0.00031, -0.00047)), (33, 17, 36, 40, (-0.0071, 0.0013))):
        g = _geom(px, 1.1 * px, 6, 0, 2.0, True, nx=nx, ny=ny, fnx=fnx, fny=fny)
        f = facets[0, :2].reshape(2, -1)[:, :fnx * fny].reshape(2, fnx, fny)
        ref, ref_missed = mnp.mosaic(g, [f], [c], fill=-7.0)
        acc = _accumulator(g, 2)
        acc.add(_dev(f), *c, (g.fpx, g.fpy))
        got, missed = acc.finish(fill=-7.0)
        assert missed == ref_missed and missed < nx * ny, (nx, ny)
        assert np.abs(got.cpu().numpy() - ref).max() <= 1e-11 * np.abs(f).max(), (nx, ny)
    # a facet entirely outside the plane: a no-op; finish reports everything uncovered and writes `fill`
    g = _geom(px, 1.1 * px, 6, 0, 0.0, False, nx=17, ny=33)
    acc = _accumulator(g, 2)
    acc.num.fill_(3.0)
    for c in ((0.7, 0.1), (-0.2, -0.6), (0.0, 0.2)):
        acc.add(_dev(facets[0, :2]), *c, (g.fpx, g.fpy))
    assert float(acc.wsum.abs().max()) == 0.0 and float((acc.num - 3.0).abs().max()) == 0.0
    got, missed = acc.finish(fill=-7.0)
    assert missed == 17 * 33
    assert torch.equal(got, torch.full_like(got, -7.0))
    acc = _accumulator(g, 1)
    got, missed = acc.finish()
    assert missed == 17 * 33 and bool(torch.isnan(got).all())
    with pytest.raises(RuntimeError, match="finish"):
        acc.add(_dev(facets[0, 0]), 0.0, 0.0)


@pytest.mark.parametrize("half", [2, 6, 8])
def test_a_facet_of_ones_keeps_the_flux(gpu_device, half):
    import torch

    ones = torch.ones((1, FNX, FNY), dtype=torch.float64, device=gpu_device)
    for px, py, centres in FIELDS:
        for feather in (0.0, 5.0):
            g = _geom(px, py, half, 0, feather, False)
            acc = _accumulator(g, 1)
            for c in centres:
                acc.add(ones, *c, (g.fpx, g.fpy))
            covered = (acc.wsum > 0).cpu().numpy()
            got, _ = acc.finish()
            dev = np.abs(got.cpu().numpy()[0][covered] - 1.0).max()
            assert covered.any() and dev <= 4 * np.spacing(1.0), (px, feather, dev / np.spacing(1.0))


def test_identity_on_the_same_grid(gpu_device, facets):
    # centre (0, 0), the facet's own grid, trim 0: x = i exactly (a pixel size that is a power of two, so
    # (i px) / px is exact), the taps are a delta and the valid interior is the facet itself
    px = 2.0**-9
    for half in (2, 6, 8):
        g = mnp.Geom(FNX, FNY, px, px, FNX, FNY, px, px, half, mnp.beta_rule(half, 0.2))
        got, missed = device_mosaic([_dev(facets[0])], [(0.0, 0.0)], FNX, FNY, px, half=half, beta=g.beta, fill=0.0)
        got = got.cpu().numpy()
        lo_x, hi_x, lo_y, hi_y = mnp.bounds(g)
        inner = facets[0][:, lo_x:hi_x + 1, lo_y:hi_y + 1]
        assert missed == FNX * FNY - inner[0].size
        assert np.abs(got[:, lo_x:hi_x + 1, lo_y:hi_y + 1] - inner).max() <= 1e-15 * np.abs(inner).max()
        outside = np.ones((FNX, FNY), bool)
        outside[lo_x:hi_x + 1, lo_y:hi_y + 1] = False
        assert not got[:, outside].any()


def test_two_accumulators_sum_to_the_one_shot(gpu_device):
    pix = 2.0e-3
    cen = [(-0.021, -0.017), (-0.019, 0.018), (0.02, -0.016), (0.022, 0.019)]
    fac = np.random.default_rng(21).standard_normal((4, 2, FNX, FNY))
    kw = dict(half=6, nu_max=0.2, trim=1, feather=4.0, nscale=True)
    one, missed = device_mosaic([_dev(f) for f in fac], cen, NX, NY, pix, 1.1 * pix, facet_pixel_size=0.8 * pix, **kw)
    a, b = (MosaicAccumulator(NX, NY, pix, 1.1 * pix, 2, **kw) for _ in range(2))
    for k in (0, 2):
        a.add(_dev(fac[k]), *cen[k], 0.8 * pix)
    for k in (1, 3):
        b.add(_dev(fac[k]), *cen[k], 0.8 * pix)
    assert a.num_facets == b.num_facets == 2
    a.num += b.num
    a.wsum += b.wsum
    a.reduce()  # no process group: nothing
    both, missed2 = a.finish()
    assert missed2 == missed < NX * NY
    covered = ~np.isnan(one.cpu().numpy())
    assert np.array_equal(covered, ~np.isnan(both.cpu().numpy()))
    assert np.abs(both.cpu().numpy()[covered] - one.cpu().numpy()[covered]).max() <= 1e-13 * np.abs(fac).max()


def test_end_to_end_against_the_dft(gpu_device):
    """continuum_invert(mosaic=(64, 64)) on the scene of `_mosaic_scene` against
    oracle.dft_dirty(apply_w=True): no worse than the numpy statement over the
    oracle's facets (the method's own error) plus 1e-9 of the weight sum, the
    gridder's 1e-10 parity gate through taps whose absolute sum is below 10."""
    uvw, freq, vis, asec, pix = sc.scene()
    cen = sc.centres(6)
    vis4 = np.zeros(vis.shape + (4,), np.complex64)
    vis4[..., 0] = vis4[..., 3] = vis  # XX = YY = I
    wgt4 = np.ones(vis4.shape, np.float32)
    flags4 = np.zeros(vis4.shape, np.uint8)
    vis_i, eff = oracle.stokes(vis4, flags4.astype(bool), wgt4, "I")
    assert np.array_equal(vis_i, vis) and np.ptp(eff) == 0  # so both sides are the unit-weight image over sum w
    err_ref, missed_ref = sc.method_error(6, store_complex64=True)
    assert missed_ref == 0
    d = [_dev(a) for a in (vis4, flags4, wgt4, uvw, freq)]
    out = continuum_invert(*d, sc.FACET, asec, facets=cen, stokes="I", psf=False, support=sc.SUPPORT,
                           do_wstacking=True, mosaic=(sc.NPIX, sc.NPIX), mosaic_half=6, mosaic_nu_max=sc.NU)
    assert set(out) == {("I", k) for k in range(len(cen))} | {("I", "mosaic"), ("uncovered", "mosaic")}
    assert out[("uncovered", "mosaic")] == 0
    err_gpu = float(np.abs(out[("I", "mosaic")].cpu().numpy() - sc.reference()).max())
    print(f"max |mosaic - DFT| / sum w: GPU {err_gpu:.3e}, numpy statement over oracle facets {err_ref:.3e}")
    assert err_gpu <= err_ref + 1e-9
    # the default band limit is the data's: the longest |u| or |v| in cycles per pixel
    auto = continuum_invert(*d, sc.FACET, asec, facets=cen, stokes="I", psf=False, support=sc.SUPPORT,
                            do_wstacking=True, mosaic=(sc.NPIX, sc.NPIX), keep_facets=False)
    assert set(auto) == {("I", "mosaic"), ("uncovered", "mosaic")}
    assert float((auto[("I", "mosaic")] - out[("I", "mosaic")]).abs().max()) <= 1e-9
    # the one call: layout, invert, mosaic
    res = continuum_mosaic_invert(*d, sc.NPIX, sc.NPIX, sc.FACET, asec, stokes="I", support=sc.SUPPORT,
                                  mosaic_nu_max=sc.NU)
    assert set(res) == {"I", "uncovered"} and res["uncovered"] == 0
    assert float((res["I"] - out[("I", "mosaic")]).abs().max()) <= 1e-12


def test_every_refusal_is_a_value_error(gpu_device, facets):
    import torch

    f = _dev(facets[0, :1])
    base = dict(nx=NX, ny=NY, px=2e-3, py=2.3e-3, nplane=1, half=6, nu_max=0.2)

    def add(facet=f, l0=0.01, m0=0.02, size=1.6e-3, **kw):
        MosaicAccumulator(**{**base, **kw}).add(facet, l0, m0, size)

    add()
    for kw in (dict(l0=0.8, m0=0.6), dict(l0=1.5), dict(m0=float("nan")), dict(size=0.0), dict(size=float("inf")),
               dict(size=(1e-3, -1e-3)), dict(facet=f[:, :11]), dict(facet=f[:, :, :11]), dict(trim=13),
               dict(facet=f[:, :24, :24].contiguous(), trim=7), dict(facet=f.float()), dict(facet=f.cpu()),
               dict(facet=f[:, ::2]), dict(facet=_dev(facets[0, :2]))):
        with pytest.raises(ValueError):
            add(**kw)
    # the C entry points, with device pointers: each refusal of the header
    so = _lib.lib()
    num, wsum = torch.zeros((1, NX, NY), dtype=torch.float64, device=gpu_device), torch.zeros(
        (NX, NY), dtype=torch.float64, device=gpu_device)
    import ctypes

    def raw(l0=0.01, m0=0.02, nplane=1, facet=f.data_ptr(), **kw):
        g = _lib.MosaicGeom(**{**dict(nx=NX, ny=NY, px=2e-3, py=2.3e-3, fnx=FNX, fny=FNY, fpx=1.6e-3, fpy=1.6e-3,
                                      half=6, flags=0, beta=mosaic_beta(6, 0.2), trim=0, feather=0.0), **kw})
        _lib.check(so.cip_mosaic_add(ctypes.byref(g), facet, nplane, l0, m0, None, num.data_ptr(), wsum.data_ptr()))

    raw()
    torch.cuda.synchronize()
    before = (num.clone(), wsum.clone())
    for kw in (dict(nx=0), dict(fny=0), dict(nplane=0), dict(facet=None), dict(px=0.0), dict(fpy=float("nan")),
               dict(half=1), dict(half=9), dict(beta=-1.0), dict(beta=float("inf")), dict(trim=-1),
               dict(feather=-1.0), dict(feather=float("nan")), dict(flags=2), dict(l0=0.8, m0=0.6),
               dict(px=0.03, py=0.03), dict(fnx=11), dict(trim=13), dict(nx=1 << 62, ny=4)):
        with pytest.raises(ValueError, match="cip_mosaic_add"):
            raw(**kw)
    missed = ctypes.c_int64(0)
    for args in ((None, wsum.data_ptr(), 1, NX, NY), (num.data_ptr(), None, 1, NX, NY),
                 (num.data_ptr(), wsum.data_ptr(), 0, NX, NY), (num.data_ptr(), wsum.data_ptr(), 1, 0, NY),
                 (num.data_ptr(), wsum.data_ptr(), 1, 1 << 62, 4)):
        with pytest.raises(ValueError, match="cip_mosaic_finish"):
            _lib.check(so.cip_mosaic_finish(*args, 0.0, None, ctypes.byref(missed)))
    with pytest.raises(ValueError, match="cip_mosaic_finish"):
        _lib.check(so.cip_mosaic_finish(num.data_ptr(), wsum.data_ptr(), 1, NX, NY, 0.0, None, None))
    torch.cuda.synchronize()
    assert torch.equal(num, before[0]) and torch.equal(wsum, before[1])  # a refused call touches nothing
