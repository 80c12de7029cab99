"""
The workspace's cached host tables (cip_host.h `host_table`: the grid-correction
vectors, the FFT twiddles per length, the w-correction table) and its readback
staging across calls whose keys and sizes change.

A table goes up only when its key differs from the device copy's, through
pinned staging of its own and without a wait for the stream; a readback's
staging regrows when a call asks for more. Neither changes a number, so every
comparison is `torch.equal` against the same call through a fresh workspace
(`cip_release_workspace`): a table that did not follow its key, an upload that a
later stream overtook, or a read of freed staging shows as different bits.

Inputs are seeded and tiny (40 rows, 4 channels, epsilon 1e-4).
"""
import numpy as np
import pytest
import torch

from ska_sdp_cip_amd import _lib, calibrate
from ska_sdp_cip_amd import synthetic as syn
from ska_sdp_cip_amd.gridder import device_ms2dirty

pytestmark = pytest.mark.gpu

NROW, NCHAN, EPS = 40, 4, 1e-4


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _release():
    torch.cuda.synchronize()
    assert _lib.lib().cip_release_workspace() == 0


class Geometry:
    """One invert: its inputs on the device and the keywords of its call."""

    def __init__(self, dev, npix_x, npix_y, *, uvw_scale=1.0, seed=5, **kw):
        ms = syn.make_measurement_set(NROW, NCHAN, n_ant=16, array_radius_m=1000.0, seed=seed)
        uvw, f = ms.uvw() * uvw_scale, ms.channel_frequencies()
        rng = np.random.default_rng(seed)
        vis = (rng.standard_normal((NROW, NCHAN)) + 1j * rng.standard_normal((NROW, NCHAN))).astype(np.complex64)
        w = rng.uniform(0.5, 1.5, (NROW, NCHAN)).astype(np.float32)
        self.px = syn.pixel_size_for_grid(uvw, f, max(npix_x, npix_y))
        self.cols = (_t(uvw, dev), _t(f, dev), _t(vis, dev), _t(w, dev))
        self.npix = (npix_x, npix_y)
        self.kw = dict(epsilon=EPS, **kw)

    def image(self, **kw):
        img, prm = device_ms2dirty(*self.cols, *self.npix, self.px, self.px, **self.kw, **kw)
        return img, prm


def _fresh(g):
    _release()
    img, _ = g.image()
    return img


def _alternate(geoms, order):
    """Each geometry through a fresh workspace, then `order` through one workspace, then fresh again."""
    fresh = [_fresh(g) for g in geoms]
    _release()
    for k in order:
        assert torch.equal(geoms[k].image()[0], fresh[k]), f"geometry {k} in the order {order}"
    for k, g in enumerate(geoms):
        assert torch.equal(_fresh(g), fresh[k])


def test_correction_vectors_and_twiddles_follow_the_image_and_grid(gpu_device):
    a = Geometry(gpu_device, 64, 64)    # nu = nv = 128: pruned FFT, twiddles of one length
    b = Geometry(gpu_device, 96, 64)    # nu = 192: another cx, and no twiddles for it
    c = Geometry(gpu_device, 128, 64)   # nu = 256: a second twiddle length beside the first
    assert (a.image()[1].nu, b.image()[1].nu, c.image()[1].nu) == (128, 192, 256)
    img_a1, img_b = a.image()[0], b.image()[0]
    assert torch.equal(a.image()[0], img_a1)
    _alternate((a, b, c), (0, 1, 0, 2, 0, 1))
    assert float(img_a1.abs().max()) > 0.0 and float(img_b.abs().max()) > 0.0


def test_correction_vectors_follow_the_support(gpu_device):
    a = Geometry(gpu_device, 64, 64, support=6)
    b = Geometry(gpu_device, 64, 64, support=8)  # the same image and grid: only W differs in the key
    assert not torch.equal(a.image()[0], b.image()[0])
    _alternate((a, b), (0, 1, 0))


def test_w_correction_table(gpu_device):
    a = Geometry(gpu_device, 64, 64, do_wstacking=True)
    b = Geometry(gpu_device, 64, 64, do_wstacking=True, uvw_scale=3.0)  # another pixel size, so another nmin
    # the table is F on (0 .. dw |nmin|), and dw |nmin| is 1 / (2 sigma) up to its rounding, so W is what
    # changes its entries: the same pair with another support alternates two different tables
    c = Geometry(gpu_device, 64, 64, do_wstacking=True, support=6)
    d = Geometry(gpu_device, 64, 64, do_wstacking=True, support=8)
    assert a.image()[1].nmin != b.image()[1].nmin and a.image()[1].nplanes > 1
    _alternate((a, b), (0, 1, 0))
    _alternate((c, d), (0, 1, 0))


def test_no_wait_is_needed_behind_an_upload(gpu_device):
    a, b = Geometry(gpu_device, 64, 64), Geometry(gpu_device, 128, 64)
    fresh_a, fresh_b = _fresh(a), _fresh(b)
    _release()
    side = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(side):
        first, _ = a.image(synchronize=False)  # every table of A goes up here, and nothing waits for it
    second, _ = b.image(synchronize=True)      # at once, on the default stream
    with torch.cuda.stream(side):
        third, _ = a.image(synchronize=False)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(first, fresh_a) and torch.equal(second, fresh_b) and torch.equal(third, fresh_a)


def test_readback_staging_regrows_inside_a_call(gpu_device):
    n_ant = 4
    a1, a2, dump = syn.baseline_indices(NROW, n_ant)
    rng = np.random.default_rng(9)
    shape = (NROW, NCHAN)
    model = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    gains = syn.random_gains(1, n_ant, 0.2, 0.6, rng)[0]
    vis = (gains[a1][:, None] * model * np.conj(gains[a2])[:, None]).astype(np.complex64)
    wgt = rng.uniform(0.5, 1.5, shape).astype(np.float32)
    cols = [_t(x, gpu_device) for x in (vis, model, wgt, a1.astype(np.int32), a2.astype(np.int32))]
    one = _t(np.zeros(NROW, dtype=np.int32), gpu_device)
    per_dump = _t(dump.astype(np.int32), gpu_device)  # intervals past the last dump hold no sample

    def run(interval, n_int):
        g, ok, info = calibrate.device_gaincal(*cols, interval, n_ant, n_int, niter=30, tol=1e-9)
        return g, ok, info.pop("iters"), info

    def same(x, y):
        return all(torch.equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3]

    _release()
    fresh_many = run(per_dump, 40)
    _release()
    first = run(one, 1)        # the staging: a few words
    many = run(per_dump, 40)   # 40 intervals' solve statistics outgrow it inside the call
    again = run(one, 1)
    assert same(first, again) and same(many, fresh_many)
    assert first[3]["n_added"] == NROW * NCHAN and first[3]["n_dead"] == 0
    assert many[3]["n_added"] == NROW * NCHAN and many[0].shape == (40, n_ant)
