"""
The call scope and the plan pipeline of the host API (cip_host.h `Call`,
`PlanScope`, `GridZero`) across streams, call kinds and an early return.

A call that only queues its kernels leaves workspace buffers in use: the scope
notes its stream on every return path, and a call on another stream waits for
it before it rewrites them. Pipelined inverts alternate two sets of planner
buffers and share one grid with every other invert and with the predict. None
of this changes a number, so every comparison is `torch.equal` against the same
call through a fresh workspace (`cip_release_workspace`), after two fresh runs
of that call were seen to agree; only the packed class, whose float atomics are
not bit-reproducible, is held to 1e-6 of its peak (the bound of
test_gpu_grid_f32.py). A wrong order shows as different numbers, never as a
fault: no buffer in these sequences is freed or resized while in use.

Inputs are seeded and tiny.
"""
import numpy as np
import pytest
import torch

from ska_sdp_cip_amd import _lib, skymodel, strips, weighting
from ska_sdp_cip_amd import synthetic as syn
from ska_sdp_cip_amd.gridder import device_dirty2ms, device_ms2dirty

pytestmark = pytest.mark.gpu

NROW, NCHAN = 40, 4


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _release():
    torch.cuda.synchronize()
    assert _lib.lib().cip_release_workspace() == 0


def _fresh(fn):
    """`fn()` through a fresh workspace, twice: the two must agree bit for bit."""
    _release()
    one = fn()
    _release()
    two = fn()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(one, two)), "two fresh-workspace runs differ"
    return one


def _busy(dev):
    """Some tens of milliseconds of unrelated work on the current stream."""
    a = torch.ones((8192, 8192), dtype=torch.float32, device=dev)
    for _ in range(8):
        a = (a @ a) * 1e-4
    return a


# ------------------------------------------- queued-only entry points ----
def _rows(seed, scale=1.0):
    ms = syn.make_measurement_set(NROW, NCHAN, n_ant=16, array_radius_m=1000.0, seed=seed)
    return ms.uvw() * scale, ms.channel_frequencies()


def _dft_pair(dev):
    uvw, f = _rows(5)
    tu, tf = _t(uvw, dev), _t(f, dev)
    rng = np.random.default_rng(11)

    def sky():
        lm = rng.uniform(-0.02, 0.02, (6, 2))
        return skymodel.SkyModel(_t(lm, dev), _t(rng.uniform(0.5, 2.0, (6, 1)), dev))

    return [lambda s=s: (skymodel.device_dft_predict(tu, tf, s),) for s in (sky(), sky())]


def _grid128(uvw, f):
    px = syn.pixel_size_for_grid(uvw, f, 64)
    prm = _lib.choose_params(64, 64, px, px, 1e-4, 8)
    assert prm.nv == 128
    return prm, px


def _histogram_pair(dev):
    (uvw_a, f), (uvw_b, _) = _rows(5), _rows(6, 0.7)
    prm, px = _grid128(uvw_a, f)
    tf = _t(f, dev)
    return [lambda u=_t(u, dev): tuple(strips.strip_histogram(u, tf, prm, px, px)) for u in (uvw_a, uvw_b)]


def _split_pair(dev):
    # cip_strip_split's emit phase (the count phase ends in a readback)
    (uvw_a, f), (uvw_b, _) = _rows(5), _rows(6, 0.7)
    prm, px = _grid128(uvw_a, f)
    tf = _t(f, dev)
    rng = np.random.default_rng(3)
    vis = _t((rng.standard_normal((NROW, NCHAN)) + 1j * rng.standard_normal((NROW, NCHAN))).astype(np.complex64), dev)
    wgt = _t(rng.uniform(0.5, 1.5, (NROW, NCHAN)).astype(np.float32), dev)
    # pylint: disable-next=protected-access
    return [lambda u=_t(u, dev): strips._split_device(u, tf, prm, px, 0, 128, vis, wgt) for u in (uvw_a, uvw_b)]


def _weight_apply_pair(dev):
    # cip_weight_apply reads the reciprocal wavelengths the call itself put into the workspace
    uvw, f = _rows(5)
    px = syn.pixel_size_for_grid(uvw, f, 64)
    tu, tf = _t(uvw, dev), _t(f, dev)
    wgt = _t(np.random.default_rng(4).uniform(0.5, 1.5, (NROW, NCHAN)).astype(np.float32), dev)
    wd = weighting.WeightDensity(64, 64, px, px, 1.5, NROW * NCHAN, dev)
    wd.add_ms(tu, tf, wgt)
    wd.add_ms(tu, tf * 0.8, wgt)
    wd.finish("uniform")
    return [lambda fr=fr: (wd.apply(tu, fr, wgt),) for fr in (tf, tf * 0.8)]


@pytest.mark.parametrize("first", ["side", "default"])
@pytest.mark.parametrize("pair", [_dft_pair, _histogram_pair, _split_pair, _weight_apply_pair],
                         ids=["dft_predict", "strip_histogram", "strip_split", "weight_apply"])
def test_queued_call_then_another_stream(gpu_device, pair, first):
    call_a, call_b = pair(gpu_device)
    fresh_a, fresh_b = _fresh(call_a), _fresh(call_b)
    assert not all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(fresh_a, fresh_b))
    _release()
    call_a()  # the workspace buffers exist at their sizes: the calls below only rewrite their contents
    torch.cuda.synchronize()
    # A on a side stream and B on the default stream (the library sees it as stream NULL), and the reverse
    side = torch.cuda.Stream(device=gpu_device)
    streams = [side, torch.cuda.current_stream(gpu_device)]
    if first == "default":
        streams.reverse()
    with torch.cuda.stream(streams[0]):
        busy = _busy(gpu_device)
        got_a = call_a()  # queued behind the matmuls, and nothing waits for it
    with torch.cuda.stream(streams[1]):
        got_b = call_b()  # at once, on the other stream: the same buffers, other contents
    side.synchronize()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(busy[0, 0]))
    for got, fresh, name in ((got_a, fresh_a, "A"), (got_b, fresh_b, "B")):
        for k, (p, q) in enumerate(zip(got, fresh)):
            assert torch.equal(p, q), f"call {name}, output {k}"


# ------------------------------------------------- pipelined inverts ----
class Inverts:
    """200 x 8 uvw tracks, 4 channels, support 8 (test_gpu_api_validation._inputs); images with their weight sums."""

    def __init__(self, dev):
        uvw = syn.uvw_tracks(200, 8, array_radius_m=500.0, seed=2)
        f = syn.channel_frequencies(4)
        rng = np.random.default_rng(0)
        vis = (rng.standard_normal((uvw.shape[0], 4)) + 1j).astype(np.complex64)
        self.host = (uvw, f)
        self.cols = [_t(uvw, dev), _t(f, dev), _t(vis, dev), _t(np.ones(vis.shape, np.float32), dev)]
        self.dev = dev

    def image(self, npix=512, *, cols=None, pipelined=False, **kw):
        px = syn.pixel_size_for_grid(*self.host, npix)
        sw = torch.zeros(1, dtype=torch.float64, device=self.dev)
        img, _ = device_ms2dirty(*(cols or self.cols), npix, npix, px, px, support=8, sum_weights=sw,
                                 synchronize=not pipelined, resident_inputs=pipelined, **kw)
        return img, sw

    def predict(self, model):
        px = syn.pixel_size_for_grid(*self.host, model.shape[0])
        return device_dirty2ms(self.cols[0], self.cols[1], model, self.cols[3], px, px, support=8)[0],


def test_pipelined_inverts_share_the_grid_with_everything(gpu_device):
    inv = Inverts(gpu_device)
    model = _t(np.random.default_rng(1).standard_normal((512, 512)), gpu_device)
    packed = dict(single_precision_accumulation=True)
    ref_2d = _fresh(inv.image)
    ref_256 = _fresh(lambda: inv.image(256))
    ref_w = _fresh(lambda: inv.image(do_wstacking=True))
    ref_vis = _fresh(lambda: inv.predict(model))
    _release()
    ref_packed = inv.image(**packed)
    _release()
    got = [inv.image(pipelined=True),                     # 1
           inv.predict(model),                            # 2: borrows the grid, plans unscoped
           inv.image(pipelined=True),                     # 3
           inv.image(pipelined=True, **packed),           # 4: another cell type and clean byte count
           inv.image(pipelined=True),                     # 5
           inv.image(256),                                # 6: synchronous, a smaller grid
           inv.image(pipelined=True),                     # 7
           inv.image(pipelined=True, do_wstacking=True),  # 8
           inv.image(pipelined=True)]                     # 9
    torch.cuda.synchronize()
    refs = [ref_2d, ref_vis, ref_2d, None, ref_2d, ref_256, ref_2d, ref_w, ref_2d]
    for step, (g, r) in enumerate(zip(got, refs), 1):
        if r is not None:
            assert all(torch.equal(p, q) for p, q in zip(g, r)), f"step {step}"
    peak = float(ref_packed[0].abs().max())
    assert float((got[3][0] - ref_packed[0]).abs().max()) <= 1e-6 * peak
    assert peak > 0.0
    assert float(ref_2d[0].abs().max()) > 0.0 and float(ref_vis[0].abs().max()) > 0.0


def test_early_return_inside_the_plan_scope(gpu_device):
    inv = Inverts(gpu_device)
    ref_2d = _fresh(inv.image)
    bad = list(inv.cols)
    bad[2] = inv.cols[2].clone()
    bad[2][17, 2] = float("nan")
    _release()
    first = inv.image(pipelined=True)
    with pytest.raises(ValueError, match="non-finite visibility or weight"):
        inv.image(cols=bad, pipelined=True)  # reported after the planner's readback, inside the scope
    second, third = inv.image(pipelined=True), inv.image(pipelined=True)
    side = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(side):
        fourth = inv.image()  # synchronous, on a second stream right behind them
    side.synchronize()
    torch.cuda.synchronize()
    for k, g in enumerate((first, second, third, fourth)):
        assert all(torch.equal(p, q) for p, q in zip(g, ref_2d)), f"call {k}"
