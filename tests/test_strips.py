"""
Strong-scaling uv-strip decomposition (ska_sdp_cip_amd.strips):
the strip plan covers every visibility exactly once, the single-process
emulation of the halo exchange / all-to-all equals the one-shot image, and a
world-size-2 (and 3) gloo run of the real collectives gives the single-process
image at 1e-13 - with the CPU restatement of the per-rank stages
(tests/_strip_np.py) standing in for the GPU; a recorder in the gloo ranks pins
the per-rank order of backend stages and collectives. The GPU form of the same
checks is in test_gpu_strips.py.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from ska_sdp_cip_amd import strips
from ska_sdp_cip_amd import synthetic as syn

NPIX = 64


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _case(nrow=801, nchan=16, seed=4):
    ms = syn.make_measurement_set(nrow, nchan, n_ant=12, array_radius_m=800.0, seed=seed)
    vis, _, _, w = oracle.stokes_i(ms.visibilities(), ms.flags(), ms.weights())
    uvw, f = ms.uvw(), ms.channel_frequencies()
    px = syn.pixel_size_for_grid(uvw, f, NPIX)
    return uvw, f, vis, w, px


def _prm(px, W, wstack=None):
    """2-D parameters, or with wstack = (uvw, freq) the w-stacking stack of that data."""
    if wstack is None:
        return oracle.choose_params(NPIX, NPIX, px, px, support=W)
    wmin, wmax = oracle.w_range(*wstack)
    return oracle.choose_params(NPIX, NPIX, px, px, support=W, do_wstacking=True, wmin=wmin, wmax=wmax)


class _P:  # the fields plan_strips / strip_slices read from cip_gridder_params
    def __init__(self, prm):
        self.nu, self.nv, self.support = prm["nu"], prm["nv"], prm["support"]


def _strip_datas(uvw, f, vis, w, px, prm, layout):
    tu, tf = torch.from_numpy(uvw), torch.from_numpy(f)
    tv = torch.from_numpy(vis.astype(np.complex128))
    tw = torch.from_numpy(w.astype(np.float64))
    out = []
    for r in range(layout.world):
        y0, y1 = layout.rows(r)
        rows, c0, c1 = strips.strip_slices(tu, tf, _P(prm), px, y0, y1)
        out.append(strips.gather_strip(tu, tv, tw, rows, c0, c1))
    return out


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_strip_plan_partitions_visibilities(world):
    uvw, f, vis, w, px = _case()
    prm = _prm(px, 8)
    layout = strips.plan_strips(torch.from_numpy(uvw), torch.from_numpy(f), _P(prm), px, NPIX, NPIX, world,
                                balance="vis")
    yb = layout.y_bounds
    assert yb[0] == 0 and yb[-1] == prm["nv"]
    assert all(b - a >= prm["support"] for a, b in zip(yb, yb[1:]))
    xb = layout.x_bounds
    assert xb[0] == 0 and xb[-1] == NPIX and all(x % 4 == 0 and b > a for x, a, b in zip(xb, xb, xb[1:]))
    count = np.zeros(vis.shape, dtype=np.int64)
    datas = _strip_datas(uvw, f, vis, w, px, prm, layout)
    for d in datas:
        for r, a, b in zip(d.rows.numpy(), d.chan_start.numpy(), d.chan_stop.numpy()):
            assert a < b
            count[r, a:b] += 1
    assert (count == 1).all()
    sizes = np.array([d.nvis for d in datas])
    assert sizes.sum() == vis.size
    if world > 1:  # balanced, up to the granularity of strips at least W rows high
        iy = strips.origin_rows(torch.from_numpy(uvw[:, 1]), torch.from_numpy(f) / strips.SPEED_OF_LIGHT,
                                prm["nv"] * px, prm["nv"], prm["support"])
        hist = np.bincount(iy.numpy().ravel(), minlength=prm["nv"])
        window = np.convolve(hist, np.ones(2 * prm["support"], dtype=np.int64)).max()
        assert sizes.max() <= 1.1 * vis.size / world + window
    # the gathered visibilities are the right ones
    d = datas[-1]
    k = 0
    for r, a, b in zip(d.rows.numpy()[:50], d.chan_start.numpy()[:50], d.chan_stop.numpy()[:50]):
        np.testing.assert_array_equal(d.vis.numpy()[k:k + b - a], vis[r, a:b])
        k += b - a


def test_strip_plan_rejects_bad_splits():
    uvw, f, _, _, px = _case(nrow=50, nchan=2)
    prm = _prm(px, 8)
    with pytest.raises(ValueError):  # fewer blocks of 4 image rows than ranks
        strips.plan_strips(torch.from_numpy(uvw), torch.from_numpy(f), _P(prm), px, NPIX, NPIX, 17)
    with pytest.raises(ValueError):  # strips lower than the kernel support
        strips.plan_strips(torch.from_numpy(uvw), torch.from_numpy(f), _P(prm), px, NPIX, NPIX, 32)


@pytest.mark.parametrize("world,W", [(1, 8), (2, 8), (3, 8), (4, 6), (8, 4)])
def test_strip_emulation_equals_one_shot(world, W):
    from _strip_np import NumpyStripBackend

    uvw, f, vis, w, px = _case()
    prm = _prm(px, W)
    layout = strips.plan_strips(torch.from_numpy(uvw), torch.from_numpy(f), _P(prm), px, NPIX, NPIX, world)
    datas = _strip_datas(uvw, f, vis, w, px, prm, layout)
    be = NumpyStripBackend(prm, px, px, NPIX, NPIX)
    img = strips.invert_strips_local(datas, torch.from_numpy(f), layout, be).numpy()
    full = oracle.ms2dirty(uvw, f, vis, w, NPIX, NPIX, px, px, support=W, nthreads=1) / w.astype(np.float64).sum()
    assert np.abs(img - full).max() < 1e-13 * max(1.0, np.abs(full).max())
    # every rank's buffer holds only its strip + halo rows and is left clean
    assert len(be.ranks) == world
    for r, b in enumerate(be.ranks):
        assert b.rows == strips.strip_buffer_rows(layout, r)
        assert float(b.grid.abs().max()) == 0.0 and not b.dirty
    if world > 1:
        assert sum(b.rows[1] for b in be.ranks) == prm["nv"] + world * (W - 1)


def test_backend_without_the_base_class_still_works():
    # a backend written before StripBackend existed: the stages and nothing
    # else (no base class, no ranks / device / single / live_rows); the drivers
    # give it the base's defaults
    from _strip_np import NumpyStripBackend

    members = {k: v for k, v in vars(NumpyStripBackend).items() if k == "__init__" or not k.startswith("__")}
    members["spawn"] = lambda self: Plain(self.prm, self.px, self.py, self.npix_x, self.npix_y, rows=self.rows)
    Plain = type("Plain", (), members)
    world, W = 3, 6
    uvw, f, vis, w, px = _case()
    prm = _prm(px, W)
    layout = strips.plan_strips(torch.from_numpy(uvw), torch.from_numpy(f), _P(prm), px, NPIX, NPIX, world)
    datas = _strip_datas(uvw, f, vis, w, px, prm, layout)
    be = Plain(prm, px, px, NPIX, NPIX)
    assert not isinstance(be, strips.StripBackend) and not hasattr(be, "ranks")
    img = strips.invert_strips_local(datas, torch.from_numpy(f), layout, be).numpy()
    full = oracle.ms2dirty(uvw, f, vis, w, NPIX, NPIX, px, px, support=W, nthreads=1) / w.astype(np.float64).sum()
    assert np.abs(img - full).max() < 1e-13 * max(1.0, np.abs(full).max())
    assert len(be.ranks) == world and be.ranks[0] is be and all(isinstance(b, Plain) for b in be.ranks)
    for b in be.ranks:
        assert float(b.grid.abs().max()) == 0.0 and not b.dirty


@pytest.mark.parametrize("world,W", [(1, 6), (2, 6), (3, 4), (5, 8)])
def test_wstacking_strip_emulation_equals_one_shot(world, W):
    # the reference's own gridding mode split by uv strips: every plane's
    # strip rows, the halos of all planes, per-plane pass A / regrouping /
    # pass B with the w screen, then the final w correction per rank
    from _strip_np import NumpyStripBackend

    uvw, f, vis, w, px = _case(nrow=601, nchan=8)
    uvw = uvw * np.array([1.0, 1.0, 40.0])  # a deep w range: several planes
    prm = _prm(px, W, wstack=(uvw, f))
    assert prm["nplanes"] > W
    layout = strips.plan_strips(torch.from_numpy(uvw), torch.from_numpy(f), _P(prm), px, NPIX, NPIX, world)
    datas = _strip_datas(uvw, f, vis, w, px, prm, layout)
    be = NumpyStripBackend(prm, px, px, NPIX, NPIX)
    img = strips.invert_strips_local(datas, torch.from_numpy(f), layout, be).numpy()
    full = oracle.ms2dirty(uvw, f, vis, w, NPIX, NPIX, px, px, support=W, do_wstacking=True,
                           nthreads=1) / w.astype(np.float64).sum()
    assert np.abs(img - full).max() < 1e-13 * max(1.0, np.abs(full).max())
    for b in be.ranks:
        assert float(b.grid.abs().max()) == 0.0 and not b.dirty


def _join_gloo(rank, world, port, W, wstack):
    """A spawned rank's start: the import paths, the gloo group, the case and
    this rank's strip -> (NumpyStripBackend, uvw, f, vis, w, px, prm, layout, data)."""
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root / "ska-sdp-continuum-imaging-pipeline_amd"), str(root / "oracle"), str(root / "tests")]
    from _strip_np import NumpyStripBackend

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if wstack:
        uvw, f, vis, w, px = _case(nrow=601, nchan=8)
        uvw = uvw * np.array([1.0, 1.0, 40.0])
        prm = _prm(px, W, wstack=(uvw, f))
    else:
        uvw, f, vis, w, px = _case()
        prm = _prm(px, W)
    layout = strips.plan_strips(torch.from_numpy(uvw), torch.from_numpy(f), _P(prm), px, NPIX, NPIX, world)
    data = _strip_datas(uvw, f, vis, w, px, prm, layout)[rank]  # each rank holds only its strip
    return NumpyStripBackend, uvw, f, vis, w, px, prm, layout, data


def _worker(rank, world, port, q, W, wstack=False):
    backend, uvw, f, vis, w, px, prm, layout, data = _join_gloo(rank, world, port, W, wstack)
    be = backend(prm, px, px, NPIX, NPIX)
    img = strips.invert_strips(data, torch.from_numpy(f), layout, be, dst=0)
    # two more inverts with the gather in flight while the next one grids
    p1 = strips.invert_strips(data, torch.from_numpy(f), layout, be, dst=0, gather_async=True)
    p2 = strips.invert_strips(data, torch.from_numpy(f), layout, be, dst=0, gather_async=True)
    img1, img2 = p1.wait(), p2.wait()
    if rank == 0:
        full = oracle.ms2dirty(uvw, f, vis, w, NPIX, NPIX, px, px, support=W, do_wstacking=wstack,
                               nthreads=1) / w.astype(np.float64).sum()
        err = max(float(np.abs(i.numpy() - full).max()) for i in (img, img1, img2))
        q.put((err, float(np.abs(full).max()), float(be.grid.abs().max())))
    else:
        assert img is None and img1 is None and img2 is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,W,wstack", [(2, 8, False), (3, 6, False), (2, 6, True)])
def test_strip_halo_exchange_gloo(world, W, wstack):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, W, wstack)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
    assert all(p.exitcode == 0 for p in procs)
    err, peak, left = q.get(timeout=5)
    assert err < 1e-13 * max(1.0, peak)
    assert left == 0.0


STAGE_CALLS = ("grid_strip", "mark_clean", "pass_rows", "pass_rows_packed", "pass_cols", "pass_cols_wplane",
               "finish_rows")
DIST_CALLS = ("batch_isend_irecv", "all_reduce", "all_gather", "all_to_all_single", "gather")


def _record(obj, names, log, depth):
    """Replace obj's callables `names` by ones that append their name to `log`;
    only the outermost call is logged (a recorded call made from inside another -
    the base pass_rows_packed's pass_rows - is part of that stage)."""
    def wrapped(name, fn):
        def call(*args, **kwargs):
            if depth[0] == 0:
                log.append(name)
            depth[0] += 1
            try:
                return fn(*args, **kwargs)
            finally:
                depth[0] -= 1
        return call

    for name in names:
        setattr(obj, name, wrapped(name, getattr(obj, name)))


def _order_worker(rank, world, port, q, W, sparse, knows_live, wstack):
    base, uvw, f, vis, w, px, prm, layout, data = _join_gloo(rank, world, port, W, wstack)

    class KnowsLiveRows(base):
        """Knows its live rows before pass A: the rows of its buffer plane that hold a non-zero."""

        def live_rows(self, h, plane=0):
            buf = self.grid if self.nplanes == 1 else self.grid[plane]
            return (buf[:h] != 0).reshape(h, -1).any(dim=1)

    be = (KnowsLiveRows if knows_live else base)(prm, px, px, NPIX, NPIX)
    log, depth = [], [0]
    _record(be, STAGE_CALLS, log, depth)
    _record(dist, DIST_CALLS, log, depth)
    img = strips.invert_strips(data, torch.from_numpy(f), layout, be, dst=0, sparse=sparse)
    if rank == 0:
        full = oracle.ms2dirty(uvw, f, vis, w, NPIX, NPIX, px, px, support=W, do_wstacking=wstack,
                               nthreads=1) / w.astype(np.float64).sum()
        q.put((log, int(prm["nplanes"]) if wstack else 1, float(np.abs(img.numpy() - full).max()),
               float(np.abs(full).max())))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", ["sparse", "dense", "knows_live", "knows_live_wstack"])
def test_per_rank_call_order_gloo(case):
    """The per-rank sequence of backend stages and collectives of the
    distributed invert (rank 0 of 2, W = 6): the N-GPU speed depends on it (a
    collective more, or pass A on the wrong side of the mask all-gather, costs
    a rendezvous per plane). `bind` comes first in every case and is not
    recorded; with w-stacking `mark_clean` may come anywhere after the last
    plane's pass A."""
    world, W = 2, 6
    sparse, knows_live, wstack = case != "dense", case.startswith("knows_live"), case.endswith("wstack")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_order_worker, args=(r, world, port, q, W, sparse, knows_live, wstack))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
    assert all(p.exitcode == 0 for p in procs)
    log, nplanes, err, peak = q.get(timeout=5)
    head = ["grid_strip", "batch_isend_irecv", "all_reduce"]
    if wstack:
        assert nplanes > W
        want = head + ["all_gather", "pass_rows_packed", "all_to_all_single", "pass_cols_wplane"] * nplanes + \
            ["finish_rows", "gather"]
        at = log.index("mark_clean")
        assert "pass_rows_packed" not in log[at:]
        log = log[:at] + log[at + 1:]
    elif knows_live:
        want = head + ["all_gather", "pass_rows_packed", "mark_clean", "all_to_all_single", "pass_cols", "gather"]
    else:
        want = head + ["pass_rows", "mark_clean"] + ["all_gather"] * sparse + ["all_to_all_single", "pass_cols",
                                                                               "gather"]
    assert log == want
    if knows_live:
        assert err < 1e-13 * max(1.0, peak)


def test_strips_with_empty_strips_and_no_data():
    # a compact array (every footprint in a few grid rows): most strips hold
    # no visibilities; the decomposition still equals the one-shot image
    from _strip_np import NumpyStripBackend

    uvw, f, vis, w, px = _case(nrow=300, nchan=4)
    uvw = uvw * 0.02  # all baselines near the uv origin
    prm = _prm(px, 8)
    world = 6
    layout = strips.plan_strips(torch.from_numpy(uvw), torch.from_numpy(f), _P(prm), px, NPIX, NPIX, world)
    datas = _strip_datas(uvw, f, vis, w, px, prm, layout)
    assert sum(d.nvis for d in datas) == vis.size
    assert sum(d.nvis == 0 for d in datas) >= 2
    be = NumpyStripBackend(prm, px, px, NPIX, NPIX)
    img = strips.invert_strips_local(datas, torch.from_numpy(f), layout, be).numpy()
    full = oracle.ms2dirty(uvw, f, vis, w, NPIX, NPIX, px, px, support=8, nthreads=1) / w.astype(np.float64).sum()
    assert np.abs(img - full).max() < 1e-13 * max(1.0, np.abs(full).max())
    # no rows at all: a valid layout, empty strips
    e = torch.zeros((0, 3), dtype=torch.float64)
    layout0 = strips.plan_strips(e, torch.from_numpy(f), _P(prm), px, NPIX, NPIX, 4)
    assert layout0.y_bounds[0] == 0 and layout0.y_bounds[-1] == prm["nv"]
    rows, c0, c1 = strips.strip_slices(e, torch.from_numpy(f), _P(prm), px, *layout0.rows(1))
    assert rows.numel() == 0


@pytest.mark.parametrize("world", [2, 4, 8])
def test_strip_plan_balances_the_cost_model(world):
    # the default balance: modelled per-rank cost (visibilities, row slices,
    # pass-A rows; strips.row_costs) near-equal across strips
    uvw, f, vis, w, px = _case(nrow=1500, nchan=32)
    prm = _prm(px, 8)
    tu, tf = torch.from_numpy(uvw), torch.from_numpy(f)
    cost = strips.row_costs(tu, tf, _P(prm), px, px)
    assert cost.shape == (prm["nv"],) and (cost > 0).all()
    layout = strips.plan_strips(tu, tf, _P(prm), px, NPIX, NPIX, world)
    share = [cost[a:b].sum() for a, b in zip(layout.y_bounds, layout.y_bounds[1:])]
    window = np.convolve(cost, np.ones(2 * prm["support"])).max()
    assert max(share) <= cost.sum() / world + window
    # the strips still partition the visibilities
    datas = _strip_datas(uvw, f, vis, w, px, prm, layout)
    assert sum(d.nvis for d in datas) == vis.size


@pytest.mark.parametrize("wstack", [False, True])
def test_sparse_alltoall_equals_dense_and_sends_less(wstack):
    # the all-to-all carries only each rank's live pass-A rows (rows of an empty
    # grid row transform to exact zeros): the same image bit for bit, fewer
    # bytes. A concentrated uv coverage (short baselines) on a 256^2 image
    # leaves most grid rows empty.
    from _strip_np import NumpyStripBackend

    npix, world, W = 256, 4, 6
    uvw, f, vis, w, _ = _case(nrow=700, nchan=8)
    px = syn.pixel_size_for_grid(uvw, f, npix) * 0.3  # the tracks fill ~30 % of the uv plane
    if wstack:
        wmin, wmax = oracle.w_range(uvw, f)
        prm = oracle.choose_params(npix, npix, px, px, support=W, do_wstacking=True, wmin=wmin, wmax=wmax)
    else:
        prm = oracle.choose_params(npix, npix, px, px, support=W)
    layout = strips.plan_strips(torch.from_numpy(uvw), torch.from_numpy(f), _P(prm), px, npix, npix, world,
                                balance="vis")
    datas = _strip_datas(uvw, f, vis, w, px, prm, layout)
    imgs, sent = {}, {}
    for sparse in (False, True):
        be = NumpyStripBackend(prm, px, px, npix, npix)
        st = []
        imgs[sparse] = strips.invert_strips_local(datas, torch.from_numpy(f), layout, be, stages=st,
                                                  sparse=sparse).numpy()
        sent[sparse] = sum(s["a2a_send_bytes"] for s in st)
    # (the oracle's OpenMP gridding sums in thread order: ~1e-16 run to run)
    assert np.abs(imgs[True] - imgs[False]).max() <= 1e-14 * np.abs(imgs[False]).max()
    assert sent[True] < 0.8 * sent[False], sent
