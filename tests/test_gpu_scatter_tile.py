"""
The 2-D lane scatter's work tile (csrc/cip_params.hip scatter_tile_shape: a
property of the plan, 32 x 32, 64 x 32, 32 x 64 or 64 x 64 cells; the dirty
mask keeps its 32-cell unit). The rule picks a larger tile only on grids of
2048^2 cells and more, so every case here forces the shape with
CIP_SCATTER_TILE in a child process (read once per process); this process,
with the switch unset, runs the 32 x 32 plans.

Per shape, `_cases()` runs: cip_ms2dirty on multichannel input at W = 4, 8, 16
(fp64 class; W = 16 has no larger instance and must fall back), a hot tile (80,000
single-channel visibilities at the grid centre, which lies inside one 64-cell
tile and on the corner of four 32-cell ones), baselines that wrap through the
periodic seam, a grid of no whole tiles (nu = 140), the PSF, CIP_NORMALISE,
complex128 input, the packed class, two calls of different uv coverage and an
empty one on the pruned-FFT path (a stale or too small dirty mask leaves
residue in the kept-clean grid), plan reuse between invert and predict, and
back-to-back pipelined calls.

Bounds: against the fp64 oracle, test_gpu_invert_parity.py's (1e-10 of the
weight sum for the fp64 class, 1e-5 for the packed class); between shapes,
test_gpu_row_phases.py's "equal images" (1e-12 of the peak) for the fp64
class: its integer sub-grid sums are exact, only the flush's fp64 adds come in
another order. The packed class rounds every tap to a quantum that follows the
work unit's size (packed_chunk_gain), so another tile's work units are another
quantisation of the same sums, not the same image: it is held to its oracle
bound at every shape and to equal sums and counts, not to "equal images".
Weight sums and visibility counts are equal bit for bit.
"""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SHAPES = ("64x32", "32x64", "64")
TIGHT = 1e-10  # test_gpu_invert_parity.py: fp64 class against the oracle, of the weight sum
SINGLE = 1e-5  # the packed class there
EQUAL = 1e-12  # test_gpu_row_phases.py: equal images, of the peak


def _ms(n_rows, nchan, seed, radius=1500.0, n_ant=20):
    from ska_sdp_cip_amd import synthetic as syn
    from ska_sdp_cip_amd.invert import StokesIGridderInput

    ms = syn.make_measurement_set(n_rows, nchan, n_ant=n_ant, array_radius_m=radius, seed=seed)
    gi = StokesIGridderInput.from_measurement_set_reader(ms)
    return gi.uvw, gi.channel_frequencies, gi.visibilities, gi.effective_weights().astype(np.float32)


def _inputs():
    """The host inputs of every case (the same in each process): name -> (uvw, f, vis, w, npix, px, kwargs)."""
    from ska_sdp_cip_amd import synthetic as syn

    out = {}
    uvw, f, vis, w = _ms(3_000, 16, 5)
    for W in (4, 8, 16):
        out[f"w{W}"] = (uvw, f, vis, w, 128, syn.pixel_size_for_grid(uvw, f, 128, support=W), dict(support=W))
    # the hot tile of test_gpu_dirty2ms.py::test_hot_tile_is_split on a 192^2 grid:
    # its centre (96, 96) is a corner of four 32-cell tiles, inside one 64-cell tile
    big = syn.uvw_tracks(100, 16, array_radius_m=1000.0, seed=1)
    f1 = syn.channel_frequencies(1)
    hot = syn.uvw_tracks(80_000, 16, array_radius_m=50.0, seed=2)
    rng = np.random.default_rng(4)
    hv = (rng.standard_normal((80_000, 1)) + 1j * rng.standard_normal((80_000, 1))).astype(np.complex64)
    out["hot"] = (hot, f1, hv, np.ones((80_000, 1), np.float32), 96, syn.pixel_size_for_grid(big, f1, 96),
                  dict(support=8))
    # a pixel 3x too coarse: baselines wrap through the edge tiles, halos cross the seam
    out["wrap"] = (uvw, f, vis, w, 128, 3.0 * syn.pixel_size_for_grid(uvw, f, 128), dict(support=8))
    # nu = 140: two whole 64-cell tiles and a 12-cell edge tile per axis; the hipFFT path
    out["n140"] = (uvw, f, vis, w, 70, syn.pixel_size_for_grid(uvw, f, 70), dict(support=8))
    px = syn.pixel_size_for_grid(uvw, f, 128)
    out["psf"] = (uvw, f, None, w, 128, px, dict(support=8, psf=True))
    out["norm"] = (uvw, f, vis, w, 128, px, dict(support=8, normalise=True))
    out["c128"] = (uvw, f, vis.astype(np.complex128), w.astype(np.float64), 128, px, dict(support=6))
    out["single"] = (uvw, f, vis, w, 128, px, dict(support=8, single_precision_accumulation=True))
    # the pruned-FFT path (a 1024^2 grid: 32 mask tiles per row) with two uv coverages
    a = _ms(2_000, 8, 21, radius=1500.0, n_ant=16)
    b = _ms(1_500, 4, 22, radius=400.0, n_ant=10)
    out["mask_a"] = a + (512, syn.pixel_size_for_grid(a[0], a[1], 512), dict(support=8))
    out["mask_b"] = b + (512, syn.pixel_size_for_grid(b[0], b[1], 512), dict(support=8))
    return out


ORDER = ("w4", "w8", "w16", "hot", "wrap", "n140", "psf", "norm", "c128", "single", "mask_a", "mask_b")


def _cases(only=None):
    """Everything one process computes at its CIP_SCATTER_TILE, as arrays."""
    import torch

    from ska_sdp_cip_amd import _lib, gridder

    dev = torch.device("cuda", 0)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    inp = _inputs()
    out = {}
    _lib.profile_enable(True)
    try:
        for name in (only or ORDER):
            uvw, f, vis, w, npix, px, kw = inp[name]
            sw = torch.empty(1, dtype=torch.float64, device=dev)
            img, prm = gridder.device_ms2dirty(t(uvw), t(f), t(vis), t(w), npix, npix, px, px, sum_weights=sw, **kw)
            prof = _lib.profile_last()
            out[f"img_{name}"] = img.cpu().numpy()
            out[f"sw_{name}"] = np.array([sw.item()])
            out[f"cnt_{name}"] = np.array([prof["visibilities"], prof["runs"], prof["chunks"], prm.tile], np.int64)
    finally:
        _lib.profile_enable(False)
    if only:
        return out
    # mask_b ran last on this workspace: an empty call must find the grid clean
    uvw, f, vis, w, npix, px, kw = inp["mask_b"]
    img, _ = gridder.device_ms2dirty(t(uvw[:0]), t(f), t(vis[:0]), t(w[:0]), npix, npix, px, px, **kw)
    out["img_mask_empty"] = img.cpu().numpy()
    # plan reuse: invert (this process's tile) -> predict reusing -> invert reusing the predict's plan
    uvw, f, vis, w, npix, px, kw = inp["w8"]
    tu, tf, tv, tw = t(uvw), t(f), t(vis), t(w)
    model = torch.from_numpy(np.random.default_rng(9).standard_normal((npix, npix))).to(dev)
    fresh, _ = gridder.device_dirty2ms(tu, tf, model, tw, px, px, support=8)
    gridder.device_ms2dirty(tu, tf, tv, tw, npix, npix, px, px, support=8)
    reused, _ = gridder.device_dirty2ms(tu, tf, model, tw, px, px, support=8, reuse_plan=True)
    out["predict_equal"] = np.array([int(torch.equal(fresh, reused))])
    again, _ = gridder.device_ms2dirty(tu, tf, tv, tw, npix, npix, px, px, support=8, reuse_plan=True)
    out["img_reuse"] = again.cpu().numpy()
    # pipelined back-to-back calls alternating two resident data sets
    sets = [(tu, tf, tv, tw), (tu, tf, tv * (0.5 - 2.0j), tw * 0.25 + 1.0)]
    outs = []
    for k in range(6):
        o = torch.empty((npix, npix), dtype=torch.float64, device=dev)
        s = torch.empty(1, dtype=torch.float64, device=dev)
        gridder.device_ms2dirty(*sets[k % 2], npix, npix, px, px, support=8, normalise=True, out=o, sum_weights=s,
                                synchronize=False, resident_inputs=True)
        outs.append((o, s))
    torch.cuda.synchronize()
    for k, (o, s) in enumerate(outs):
        out[f"img_pipe{k}"] = o.cpu().numpy()
        out[f"sw_pipe{k}"] = np.array([s.item()])
    for k in range(2):
        ref, _ = gridder.device_ms2dirty(*sets[k], npix, npix, px, px, support=8, normalise=True)
        out[f"img_pipe_ref{k}"] = ref.cpu().numpy()
    torch.cuda.synchronize()
    return out


CHILD = """
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {orc!r}, {tests!r}]
import numpy as np
import test_gpu_scatter_tile as t
np.savez({out!r}, **t._cases({only!r}))
"""


def _child(tmp, tag, env, only=None):
    out = tmp / f"{tag}.npz"
    code = CHILD.format(root=str(ROOT), pkg=str(ROOT / "ska-sdp-continuum-imaging-pipeline_amd"),
                        orc=str(ROOT / "oracle"), tests=str(ROOT / "tests"), out=str(out), only=only)
    subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), check=True, timeout=300)
    return dict(np.load(out))


@pytest.fixture(scope="module")
def runs(gpu_device, tmp_path_factory):
    """Every shape's arrays, computed once: "32" in this process, the others in children."""
    tmp = tmp_path_factory.mktemp("scatter_tile")
    res = {"32": _cases()}
    for shape in SHAPES:
        res[shape] = _child(tmp, shape.replace("x", "_"), {"CIP_SCATTER_TILE": shape})
    return res


@pytest.fixture(scope="module")
def refs():
    """The fp64 oracle's image of each case, computed once."""
    import oracle

    out = {}
    for name, (uvw, f, vis, w, npix, px, kw) in _inputs().items():
        v = np.ones((uvw.shape[0], f.size), np.complex64) if vis is None else vis
        img = oracle.ms2dirty(uvw, f, v, w, npix, npix, px, px, support=kw["support"])
        sumw = float(np.asarray(w, np.float64).sum())
        out[name] = (img / sumw if kw.get("normalise") else img, 1.0 if kw.get("normalise") else sumw)
    return out


def _peak_err(a, b):
    peak = float(np.abs(b).max())
    assert peak > 0
    return float(np.abs(a - b).max()) / peak


@pytest.mark.parametrize("shape", ("32",) + SHAPES)
def test_images_match_the_oracle(runs, refs, shape):
    r = runs[shape]
    for name in ORDER:
        ref, sumw = refs[name]
        err = float(np.abs(r[f"img_{name}"] - ref).max()) / sumw
        print(f"{shape} {name}: |gpu - oracle| / sum w = {err:.3e}")
        assert err < (SINGLE if name == "single" else TIGHT), (shape, name, err)


@pytest.mark.parametrize("shape", SHAPES)
def test_images_sums_and_counts_across_shapes(runs, shape):
    base, r = runs["32"], runs[shape]
    assert sorted(base) == sorted(r)
    for name in ORDER:
        err = _peak_err(r[f"img_{name}"], base[f"img_{name}"])
        print(f"{shape} {name}: |img - img32| / peak = {err:.3e}, runs {r[f'cnt_{name}'][1]} vs {base[f'cnt_{name}'][1]}, "
              f"chunks {r[f'cnt_{name}'][2]} vs {base[f'cnt_{name}'][2]}")
        if name != "single":  # (the packed class: see the module's docstring)
            assert err <= EQUAL, (shape, name, err)
        assert np.array_equal(r[f"sw_{name}"], base[f"sw_{name}"]), (shape, name)
        assert r[f"cnt_{name}"][0] == base[f"cnt_{name}"][0], (shape, name)  # visibilities
        assert r[f"cnt_{name}"][3] == 32  # GridderParams.tile: the mask unit
    # multichannel input: longer row slices on the larger tile, strictly fewer runs;
    # W = 16 (fp64 class) has no larger instance: the 32 x 32 plan, run for run
    for name in ("w4", "w8", "wrap", "n140", "psf", "norm", "c128", "single", "mask_a", "mask_b"):
        assert r[f"cnt_{name}"][1] < base[f"cnt_{name}"][1], (shape, name)
    assert np.array_equal(r["cnt_w16"], base["cnt_w16"])


def test_hot_tile_is_split_on_the_64_tile(runs):
    c32, c64 = runs["32"]["cnt_hot"], runs["64"]["cnt_hot"]
    print("hot tile: chunks", c64[2], "on 64 x 64,", c32[2], "on 32 x 32")
    assert c64[0] == c32[0] == 80_000
    # one 64-cell tile holds them all: more than one work unit in it (none of
    # them the tile's sole unit), fewer than the four 32-cell tiles' units
    assert c64[2] == -(-80_000 // 16384) and c64[2] > 1
    assert c64[2] < c32[2]


@pytest.mark.parametrize("shape", ("32",) + SHAPES)
def test_grid_is_left_clean_and_masks_cover_the_flush(runs, shape):
    # mask_a and mask_b passed the oracle bound above on one workspace; the
    # empty call after them reads the kept-clean grid densely
    assert not np.any(runs[shape]["img_mask_empty"]), shape


@pytest.mark.parametrize("shape", ("32",) + SHAPES)
def test_plan_reuse_between_invert_and_predict(runs, shape):
    r = runs[shape]
    assert int(r["predict_equal"][0]) == 1, shape
    err = _peak_err(r["img_reuse"], r["img_w8"])
    print(f"{shape}: invert through the predict's plan, |img - fresh| / peak = {err:.3e}")
    assert err <= EQUAL, (shape, err)


@pytest.mark.parametrize("shape", ("32",) + SHAPES)
def test_pipelined_calls(runs, shape):
    r = runs[shape]
    for k in range(6):
        err = _peak_err(r[f"img_pipe{k}"], r[f"img_pipe_ref{k % 2}"])
        assert err <= EQUAL, (shape, k, err)
    assert r["sw_pipe0"][0] == r["sw_pipe2"][0] == r["sw_pipe4"][0] == r["sw_w8"][0]
    assert r["sw_pipe1"][0] == r["sw_pipe3"][0] == r["sw_pipe5"][0] != r["sw_pipe0"][0]


def test_flush_stores_agree_with_atomics(runs, tmp_path):
    names = ("w8", "hot", "wrap", "mask_a")
    st = _child(tmp_path, "stores", {"CIP_SCATTER_TILE": "64", "CIP_FLUSH_STORE": "1"}, only=names)
    for name in names:
        err = _peak_err(st[f"img_{name}"], runs["64"][f"img_{name}"])
        print(f"stores {name}: |stores - atomics| / peak = {err:.3e}")
        assert err <= EQUAL, (name, err)
        assert np.array_equal(st[f"cnt_{name}"], runs["64"][f"cnt_{name}"])
