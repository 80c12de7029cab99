"""
GPU tests of the island mask (`noise.device_auto_mask`): the mask bytes and
`n_seed`, `n_island` and `n_out` equal the numpy statement `_noise_np.auto_mask`.
`rounds` is informative and is only printed. The library's tile is 32 x 64
pixels, so the shapes and the islands below cross tile edges in both
directions, pass through a tile corner, and (the serpentine) need far more
rounds than one read-back of the flags covers.
"""
import numpy as np
import pytest

import _noise_np
from ska_sdp_cip_amd import noise

pytestmark = pytest.mark.gpu


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(x, seed, grow=None, region=None, base=None, what="", **kw):
    want_mask, want = _noise_np.auto_mask(x, seed, grow, region=region, base=base, **kw)
    mask, info = noise.device_auto_mask(_t(x), seed, grow, region=None if region is None else _t(region),
                                        base=None if base is None else _t(base), **kw)
    print(what, x.shape, kw, "library", info, "numpy", want)
    got = mask.cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want_mask), what
    for key in ("n_seed", "n_island", "n_out"):
        assert info[key] == want[key], (what, key)
    assert info["rounds"] >= 1
    return got, info


def _smooth_field(seed, n=300):
    rng = np.random.default_rng(seed)
    f = np.fft.rfft2(rng.standard_normal((n, n)))
    k = np.hypot(np.fft.fftfreq(n)[:, None], np.fft.rfftfreq(n)[None, :])
    return np.fft.irfft2(f * np.exp(-(k / 0.03) ** 2), s=(n, n))


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (67, 131), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_with_a_seed_in_every_corner(shape):
    rng = np.random.default_rng(shape[0] + shape[1])
    x = rng.standard_normal(shape)
    for i in (0, shape[0] - 1):
        for j in (0, shape[1] - 1):
            x[i, j] = 9.0
    for conn in (8, 4):
        got, info = _check(x, 4.0, 1.0, connectivity=conn, what="corners")
        assert got[0, 0] == got[-1, -1] == got[0, -1] == got[-1, 0] == 1 and info["n_seed"] >= 1


def test_island_crossing_tile_edges_in_both_directions():
    x = np.zeros((130, 200))
    x[20:110, 60:70] = 1.0   # down through the tile rows 32, 64 and 96
    x[50:55, 10:190] = 1.0   # across the tile columns 64 and 128
    x[52, 100] = 5.0
    x[120:125, 150:160] = 1.0  # a second island without a seed
    got, info = _check(x, 5.0, 1.0, what="cross")
    assert info["n_seed"] == 1 and info["n_island"] == 90 * 10 + 5 * 180 - 5 * 10 and got[122, 155] == 0


def test_staircase_through_a_tile_corner():
    x = np.zeros((96, 192))
    for k in range(-20, 21):  # a diagonal through the corner (32, 64) of four tiles
        x[32 + k, 64 + k] = 1.0
    x[12, 44] = 3.0  # the upper end
    got8, info8 = _check(x, 3.0, 1.0, what="stairs 8")
    assert info8["n_island"] == 41 and got8[52, 84] == 1
    got4, info4 = _check(x, 3.0, 1.0, connectivity=4, what="stairs 4")
    assert info4["n_island"] == 1 and got4[13, 45] == 0


def test_serpentine_needs_many_rounds_and_has_no_cap():
    x = _noise_np.serpentine(150)
    x[0, 0] = 2.0
    for conn in (4, 8):
        got, info = _check(x, 2.0, 1.0, connectivity=conn, what="serpentine")
        assert info["n_seed"] == 1 and info["n_island"] == int((x > 0).sum()) == 75 * 150 + 75
        assert got[149, 149] == 1 or got[149, 0] == 1  # the far end of the path
        assert info["rounds"] > 8  # more than one read-back of the flags


def test_two_islands_one_seed_and_inclusive_thresholds():
    x = np.zeros((40, 90))
    x[5:10, 5:10] = 0.3    # exactly grow
    x[7, 7] = 0.5          # exactly seed
    x[20:25, 60:70] = 0.4  # above grow, no seed
    x[30, 30] = np.nextafter(0.5, 0.0)  # just below seed, alone
    x[9, 10] = np.nextafter(0.3, 0.0)   # just below grow, beside the island
    got, info = _check(x, 0.5, 0.3, what="inclusive")
    assert (info["n_seed"], info["n_island"]) == (1, 25) and got[9, 10] == 0 and got[22, 65] == 0
    got, info = _check(x, 0.4, 0.4, what="seed == grow")  # every pixel at or above is its own seed
    assert info["n_seed"] == info["n_island"] == 50 + 1 + 1
    got, info = _check(x, 0.4, what="grow=None")
    assert info["n_island"] == 52


def test_nan_and_region_gaps_sever_an_island():
    x = np.zeros((50, 140))
    x[10, 5:135] = 1.0
    x[10, 5] = 4.0
    cut = x.copy()
    cut[10, 64] = np.nan
    got, info = _check(cut, 4.0, 1.0, what="nan")
    assert info["n_island"] == 59 and got[10, 65] == 0
    # a NaN that 8-connectivity walks round
    bridge = cut.copy()
    bridge[9, 64] = 1.0
    assert _check(bridge, 4.0, 1.0, what="bridge 8")[1]["n_island"] == 130
    assert _check(bridge, 4.0, 1.0, connectivity=4, what="bridge 4")[1]["n_island"] == 59
    region = np.ones(x.shape, dtype=np.uint8)
    region[:, 100] = 0
    got, info = _check(x, 4.0, 1.0, region=region, what="region gap")
    assert info["n_island"] == 95 and got[10, 101] == 0
    seedless = np.ones(x.shape, dtype=np.uint8)
    seedless[10, 5] = 0  # the seed itself lies outside the region
    assert _check(x, 4.0, 1.0, region=seedless, what="seed outside")[1]["n_seed"] == 0


def test_negative_island_with_and_without_positive():
    x = np.zeros((70, 70))
    x[10:20, 10:20] = -1.0
    x[15, 15] = -6.0
    x[40:50, 40:50] = 1.0
    x[45, 45] = 6.0
    got, info = _check(x, 5.0, 0.5, what="absolute")
    assert info["n_seed"] == 2 and info["n_island"] == 200
    got, info = _check(x, 5.0, 0.5, positive=True, what="positive")
    assert info["n_seed"] == 1 and info["n_island"] == 100 and got[15, 15] == 0


def test_base_is_ored_in_and_out_may_be_base():
    import torch

    rng = np.random.default_rng(3)
    x = _smooth_field(7, 130)
    hi_t, lo_t = np.percentile(np.abs(x), [99, 90])
    base = (rng.random(x.shape) < 0.05).astype(np.uint8) * 7  # any nonzero value counts
    got, info = _check(x, hi_t, lo_t, base=base, what="base")
    assert info["n_out"] > info["n_island"] > 0 and set(np.unique(got)) == {0, 1}
    # in place: out is base
    grown = _t((base != 0).astype(np.uint8))
    mask, info2 = noise.device_auto_mask(_t(x), hi_t, lo_t, base=grown, out=grown)
    assert mask is grown and np.array_equal(grown.cpu().numpy(), got) and info2["n_out"] == info["n_out"]
    # a bool out, and a second pass over the grown mask changes nothing
    flags = torch.zeros(x.shape, dtype=torch.bool, device="cuda")
    mask, _ = noise.device_auto_mask(_t(x), hi_t, lo_t, base=grown, out=flags)
    assert mask is flags and np.array_equal(flags.cpu().numpy(), got != 0)
    # no pixel at or above seed: the output is the base
    got0, info0 = _check(x, 2.0 * np.abs(x).max(), lo_t, base=base, what="no seed")
    assert info0["n_seed"] == 0 == info0["n_island"] and np.array_equal(got0, (base != 0).astype(np.uint8))
    assert _check(x, 2.0 * np.abs(x).max(), lo_t, what="nothing")[1]["n_out"] == 0


def test_every_pixel_above_seed():
    x = np.full((67, 131), 3.0)
    got, info = _check(x, 2.0, 1.0, what="all")
    assert info["n_seed"] == info["n_island"] == info["n_out"] == x.size and got.all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_smooth_fields(seed):
    x = _smooth_field(seed)
    hi_t, lo_t = np.percentile(np.abs(x), [99, 90])
    for conn in (8, 4):
        got, info = _check(x, hi_t, lo_t, connectivity=conn, what="field")
        assert 0 < info["n_seed"] < info["n_island"] < (np.abs(x) >= lo_t).sum()


def test_host_wrapper_and_argument_errors():
    import torch

    x = _smooth_field(4, 90)
    hi_t, lo_t = np.percentile(np.abs(x), [99, 90])
    keep = x.copy()
    want, winfo = _noise_np.auto_mask(x, hi_t, lo_t)
    mask, info = noise.auto_mask(x, hi_t, lo_t)
    assert isinstance(mask, np.ndarray) and np.array_equal(mask, want) and info["n_island"] == winfo["n_island"]
    mask, _ = noise.auto_mask(torch.from_numpy(x), hi_t, lo_t, base=np.zeros(x.shape, dtype=bool))
    assert torch.is_tensor(mask) and mask.is_cuda and np.array_equal(mask.cpu().numpy(), want)
    assert np.array_equal(x, keep)
    img = _t(x)
    nan = float("nan")
    for seed, grow in ((1.0, 2.0), (1.0, 0.0), (nan, 1.0), (1.0, nan), (float("inf"), 1.0), (0.0, None), (-1.0, -2.0)):
        with pytest.raises(ValueError, match="cip_auto_mask"):
            noise.device_auto_mask(img, seed, grow)
    with pytest.raises(ValueError, match="connectivity"):
        noise.device_auto_mask(img, 2.0, 1.0, connectivity=6)
    for bad in (img.float(), img.t(), img[0]):
        with pytest.raises(ValueError):
            noise.device_auto_mask(bad, 2.0, 1.0)
    for kw in (dict(region=torch.ones((90, 91), dtype=torch.uint8, device="cuda")),
               dict(base=torch.ones((90, 90), dtype=torch.float64, device="cuda")),
               dict(out=torch.ones((90, 90), dtype=torch.uint8))):
        with pytest.raises(ValueError):
            noise.device_auto_mask(img, 2.0, 1.0, **kw)
