"""
GPU tests of the order statistic and the noise estimate (`noise.device_image_select`,
`noise.device_image_noise`): equality with the numpy statement `_noise_np` (`==`
on the values, the exact `count`), never closeness.

The shapes run from one pixel to several workgroups plus a tail; the contents
are the ones a radix select can get wrong: an all-equal image (the candidates
never shrink, so beyond the compaction capacity of 65536 keys every pass is a
full one: 1031 x 517; below it the compacted path: 65 x 129), values that
differ only in the last digit, signs with both zeros and denormals, +-1e308
(|x - median| overflows), NaN and +-inf (no samples) and heavy ties.
"""
import ctypes
import math

import numpy as np
import pytest

import _noise_np
from ska_sdp_cip_amd import _lib, noise

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (1, 63), (7, 9), (65, 129), (257, 255), (1031, 517)]


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _equal(shape, rng):
    return np.full(shape, 0.375)


def _last_digit(shape, rng):
    n = shape[0] * shape[1]
    return (1.0 + rng.permutation(n) * 2.0 ** -52).reshape(shape)


def _mixed(shape, rng):
    x = rng.standard_normal(shape)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308])
    pick = rng.random(shape) < 0.3
    x[pick] = rng.choice(special, size=int(pick.sum()))
    return x


def _huge(shape, rng):
    return rng.choice(np.array([1e308, -1e308, 0.5e308, -1.7e308, 1.0, -3.0, 0.0]), size=shape)


def _nonfinite(shape, rng):
    x = rng.standard_normal(shape)
    pick = rng.random(shape) < 0.2
    x[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf]), size=int(pick.sum()))
    return x


def _all_nan(shape, rng):
    return np.full(shape, np.nan)


def _ties(shape, rng):
    return rng.integers(-2, 3, size=shape).astype(np.float64)


CONTENTS = {f.__name__[1:]: f for f in (_equal, _last_digit, _mixed, _huge, _nonfinite, _all_nan, _ties)}


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _check_noise(got, want, what):
    print(what, "library", got, "numpy", want)
    assert got["count"] == want["count"], what
    for key in ("median", "mad", "sigma"):
        assert _same(got[key], want[key]), (what, key, got[key], want[key])


def _check_ranks(img, x, region=None):
    v = np.sort(_noise_np.samples(x, region))
    dev_region = None if region is None else _t(region)
    if v.size == 0:  # no sample: every rank lies outside
        with pytest.raises(ValueError, match="cip_image_select"):
            noise.device_image_select(img, 0, region=dev_region)
        return
    for rank in sorted({0, v.size - 1, v.size // 4, v.size // 2, (3 * v.size) // 4}):
        value, count = noise.device_image_select(img, rank, region=dev_region)
        assert count == v.size and value == v[rank], (rank, value, v[rank])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("content", list(CONTENTS))
def test_noise_equals_the_numpy_statement(content, shape):
    x = CONTENTS[content](shape, np.random.default_rng(shape[0] * 1000 + shape[1]))
    img = _t(x)
    _check_noise(noise.device_image_noise(img), _noise_np.noise(x), (content, shape))
    assert np.array_equal(img.cpu().numpy().view(np.int64), x.view(np.int64))  # the image is only read
    if content in ("mixed", "ties", "equal", "nonfinite") and shape in ((1, 1), (7, 9), (65, 129), (1031, 517)):
        _check_ranks(img, x)


def test_lower_median_of_two_and_all_nan():
    got = noise.device_image_noise(_t(np.array([[3.0, 1.0]])))
    assert (got["count"], got["median"], got["mad"], got["sigma"]) == (2, 1.0, 0.0, 0.0)
    got = noise.device_image_noise(_t(np.full((5, 3), np.nan)))
    assert got["count"] == 0 and all(math.isnan(got[k]) for k in ("median", "mad", "sigma"))


def test_rank_equal_to_count_is_erange_with_the_count_set():
    x = np.random.default_rng(0).standard_normal((9, 11))
    x[2, 3], x[4, 5] = np.nan, np.inf
    img = _t(x)
    import torch

    count, value = ctypes.c_int64(-1), ctypes.c_double(0.0)
    stream = torch.cuda.current_stream().cuda_stream
    rc = _lib.lib().cip_image_select(img.data_ptr(), 9, 11, None, 97, stream, ctypes.byref(count), ctypes.byref(value))
    assert rc == _lib.CIP_ERANGE and count.value == 97 and b"cip_image_select" in _lib.lib().cip_last_error()
    with pytest.raises(ValueError, match="cip_image_select"):
        noise.device_image_select(img, 97)
    assert noise.device_image_select(img, 96) == (np.sort(x[np.isfinite(x)])[96], 97)
    with pytest.raises(ValueError, match="rank"):
        noise.device_image_select(img, -1)


@pytest.mark.parametrize("shape", [(7, 9), (257, 255)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_regions_odd_even_and_none(shape):
    rng = np.random.default_rng(5)
    x = _nonfinite(shape, rng)
    img = _t(x)
    region = (rng.random(shape) < 0.5).astype(np.uint8)
    finite = np.isfinite(x)
    for want_odd in (True, False):
        r = region.copy()
        if (int((finite & (r != 0)).sum()) % 2 == 1) != want_odd:  # flip one finite pixel
            i, j = np.argwhere(finite)[0]
            r[i, j] ^= 1
        assert int((finite & (r != 0)).sum()) % 2 == int(want_odd)
        _check_noise(noise.device_image_noise(img, region=_t(r)), _noise_np.noise(x, r), ("region", want_odd))
        _check_noise(noise.device_image_noise(img, region=_t(r != 0)), _noise_np.noise(x, r), ("bool region", want_odd))
        _check_ranks(img, x, r)
    none = np.zeros(shape, dtype=np.uint8)
    got = noise.device_image_noise(img, region=_t(none))
    assert got["count"] == 0 and math.isnan(got["sigma"])
    only_bad = (~finite).astype(np.uint8)  # a region of NaN and inf alone
    assert noise.device_image_noise(img, region=_t(only_bad))["count"] == 0


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (7, 9), (257, 255), (1031, 517)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_base_aligned_to_8_bytes_only(shape):
    import torch

    rng = np.random.default_rng(8)
    n = shape[0] * shape[1]
    flat = torch.empty(n + 3, dtype=torch.float64, device="cuda")
    assert flat.data_ptr() % 16 == 0
    x = _mixed(shape, rng)
    region = (rng.random(shape) < 0.7).astype(np.uint8)
    img = flat[1:n + 1].view(shape)
    img.copy_(_t(x))
    assert img.data_ptr() % 16 == 8 and img.is_contiguous()
    _check_noise(noise.device_image_noise(img), _noise_np.noise(x), ("misaligned", shape))
    # the region's base moved by one byte as well
    rflat = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    rview = rflat[1:].view(shape)
    rview.copy_(_t(region))
    _check_noise(noise.device_image_noise(img, region=rview), _noise_np.noise(x, region), ("misaligned region", shape))
    _check_ranks(img, x)


def test_non_default_stream():
    import torch

    x = _mixed((257, 255), np.random.default_rng(9))
    want = _noise_np.noise(x)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        img = _t(x)
        got = noise.device_image_noise(img)
        value, count = noise.device_image_select(img, 1000)
    stream.synchronize()
    _check_noise(got, want, "stream")
    assert (value, count) == (np.sort(x.ravel())[1000], x.size)


def test_bad_images_raise_before_the_library():
    import torch

    good = torch.zeros((8, 6), dtype=torch.float64, device="cuda")
    for bad in (good.t(), good[:, ::2], good.float(), good[0], good.cpu(), good.unsqueeze(0)):
        with pytest.raises(ValueError):
            noise.device_image_noise(bad)
        with pytest.raises(ValueError):
            noise.device_image_select(bad, 0)
    for region in (torch.ones((6, 8), dtype=torch.uint8, device="cuda"),
                   torch.ones((8, 6), dtype=torch.float64, device="cuda"),
                   torch.ones((8, 6), dtype=torch.uint8), torch.ones((6, 8), dtype=torch.uint8, device="cuda").t()):
        with pytest.raises(ValueError):
            noise.device_image_noise(good, region=region)


def test_host_wrapper_with_numpy_and_torch():
    import torch

    rng = np.random.default_rng(10)
    x = _nonfinite((65, 129), rng)
    region = rng.random((65, 129)) < 0.6
    keep = x.copy()
    want = _noise_np.noise(x, region)
    _check_noise(noise.image_noise(x, region=region), want, "numpy")
    _check_noise(noise.image_noise(torch.from_numpy(x), region=torch.from_numpy(region)), want, "torch host")
    _check_noise(noise.image_noise(_t(x), region=region.astype(np.uint8)), want, "torch device")
    _check_noise(noise.image_noise(x[:, ::2]), _noise_np.noise(x[:, ::2]), "strided numpy")
    assert np.array_equal(x.view(np.int64), keep.view(np.int64))


def test_gaussian_noise_with_bright_pixels_at_512():
    rng = np.random.default_rng(12)
    x = 0.02 * rng.standard_normal((512, 512))
    x[100, 200], x[300, 17], x[511, 511], x[0, 0] = 1.0, 0.5, -0.8, 2.0
    got, want = noise.device_image_noise(_t(x)), _noise_np.noise(x)
    _check_noise(got, want, "gaussian")
    assert got["sigma"] == want["sigma"] == noise.MAD_TO_SIGMA * want["mad"]
    print("sigma", got["sigma"], "true", 0.02)  # the estimate itself: not a tolerance on the true sigma
