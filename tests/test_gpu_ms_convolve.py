"""
GPU tests of the separable scale convolution (`cip_ms_convolve`, through
`multiscale.device_ms_convolve`).

The operator's rounding and its tap order are its definition
(include/cip_ms.h), so every case asserts equality of BITS with the numpy
statement `_ms_np.convolve`, which is handed the same tap table as the device:
no test shares an exp with the library, and there are no tolerances.

The row pass takes 256-column segments of 4 rows and the column pass 4 x 64
pixels per workgroup; the shapes below are smaller than a workgroup, partial
in both, and more than one workgroup along each axis.
"""

import numpy as np
import pytest

import _ms_np
from ska_sdp_cip_amd import _lib, multiscale

pytestmark = pytest.mark.gpu


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    """Equal bits (NaNs in the same places; no -0 / +0 confusion)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


def _taps(radius, seed=1):
    """2 R + 1 seeded taps of both signs, not symmetric: a pass that ran its taps backwards would show."""
    return np.random.default_rng(seed + radius).standard_normal(2 * radius + 1) / (radius + 1)


def _image(shape, seed=2):
    return np.random.default_rng(seed).standard_normal(shape)


def _check(img, taps):
    got = multiscale.device_ms_convolve(_t(img), None, taps=taps)
    assert _same(got.cpu().numpy(), _ms_np.convolve(img, taps))
    return got


@pytest.mark.parametrize("shape", [(1, 1), (5, 300), (300, 5), (64, 256), (70, 45)])
@pytest.mark.parametrize("radius", [0, 3, 20])
def test_shapes(shape, radius):
    _check(_image(shape), _taps(radius))


@pytest.mark.parametrize("shape, radius", [((7, 9), 0), ((7, 9), 3), ((7, 9), 20), ((130, 140), 128)])
def test_radius_against_image_size(shape, radius):
    # 7 x 9 under radius 20: every output misses taps on both sides; 128: the largest table
    _check(_image(shape, seed=5), _taps(radius))


def test_scale_taps_of_the_library():
    img = _image((70, 45), seed=7)
    for width in (1.0, 4.0, 10.0):
        got = multiscale.device_ms_convolve(_t(img), width)
        assert _same(got.cpu().numpy(), _ms_np.convolve(img, multiscale.scale_taps(width)))
        # unit-sum taps keep the flux of an interior source
    spot = np.zeros((96, 96))
    spot[48, 48] = 2.0
    assert multiscale.device_ms_convolve(_t(spot), 10.0).sum().item() == pytest.approx(2.0, abs=1e-14)


def test_width_zero_is_a_copy():
    import torch

    img = _image((70, 45))
    img[3, 4] = -0.0
    src = _t(img)
    got = multiscale.device_ms_convolve(src, 0.0)
    assert got.data_ptr() != src.data_ptr() and _same(got.cpu().numpy(), img)
    out = torch.empty_like(src)
    assert multiscale.device_ms_convolve(src, 0, out=out) is out and _same(out.cpu().numpy(), img)


def test_out_may_be_the_input():
    img, taps = _image((70, 300)), _taps(20)
    buf = _t(img)
    got = multiscale.device_ms_convolve(buf, None, taps=taps, out=buf)
    assert got is buf and _same(buf.cpu().numpy(), _ms_np.convolve(img, taps))


def test_base_aligned_to_8_bytes_only():
    import torch

    img, taps = _image((64, 130)), _taps(3)
    storage = torch.zeros(img.size + 2, dtype=torch.float64, device="cuda")
    view = storage[1:-1].view(img.shape)
    view.copy_(_t(img))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    out_storage = torch.zeros(img.size + 2, dtype=torch.float64, device="cuda")
    out = out_storage[1:-1].view(img.shape)
    multiscale.device_ms_convolve(view, None, taps=taps, out=out)
    assert _same(out.cpu().numpy(), _ms_np.convolve(img, taps))
    assert out_storage[0].item() == 0.0 and out_storage[-1].item() == 0.0  # nothing written beside the image
    assert _same(view.cpu().numpy(), img)


def test_nan_and_negative_zero():
    img = _image((70, 45))
    img[10, 10], img[69, 44] = np.nan, np.inf
    taps = _taps(3)
    got = _check(img, taps).cpu().numpy()
    assert np.isnan(got[7:14, 7:14]).all() and not np.isnan(got[:6]).any()  # NaN spreads R each way, no further
    # -0.0 everywhere: +0.0 + (t * -0.0) is +0.0 for t > 0, and the sum starts at +0.0 either way
    zeros = np.full((9, 11), -0.0)
    out = _check(zeros, np.abs(_taps(3)))
    assert not np.signbit(out.cpu().numpy()).any()
    _check(zeros, _taps(3))


def test_two_calls_give_the_same_bits_and_the_table_follows_the_taps():
    img = _image((130, 140), seed=9)
    a, b = _taps(20, seed=1), _taps(20, seed=4)  # the same radius, other values: the device table must change
    first = _check(img, a).cpu().numpy()
    assert _same(_check(img, a).cpu().numpy(), first)
    assert not _same(_check(img, b).cpu().numpy(), first)
    assert _same(_check(img, a).cpu().numpy(), first)


def test_alternating_shapes_release_and_stream():
    import torch

    cases = [(_image((70, 45)), _taps(3)), (_image((300, 260), seed=4), _taps(20)), (_image((5, 300)), _taps(0))]
    for img, taps in cases + cases[::-1]:
        _check(img, taps)
    torch.cuda.synchronize()
    assert _lib.lib().cip_release_workspace() == 0
    _check(*cases[1])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _check(*cases[0])
    stream.synchronize()


def test_invalid_arguments():
    import torch

    img = _t(_image((8, 8)))
    for kw in (dict(taps=np.ones(4)), dict(taps=np.ones((3, 3))), dict(taps=np.array([0.5, np.nan, 0.5])),
               dict(taps=np.ones(2 * 129 + 1)), dict(out=torch.empty((8, 9), dtype=torch.float64, device="cuda")),
               dict(out=torch.empty((8, 8), dtype=torch.float32, device="cuda"))):
        with pytest.raises(ValueError):
            multiscale.device_ms_convolve(img, 2.0, **kw)
    for width in (0.5, -1.0, float("nan"), 60.0):  # 60 px needs a radius above 128 at 1e-8
        with pytest.raises(ValueError):
            multiscale.device_ms_convolve(img, width)
    with pytest.raises(ValueError):
        multiscale.device_ms_convolve(img.float(), 2.0)
    with pytest.raises(ValueError):
        multiscale.device_ms_convolve(img.cpu(), 2.0)
