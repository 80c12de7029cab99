"""
Host-side checks of the degridder's interface (no GPU): the built library
exports `cip_dirty2ms`, its flag does not collide, the Python entry points
exist and refuse to run without a GPU, and the zero-padding index convention
the image-preparation kernel follows is the inverse of `oracle._crop`.
"""

import numpy as np
import pytest

import oracle
from ska_sdp_cip_amd import _lib


def test_library_exports_cip_dirty2ms():
    so = _lib.lib()
    assert "cip_dirty2ms" in _lib.EXPORTED_SYMBOLS
    assert hasattr(so, "cip_dirty2ms")
    assert len(so.cip_dirty2ms.argtypes) == 18


def test_subtract_flag_is_a_free_bit():
    flags = {name: getattr(_lib, name) for name in
             ("CIP_WSTACKING", "CIP_ACC_SINGLE", "CIP_PSF", "CIP_NORMALISE", "CIP_ASYNC", "CIP_PIPELINE",
              "CIP_REUSE_PLAN", "CIP_GRID_ZEROED", "CIP_SUBTRACT")}
    assert bin(flags["CIP_SUBTRACT"]).count("1") == 1
    assert len(set(flags.values())) == len(flags)
    others = 0
    for name, bit in flags.items():
        if name != "CIP_SUBTRACT":
            others |= bit
    assert flags["CIP_SUBTRACT"] & others == 0


def test_header_declares_the_entry_point_and_flag():
    from pathlib import Path

    text = (Path(__file__).resolve().parents[1] / "include" / "cip.h").read_text()
    assert "int cip_dirty2ms(" in text
    assert f"#define CIP_SUBTRACT {_lib.CIP_SUBTRACT}" in text


def test_entry_points_need_a_gpu():
    import torch

    import ska_sdp_cip_amd as pkg
    from ska_sdp_cip_amd import gridder, predict

    assert pkg.dirty2ms is gridder.dirty2ms
    assert pkg.ducc_predict is predict.ducc_predict and pkg.device_residual is predict.device_residual
    assert callable(gridder.device_dirty2ms)
    if torch.cuda.is_available():
        return  # the refusal shows only without a GPU
    uvw, f, img = np.zeros((2, 3)), np.array([1.0e9]), np.zeros((8, 8))
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        gridder.dirty2ms(uvw, f, img, None, 1e-4, 1e-4)
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        predict.ducc_predict(uvw, f, img, 1.0)
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        predict.device_residual(torch.zeros((2, 3)), torch.ones(1), torch.zeros((2, 1), dtype=torch.complex128),
                                torch.zeros((8, 8)), 1e-4)


def _pad(image, nu, nv):
    """The image-preparation kernel's index map (cip_degrid.hip
    degrid_pad_kernel), restated: grid cell x holds image row x + nx / 2 for
    x < nx / 2, row x - nu + nx / 2 for x >= nu - nx / 2, zero between; the
    (-1)^(p+q) sign rides on the image (degrid_image_kernel)."""
    nx, ny = image.shape
    hx, hy = nx // 2, ny // 2
    p = np.arange(nx) - hx
    q = np.arange(ny) - hy
    sgn = np.where((p[:, None] + q[None, :]) % 2 == 0, 1.0, -1.0)
    plane = np.zeros((nu, nv), dtype=np.complex128)
    for x in range(nu):
        i = x + hx if x < nx - hx else (x - nu + hx if x >= nu - hx else -1)
        if i < 0:
            continue
        for y in range(nv):
            j = y + hy if y < ny - hy else (y - nv + hy if y >= nv - hy else -1)
            if j >= 0:
                plane[x, y] = sgn[i, j] * image[i, j]
    return plane


@pytest.mark.parametrize("nx,ny,nu,nv", [(8, 8, 16, 16), (6, 10, 12, 20), (66, 34, 132, 70)])
def test_pad_is_the_inverse_of_crop(nx, ny, nu, nv):
    img = np.random.default_rng(0).standard_normal((nx, ny))
    plane = _pad(img, nu, nv)
    assert np.array_equal(oracle._crop(plane, nx, ny), img)  # signs included
    assert np.count_nonzero(plane) == nx * ny  # everything else is padding
    # and as operators: <crop(G), I> == <G, pad(I)> for any G
    g = np.random.default_rng(1).standard_normal((nu, nv))
    assert np.isclose((oracle._crop(g, nx, ny) * img).sum(), (g * plane.real).sum(), rtol=1e-13)
