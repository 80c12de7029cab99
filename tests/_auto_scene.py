"""
The scene of the noise-driven major-cycle tests (test_gpu_auto_major.py on the
device, test_noise_host.py in numpy): the tracks of `_ms_scene` at 256 x 256
with its two point sources (no Gaussian source) plus seeded complex Gaussian
visibility noise, 2-D imaging, natural weights.

NOISE is the standard deviation of the real and of the imaginary part of every
visibility. With N = 15872 visibilities of unit weight it puts NOISE / sqrt(N)
= 0.02 flux units of noise into a pixel of the dirty image; the sidelobes of
the two sources add to the first residual's spread, and test_noise_host.py
shows that the faint source (0.5) still stands at 10 sigma or more.
"""

import numpy as np

import _ms_scene as sc

NPIX = sc.NPIX
POINTS = sc.POINTS
NOISE = 2.5
SEED = 11
AUTO = dict(auto_threshold=3.0, auto_mask=(5.0, 3.0))
MAJOR = dict(n_major=3, niter=200, gain=0.1, do_wstacking=False)


def point_visibilities(uvw, freq, pix, points=POINTS):
    """The point sources' visibilities (the sign and the 2-D phase of `_ms_scene.visibilities`)."""
    u = uvw[:, 0:1] * freq[None, :] / sc.C
    v = uvw[:, 1:2] * freq[None, :] / sc.C
    vis = np.zeros(u.shape, dtype=np.complex128)
    for (i, j), flux in points:
        l, m = (i - NPIX // 2) * pix, (j - NPIX // 2) * pix  # noqa: E741
        vis += flux * np.exp(-2j * np.pi * (u * l + v * m))
    return vis


def noisy_visibilities(uvw, freq, pix):
    """The two sources plus the seeded noise."""
    rng = np.random.default_rng(SEED)
    vis = point_visibilities(uvw, freq, pix)
    return vis + NOISE * (rng.standard_normal(vis.shape) + 1j * rng.standard_normal(vis.shape))


def model_visibilities(uvw, freq, pix, model):
    """The visibilities of a delta model image: its nonzero pixels as point sources."""
    idx = np.argwhere(model != 0.0)
    return point_visibilities(uvw, freq, pix, [((int(i), int(j)), model[i, j]) for i, j in idx])
