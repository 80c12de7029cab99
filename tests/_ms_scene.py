"""
The scene of the multiscale major-cycle tests (test_gpu_ms_major.py on the
device, test_ms_scene_host.py in numpy): a 256 x 256 image from `synthetic`
Earth-rotation tracks (32 antennas, 16 dumps of 15 minutes, two channels),
one circular Gaussian source of FWHM 8 pixels holding 5.0 flux units and two
point sources, 2-D imaging (no w term), natural weights.
"""

import numpy as np

from ska_sdp_cip_amd import synthetic

C = 299792458.0
NPIX = 256
FREQ = np.array([1.0e9, 1.05e9])
GAUSS = ((140, 120), 5.0, 8.0)  # pixel, flux, FWHM in pixels
POINTS = (((90, 170), 1.0), ((180, 60), 0.5))  # pixel, flux
BOX = 20  # half-width of the box round the Gaussian source: 5 sigma of its profile
WIDTHS = [0, 4, 8]
CLEAN = dict(gain=0.1, niter=100)


def tracks():
    """(uvw, freq, pixsize)."""
    uvw = synthetic.uvw_tracks(496 * 16, n_ant=32, array_radius_m=1000.0, dump_s=900.0, seed=5)
    # fill 0.5: about four pixels across the PSF's main lobe, enough for the clean-beam fit
    return uvw, FREQ.copy(), synthetic.pixel_size_for_grid(uvw, FREQ, NPIX, fill=0.5)


def components(pix):
    """(lm (3, 2), flux (3, 1), shape (3, 3)) of the catalogue, as `skymodel.SkyModel` takes them."""
    rows = [(GAUSS[0], GAUSS[1], GAUSS[2] * pix)] + [(pos, flux, 0.0) for pos, flux in POINTS]
    lm = np.array([[(i - NPIX // 2) * pix, (j - NPIX // 2) * pix] for (i, j), _, _ in rows])
    flux = np.array([[f] for _, f, _ in rows])
    shape = np.array([[w, w, 0.0] for _, _, w in rows])
    return lm, flux, shape


def visibilities(uvw, freq, pix):
    """The catalogue's visibilities in numpy (the sign of `synthetic.predict_visibilities`, no w term):
    flux exp(-pi^2 fwhm^2 (u^2 + v^2) / (4 ln 2)) exp(-2 pi i (u l + v m)), u and v in wavelengths."""
    lm, flux, shape = components(pix)
    u = uvw[:, 0:1] * freq[None, :] / C
    v = uvw[:, 1:2] * freq[None, :] / C
    vis = np.zeros(u.shape, dtype=np.complex128)
    for (l, m), f, fwhm in zip(lm, flux[:, 0], shape[:, 0]):  # noqa: E741
        envelope = np.exp(-(np.pi * fwhm) ** 2 * (u * u + v * v) / (4.0 * np.log(2.0)))
        vis += f * envelope * np.exp(-2j * np.pi * (u * l + v * m))
    return vis


def box_flux(model):
    """The model image's flux in the box round the Gaussian source."""
    (i, j), _, _ = GAUSS
    return float(model[i - BOX:i + BOX + 1, j - BOX:j + BOX + 1].sum())
