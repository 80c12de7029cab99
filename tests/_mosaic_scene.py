"""
The scene of the mosaic's method-error tests (test_mosaic_host.py, and the end
to end test of test_gpu_mosaic.py): 600 rows of a 12-antenna, 4 m array, 2
channels, 6 point sources in a field 0.32 rad across 64 pixels, the pixel size
chosen so that the longest |u| or |v| is NU = 0.125 cycles per pixel; 2 x 2
facets of 48^2 pixels from `facet_layout`, support 16, w-stacking. The
reference is the direct DFT of the whole field with the w term.
"""
from functools import lru_cache

import numpy as np

import _mosaic_np as mnp
import oracle
from ska_sdp_cip_amd import synthetic as syn
from ska_sdp_cip_amd.invert import pixel_size_lm
from ska_sdp_cip_amd.mosaic import facet_layout

NU = 0.125
NPIX = 64
FACET = 48
SUPPORT = 16
SEED = 8


@lru_cache(maxsize=None)
def scene():
    """uvw (600, 3), freq (2,), vis (600, 2) complex64, pixel size in arcsec
    and in direction cosines (the round trip the pipeline makes)."""
    uvw = syn.uvw_tracks(600, 12, array_radius_m=4.0, seed=SEED)
    freq = syn.channel_frequencies(2)
    px = NU / (np.abs(uvw[:, :2]).max() * freq.max() / syn.SPEED_OF_LIGHT)
    asec = syn.pixel_size_asec(px)
    pix = pixel_size_lm(asec)
    src = syn.random_sources(6, 0.8 * NPIX * pix, np.random.default_rng(SEED))
    vis = syn.predict_visibilities(uvw, freq, src).astype(np.complex64)
    return uvw, freq, vis, asec, pix


def centres(half):
    return facet_layout(NPIX, NPIX, scene()[4], FACET, half=half, trim=0)


@lru_cache(maxsize=None)
def reference():
    """The w-term-correct dirty image of the whole field over the weight sum."""
    uvw, freq, vis, _, pix = scene()
    return oracle.dft_dirty(uvw, freq, vis, None, NPIX, NPIX, pix, pix, apply_w=True) / vis.size


@lru_cache(maxsize=None)
def oracle_facets(half, store_complex64=False):
    """The oracle's w-stacked facet images (over the weight sum) at
    `centres(half)`; `store_complex64`: the rephased visibilities rounded to
    complex64, as cip_facet_rephase stores them."""
    uvw, freq, vis, _, pix = scene()
    out = []
    for c in centres(half):
        uvw_f, vis_f = oracle.facet_rephase(uvw, freq, vis, *c)
        if store_complex64:
            vis_f = vis_f.astype(np.complex64)
        out.append(oracle.ms2dirty(uvw_f, freq, vis_f, None, FACET, FACET, pix, pix, support=SUPPORT,
                                   do_wstacking=True) / vis.size)
    return out


def method_error(half, nscale=True, store_complex64=False):
    """(max |mosaic - DFT| over the weight sum, n_uncovered) of the numpy
    statement over the oracle's facets."""
    pix = scene()[4]
    g = mnp.Geom(NPIX, NPIX, pix, pix, FACET, FACET, pix, pix, half, mnp.beta_rule(half, NU), 0, 0.0,
                 mnp.NSCALE if nscale else 0)
    img, missed = mnp.mosaic(g, oracle_facets(half, store_complex64), centres(half))
    return float(np.abs(img[0] - reference()).max()), missed
