"""
The multiscale-against-Hogbom comparison of test_gpu_ms_major.py in numpy (no
GPU): the oracle's dirty image and PSF of the scene of `_ms_scene`, the minor
cycles `_ms_np.ms_clean` (widths 0 / 4 / 8 pixels, the default weights) and
`_clean_np.hogbom_clean` at the same gain and niter, and the flux each model
puts into the box round the Gaussian source (catalogue: 5.0).

Measured with gain 0.1 (the PSF has 16 % sidelobes and a main lobe of about 4
pixels FWHM, so the 8-pixel source is resolved):

    niter   multiscale   |error|   Hogbom   |error|
      50      4.517       0.483     1.785    3.215
     100      4.828       0.172     2.810    2.190
     150      4.873       0.127     3.437    1.563
     300      4.922       0.078     4.318    0.682

The test runs niter = 100, where the numpy run shows the claim with a factor
of 12 between the two errors; the assertion is the strict inequality.
"""

import numpy as np

import _clean_np
import _ms_np
import _ms_scene as sc
import oracle


def test_multiscale_recovers_the_extended_flux_hogbom_misses():
    uvw, freq, pix = sc.tracks()
    vis = sc.visibilities(uvw, freq, pix)
    wgt = np.ones(vis.shape)
    n = sc.NPIX
    dirty = oracle.ms2dirty(uvw, freq, vis, wgt, n, n, pix, pix) / wgt.sum()
    psf = oracle.ms2dirty(uvw, freq, np.ones_like(vis), wgt, n, n, pix, pix) / wgt.sum()
    assert abs(psf[n // 2, n // 2] - 1.0) < 1e-3 and psf.argmax() == (n // 2) * n + n // 2
    cross = _ms_np.cross_psfs(psf, sc.WIDTHS)
    select_weight, flux_scale = _ms_np.scale_weights(cross, sc.WIDTHS)
    models, residuals, info = _ms_np.ms_clean(_ms_np.scale_residuals(dirty, sc.WIDTHS), cross, select_weight,
                                              flux_scale, **sc.CLEAN)
    h_model, h_residual, h_info = _clean_np.hogbom_clean(dirty, psf, **sc.CLEAN)
    assert info["niter_done"] == h_info["niter_done"] == sc.CLEAN["niter"]
    want = sc.GAUSS[1]
    ms_flux, h_flux = sc.box_flux(_ms_np.ms_model(models, sc.WIDTHS)), sc.box_flux(h_model)
    print("catalogue", want, "multiscale", ms_flux, "Hogbom", h_flux)
    print("components per scale", np.bincount(info["comp_scale"], minlength=3).tolist())
    print("residual rms: multiscale", residuals[0].std(), "Hogbom", h_residual.std())
    assert abs(ms_flux - want) < abs(h_flux - want)
    assert info["comp_scale"].max() == 2  # the widest scale takes part
