"""
The oracle pipeline (gridding + FFT + correction [+ w-stacking]) against the
fp64 direct DFT that defines ms2dirty, for every supported kernel support: the
measured accuracy is the table behind the epsilon -> support choice
(cip_params.hip support_for_epsilon, oracle.support_for_epsilon).
"""
import numpy as np
import pytest

import oracle
from ska_sdp_cip_amd import synthetic as syn

EXPECTED = {4: 3e-3, 6: 3e-5, 8: 4e-7, 10: 6e-9, 12: 8e-11, 14: 2e-12, 16: 1e-13}


@pytest.fixture(scope="module")
def case():
    ms = syn.make_measurement_set(3_000, 2, n_ant=16, array_radius_m=1000.0, fov_l=0.01, seed=1)
    vis_i, _, _, eff = oracle.stokes_i(ms.visibilities(), ms.flags(), ms.weights())
    uvw, f = ms.uvw(), ms.channel_frequencies()
    npix = 64
    px = syn.pixel_size_for_grid(uvw, f, npix, fill=0.8)
    dft = {ws: oracle.dft_dirty(uvw, f, vis_i, eff, npix, npix, px, px, apply_w=ws) for ws in (False, True)}
    return uvw, f, vis_i, eff, npix, px, dft


@pytest.mark.parametrize("support", sorted(EXPECTED))
@pytest.mark.parametrize("wstack", [False, True])
def test_oracle_vs_dft(case, support, wstack):
    uvw, f, vis, w, npix, px, dft = case
    img = oracle.ms2dirty(uvw, f, vis, w, npix, npix, px, px, support=support, do_wstacking=wstack)
    err = np.abs(img - dft[wstack]).max() / w.astype(np.float64).sum()
    assert err < EXPECTED[support], err
    assert oracle.support_for_epsilon(EXPECTED[support] * 0.99) >= support


@pytest.mark.parametrize("wstack", [False, True])
def test_oracle_wraps_periodic_uv_exactly(wstack):
    # pixel 3x too coarse: most baselines lie beyond the grid and wrap; the DFT
    # on the pixel grid is periodic in u with period 1 / pixsize, so the
    # wrapped gridder must still reproduce it
    ms = syn.make_measurement_set(3_000, 2, n_ant=16, array_radius_m=1000.0, fov_l=0.02, seed=1)
    vis, _, _, w = oracle.stokes_i(ms.visibilities(), ms.flags(), ms.weights())
    uvw, f = ms.uvw(), ms.channel_frequencies()
    npix = 64
    px = syn.pixel_size_for_grid(uvw, f, npix) * 3.0
    dft = oracle.dft_dirty(uvw, f, vis, w, npix, npix, px, px, apply_w=wstack)
    img = oracle.ms2dirty(uvw, f, vis, w, npix, npix, px, px, support=12, do_wstacking=wstack)
    assert np.abs(img - dft).max() / w.astype(np.float64).sum() < 1e-10


# max |image - DFT| / sum(w) bounds of the large supports. Their shape beta
# keeps the ES kernel's edge ratio F(1/4)/F(0) >= 0.03 (2.3 W up to W = 24,
# larger beyond: oracle.es_beta, tools/gen_es_kernels.py), so the grid and w
# corrections stay conditioned like a W = 24 kernel's and the aliasing stays
# at the fp64 floor: measured <= 4e-14 in 2-D and with w-stacking (at
# beta = 2.3 W: 1e-11 .. 2e-7).
LARGE_BOUND = 1e-12


@pytest.mark.parametrize("support", [24, 32, 48, 64])
@pytest.mark.parametrize("wstack", [False, True])
def test_oracle_large_supports_vs_dft(case, support, wstack):
    uvw, f, vis, w, npix, px, dft = case
    img = oracle.ms2dirty(uvw, f, vis, w, npix, npix, px, px, support=support, do_wstacking=wstack)
    err = np.abs(img - dft[wstack]).max() / w.astype(np.float64).sum()
    assert err < LARGE_BOUND, err


@pytest.mark.parametrize("support", [4, 8, 16, 24, 32, 48, 64])
def test_kernel_shape_rule(support):
    # the tabulated kernel (es_kernels.h / .json, shared data) is the ES
    # function of the oracle's restated beta rule, to fp64 fit accuracy
    import json
    from pathlib import Path

    table = json.loads((Path(oracle.__file__).resolve().parents[1] / "ska-sdp-continuum-imaging-pipeline_amd" /
                        "ska_sdp_cip_amd" / "es_kernels.json").read_text())[str(support)]
    beta = oracle.es_beta(support)
    assert abs(table["beta"] - beta) < 1e-8 * beta
    assert oracle.choose_params(64, 64, 1e-5, 1e-5, support=support)["beta"] == beta
    r = oracle.es_edge_ratio(support, beta)
    if support > 24:
        assert abs(r - oracle.LARGE_EDGE_RATIO) < 1e-6
    else:
        assert beta == 2.3 * support and (support <= 16 or r >= oracle.LARGE_EDGE_RATIO)
    if support > 16:  # degree-15 pieces reproduce the ES formula (W <= 16: the polynomial IS the kernel)
        for k in range(0, support // 2, max(1, support // 16)):
            for y in (-0.9, -0.3, 0.0, 0.45, 0.99):
                t = 2.0 * (k + 1 - (y + 1) / 2 - support / 2) / support
                ref = np.exp(table["beta"] * (np.sqrt(1 - t * t) - 1)) if abs(t) < 1 else 0.0
                assert abs(oracle.kernel_value(support, k, y) - ref) < 1e-13


@pytest.mark.parametrize("support", [6, 8, 12])
@pytest.mark.parametrize("npix", [64, 66])  # 66: odd tile count (132-cell grid -> 5 tiles): the serial edge phase
def test_cpu_baseline_equals_oracle(case, support, npix):
    # bench.py's cpu_baseline times the tiled restatement (oracle/cpu_baseline.c):
    # it must grid what the oracle grids (same kernel, placement and wrap)
    uvw, f, vis, w, _, px, _ = case
    prm = oracle.choose_params(npix, npix, px, px, support=support)
    ref = oracle.grid_plane(uvw, f, vis, w, prm, px, px, 0, 4)
    got = oracle.grid_plane_tiled(uvw, f, vis, w, prm, px, px, 4)
    scale = float(np.abs(w.astype(np.float64) * vis).sum())
    assert np.abs(got - ref).max() / scale < 1e-12
    img = oracle.baseline_ms2dirty(uvw, f, vis, w, npix, npix, px, px, support=support, nthreads=4)
    img_ref = oracle.ms2dirty(uvw, f, vis, w, npix, npix, px, px, support=support, nthreads=4)
    assert np.abs(img - img_ref).max() / w.astype(np.float64).sum() < 1e-12
