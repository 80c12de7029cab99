"""
GPU test of `calibrate.device_selfcal(..., initial_sky_model=...)` on the 64 x 64,
12-antenna scene of test_gpu_selfcal.py, with the sky model set to the true
sources: the loop solves its first gains against the catalogue instead of
imaging the uncalibrated data.

The first gains are checked against `device_gaincal` of the same data against
a model column computed on the host by `_dft_np` and cast to complex64: the two
columns differ by complex64 rounding at most (6e-8 relative per sample), which
is the whole error budget of the 1e-6 bound on the gains. The quality
reference is the blind loop of the parent code path, run in the same test:
round 0 with the sky model is no worse than the blind loop's last round. For
the residual rms "no worse" is "not larger". For the first major cycle's peak
it is "not further from the peak of the uncorrupted data" (the parent's
`device_ms2dirty` on the scene's clean visibilities, computed here too):
phase errors lower the peak, but self-calibration against its own model can
also push it above the truth, so a larger peak is not a better one.
"""

import numpy as np
import pytest

import _dft_np as dnp
from ska_sdp_cip_amd import calibrate, skymodel
from test_gpu_selfcal import MAJOR, N_ANT, N_INT, NPIX, ROUNDS, SOURCES, _first_peak, _t, selfcal_scene

pytestmark = pytest.mark.gpu


def true_sources(pix):
    lm = np.array([[(i - NPIX // 2) * pix, (j - NPIX // 2) * pix] for (i, j), _ in SOURCES])
    return lm, np.array([[flux] for _, flux in SOURCES])


@pytest.fixture(scope="module")
def scene(gpu_device):
    s = selfcal_scene()
    d = {k: _t(s[k]) for k in ("uvw", "freq", "vis", "bad", "wgt")}
    d.update(pix=s["pix"], cols=[_t(c) for c in s["cols"]], host=s)
    d["true_peak"] = _first_peak(d, d["vis"])
    d["threshold"] = 0.02 * _first_peak(d, d["bad"])
    lm, flux = true_sources(s["pix"])
    d["sky"] = skymodel.SkyModel(_t(lm), _t(flux))
    return d


def _selfcal(s, n_rounds, **kw):
    return calibrate.device_selfcal(s["uvw"], s["freq"], s["bad"], s["wgt"], *s["cols"], NPIX, s["pix"],
                                    n_rounds=n_rounds, threshold=s["threshold"], **MAJOR, **kw)


@pytest.fixture(scope="module")
def with_model(scene):
    return _selfcal(scene, 1, initial_sky_model=scene["sky"])


def test_initial_gains_equal_gaincal_against_the_host_column(scene, with_model):
    import torch

    host = scene["host"]
    lm, flux = true_sources(host["pix"])
    column, _, _ = dnp.predict(host["uvw"], host["freq"], lm, flux, w_term=False)
    assert np.abs(column - host["vis"]).max() <= 1e-6  # the scene's own uncorrupted visibilities (complex64)
    ref, ok, info = calibrate.device_gaincal(scene["bad"], _t(column.astype(np.complex64)), scene["wgt"],
                                             *scene["cols"], N_ANT, N_INT, niter=50, tol=1e-8, refant=0,
                                             phase_only=True)
    out = with_model
    err = float((out["initial_gains"] - ref).abs().max())
    print(f"initial gains vs gaincal against the host column: {err:.3e}; solver {out['initial_solver']}")
    assert err <= 1e-6
    assert tuple(out["initial_gains"].shape) == (N_INT, N_ANT) and out["initial_gains"].dtype == torch.complex128
    assert torch.equal(out["initial_ant_ok"], ok) and bool(ok.all())
    assert out["initial_solver"]["n_converged"] == info["n_converged"] == N_INT and "iters" not in out["initial_solver"]
    # the true sources on noise-free data: the first gains are the truth, up to the solver's tolerance
    import _cal_np as cnp

    assert np.abs(out["initial_gains"].cpu().numpy() - cnp.rotate_to(host["gains"])).max() <= 1e-5
    assert len(out["round_peaks"]) == len(out["round_rms"]) == 2 and len(out["solver"]) == 1


def test_first_round_is_no_worse_than_the_blind_loops_last(scene, with_model):
    blind = _selfcal(scene, ROUNDS)  # the parent's code path: the reference
    out = with_model
    print("with the sky model: peaks", out["round_peaks"], "rms", out["round_rms"])
    print("blind:              peaks", blind["round_peaks"], "rms", blind["round_rms"])
    truth = scene["true_peak"]
    print(f"peak of the uncorrupted data {truth!r}")
    assert "initial_gains" not in blind
    assert abs(out["round_peaks"][0] - truth) <= abs(blind["round_peaks"][-1] - truth)
    assert out["round_rms"][0] <= blind["round_rms"][-1]
    # and far better than the blind loop's own first round, which images the uncalibrated data
    assert abs(out["round_peaks"][0] - truth) < 0.01 * abs(blind["round_peaks"][0] - truth)
    assert out["round_rms"][0] < 0.5 * blind["round_rms"][0]


def test_without_a_model_nothing_changes(scene):
    import torch

    plain = _selfcal(scene, 1)
    none = _selfcal(scene, 1, initial_sky_model=None)
    assert set(plain) == set(none) and "initial_gains" not in none
    for key, a in plain.items():
        b = none[key]
        if torch.is_tensor(a):
            assert torch.equal(a, b), key
        else:
            assert a == b, key
