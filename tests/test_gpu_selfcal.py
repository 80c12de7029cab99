"""
GPU test of the self-calibration loop (`calibrate.device_selfcal`): phase-only
self-calibration of a 12-antenna scene whose gains carry phase errors of up to
0.5 rad.

Scene: `uvw_tracks(66 * 16, 12, array_radius_m=1000, dump_s=600, seed=23)` with
w zeroed (16 dumps of 66 baselines), channels at 1.0 and 1.05 GHz, 64 x 64
pixels of 0.3 / (max |u, v| f_max / c) rad, sources of 1.0, 0.6 and -0.3 at
pixels (40, 25), (20, 44) and (50, 50), unit weights, 2 intervals of 8 dumps,
gains `random_gains(2, 12, 0.0, 0.5, default_rng(23))`. Major cycles: gain 0.2,
threshold 0.02 of the loop's first dirty peak, cycle_fraction 0.1, n_major 4,
niter 5000; 3 self-calibration rounds from unit gains, reference antenna 0.

Checked on the CPU before relying on it (exact DFT inverts and predicts,
`_clean_np.hogbom_clean`, `_cal_np.gaincal` / `_cal_np.apply`, fp64 data):

    round   flux at (40, 25)   residual rms   worst gain error   solver iterations
    0       0.86824            7.87e-3        0.369              16, 16
    1       0.94654            6.38e-3        0.0733             16, 16
    2       0.97310            2.77e-3        0.0141             16, 16
    3       0.97881            2.13e-3        (gains of round 2)

The same loop on the uncorrupted data gives 0.98052 and 2.05e-3. So the last
round is within 1.7e-3 of the uncorrupted flux (bound 0.01), round 0 misses it
by 0.112 (bound 0.05), the residual rms falls to 0.27 of round 0's (bound 0.5)
and the gains end 0.0141 from the truth (bound 0.02). The gridder's
epsilon = 1e-4 moves these figures in the fourth digit.
"""

import numpy as np
import pytest

import _cal_np as cnp
from ska_sdp_cip_amd import calibrate, deconvolve, gridder, synthetic

pytestmark = pytest.mark.gpu

C = 299792458.0
NPIX, N_ANT, N_INT = 64, 12, 2
SOURCES = (((40, 25), 1.0), ((20, 44), 0.6), ((50, 50), -0.3))
MAJOR = dict(n_major=4, niter=5000, gain=0.2, cycle_fraction=0.1, do_wstacking=False)
ROUNDS = 3


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def selfcal_scene():
    uvw = synthetic.uvw_tracks(66 * 16, N_ANT, array_radius_m=1000, dump_s=600, seed=23)
    uvw[:, 2] = 0.0
    freq = np.array([1.0e9, 1.05e9])
    pix = 0.3 / (np.abs(uvw[:, :2]).max() * freq.max() / C)
    a1, a2, t = synthetic.baseline_indices(len(uvw), N_ANT)
    interval = calibrate.solution_intervals(t, 8)
    vis = np.zeros((len(uvw), 2), dtype=np.complex128)
    for (i, j), flux in SOURCES:
        l, m = (i - NPIX // 2) * pix, (j - NPIX // 2) * pix  # noqa: E741
        vis += flux * np.exp(-2j * np.pi * freq[None, :] / C * (uvw[:, 0] * l + uvw[:, 1] * m)[:, None])
    gains = synthetic.random_gains(N_INT, N_ANT, 0.0, 0.5, np.random.default_rng(23))
    bad = gains[interval, a1][:, None] * vis * np.conj(gains[interval, a2])[:, None]
    return dict(uvw=uvw, freq=freq, pix=pix, cols=(a1, a2, interval), vis=vis.astype(np.complex64),
                bad=bad.astype(np.complex64), wgt=np.ones(vis.shape, dtype=np.float32), gains=gains)


def _first_peak(d, vis):
    dirty, _ = gridder.device_ms2dirty(d["uvw"], d["freq"], vis, d["wgt"], NPIX, NPIX, d["pix"], d["pix"],
                                       normalise=True)
    return float(dirty.abs().max())


@pytest.fixture(scope="module")
def scene(gpu_device):
    s = selfcal_scene()
    assert int(s["cols"][2].max()) == N_INT - 1 and np.abs(np.angle(s["gains"])).max() > 0.4
    d = {k: _t(s[k]) for k in ("uvw", "freq", "vis", "bad", "wgt")}
    d.update(pix=s["pix"], cols=[_t(c) for c in s["cols"]], gains=s["gains"])
    d["clean_threshold"] = 0.02 * _first_peak(d, d["vis"])
    d["first"] = _first_peak(d, d["bad"])
    d["threshold"] = 0.02 * d["first"]
    return d


@pytest.fixture(scope="module")
def uncorrupted(scene):
    s = scene
    return calibrate.device_selfcal(s["uvw"], s["freq"], s["vis"], s["wgt"], *s["cols"], NPIX, s["pix"], n_rounds=0,
                                    threshold=s["clean_threshold"], **MAJOR)


@pytest.fixture(scope="module")
def calibrated(scene):
    s = scene
    return calibrate.device_selfcal(s["uvw"], s["freq"], s["bad"], s["wgt"], *s["cols"], NPIX, s["pix"],
                                    n_rounds=ROUNDS, threshold=s["threshold"], **MAJOR)


def test_selfcal_recovers_the_flux_and_the_gains(scene, uncorrupted, calibrated):
    import torch

    out = calibrated
    want = uncorrupted["model"][40, 25].item()
    got = out["model"][40, 25].item()
    round0 = deconvolve.device_major_cycles(scene["uvw"], scene["freq"], scene["bad"], scene["wgt"], NPIX, scene["pix"],
                                            threshold=scene["threshold"], **MAJOR)
    first = round0["model"][40, 25].item()
    gains = out["gains"].cpu().numpy()
    err = np.abs(gains - cnp.rotate_to(scene["gains"])).max()
    print(f"flux at (40, 25): uncorrupted {want:.5f}, round 0 {first:.5f}, round {ROUNDS} {got:.5f}")
    print("round peaks", out["round_peaks"], "rms", out["round_rms"], f"worst gain error {err:.3g}")
    print("solver", out["solver"])
    assert abs(got - want) <= 0.01
    assert abs(first - want) > 0.05
    assert len(out["round_rms"]) == len(out["round_peaks"]) == ROUNDS + 1 and len(out["solver"]) == ROUNDS
    assert out["round_rms"][-1] <= 0.5 * out["round_rms"][0]
    assert out["round_rms"][0] == pytest.approx(float(torch.sqrt(torch.mean(round0["residual"] ** 2))), rel=1e-6)
    assert err <= 0.02
    assert tuple(gains.shape) == (N_INT, N_ANT) and out["ant_ok"].all() and gains.dtype == np.complex128
    assert np.abs(np.abs(gains) - 1.0).max() < 1e-12  # phase only
    assert all(info["n_converged"] == N_INT and info["n_dead"] == 0 for info in out["solver"])
    for key in ("model", "residual", "psf", "peaks", "components", "stop_reason"):
        assert key in out  # the last loop's dict


def test_no_round_is_the_major_cycle_loop(scene, uncorrupted):
    import torch

    s = scene
    ref = deconvolve.device_major_cycles(s["uvw"], s["freq"], s["vis"], s["wgt"], NPIX, s["pix"],
                                         threshold=s["clean_threshold"], **MAJOR)
    assert set(uncorrupted) == set(ref)
    assert uncorrupted["peaks"] == ref["peaks"] and uncorrupted["components"] == ref["components"]
    assert uncorrupted["stop_reason"] == ref["stop_reason"]
    for name in ("model", "residual", "psf"):
        assert torch.equal(uncorrupted[name], ref[name]), name


def test_driver_equals_the_written_out_loop(scene, calibrated):
    import torch

    s = scene
    d, cols, pix = [s["uvw"], s["freq"]], s["cols"], s["pix"]
    kw = dict(threshold=s["threshold"], **MAJOR)
    vis_c, wgt_c = s["bad"], s["wgt"]
    solver = []
    for _ in range(ROUNDS):
        res = deconvolve.device_major_cycles(*d, vis_c, wgt_c, NPIX, pix, **kw)
        model_col, _ = gridder.device_dirty2ms(*d, res["model"], None, pix, pix, do_wstacking=False,
                                               out_dtype=torch.complex64)
        gains, ok, info = calibrate.device_gaincal(s["bad"], model_col, s["wgt"], *cols, N_ANT, N_INT, niter=50,
                                                   tol=1e-8, refant=0, phase_only=True)
        solver.append(info)
        vis_c, wgt_c = calibrate.device_gain_apply(s["bad"], s["wgt"], *cols, gains, ok)
    res = deconvolve.device_major_cycles(*d, vis_c, wgt_c, NPIX, pix, **kw)
    out = calibrated
    print("driver", out["peaks"], out["components"], "loop", res["peaks"], res["components"])
    assert out["components"] == res["components"] and out["stop_reason"] == res["stop_reason"]
    gate = 1e-10 * s["first"]  # the parity gate of test_gpu_clean.py, relative to the dirty peak
    assert np.abs(np.array(out["peaks"]) - np.array(res["peaks"])).max() <= gate
    for name in ("model", "residual", "psf"):
        assert float((out[name] - res[name]).abs().max()) <= gate, name
    assert float((out["gains"] - gains).abs().max()) <= 1e-9 and torch.equal(out["ant_ok"], ok)
    for mine, theirs in zip(solver, out["solver"]):
        assert mine["n_converged"] == theirs["n_converged"] and mine["max_iter_done"] == theirs["max_iter_done"]
