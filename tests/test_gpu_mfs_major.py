"""
GPU tests of the wide-band major-cycle loop (`mfs.device_mfs_major_cycles`) and
of its pieces (`device_mfs_invert`, `device_mfs_residual`).

The scene is `major_scene` of test_gpu_clean.py (k = 45, seed 17, 64 x 64
pixels of 2e-5 rad, `umax` at the top channel, Gaussian-taper weights) with
four channels over 1.0 .. 1.3 GHz, the reference frequency 1.1 GHz off the
band's centre and three sources with linear spectra I0 + I1 x.

Checked on the CPU before relying on it (exact DFT inverts and a numpy minor
cycle in the manner of `_mfs_np`; threshold 1e-3 of the first dirty peak, gain
0.2): one term needs 2 cycles (203 and 1 components) and leaves 0.95460,
0.62685 and -0.28750 at the sources; two terms need 1 cycle of 100 components,
end by threshold and leave I0 = 0.99921, 0.59907, -0.29909 and I1 = -0.69944,
0.49919, 0.19941, with H = [[1, 0.04545], [0.04545, 0.012397]] (condition
number 97). The worst errors, 9.3e-4 (I0) and 8.2e-4 (I1), are set by the
threshold; the bound 3e-3 leaves a factor of about 3 for the epsilon = 1e-4
gridder.
"""

import numpy as np
import pytest

import dft_torch
from ska_sdp_cip_amd import deconvolve, gridder, mfs, restore
from test_gpu_clean import C, NPIX

pytestmark = pytest.mark.gpu

FREQ = np.linspace(1.0e9, 1.3e9, 4)
REF_FREQ = 1.1e9
SOURCES = (((40, 25), 1.0, -0.7), ((20, 44), 0.6, 0.5), ((50, 50), -0.3, 0.2))  # pixel, I0, I1
MAJOR = dict(n_major=6, niter=5000, gain=0.2)
TOL = 3e-3


def _t(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mfs_scene(k=45, seed=17):
    """`major_scene` with FREQ and sources whose flux is I0 + I1 x per channel."""
    rng = np.random.default_rng(seed)
    pix = 2.0e-5
    nchan = FREQ.size
    umax = 0.6 * 0.5 / pix * C / FREQ[-1]  # metres
    g = (np.arange(k) + 0.5) / k * 2.0 - 1.0
    uu, vv = np.meshgrid(g, g, indexing="ij")
    uv = np.stack([uu.ravel(), vv.ravel()], 1) + rng.uniform(-0.02, 0.02, size=(k * k, 2)) * (2.0 / k)
    uv = uv[rng.permutation(k * k)]
    uvw = np.zeros((k * k, 3))
    uvw[:, :2] = uv * umax
    wgt = np.repeat(np.exp(-0.5 * 9.0 * (uv ** 2).sum(1))[:, None], nchan, axis=1)
    vis = np.zeros((k * k, nchan), dtype=np.complex128)
    for (i, j), i0, i1 in SOURCES:
        l, m = (i - NPIX // 2) * pix, (j - NPIX // 2) * pix  # noqa: E741
        for c, f in enumerate(FREQ):
            flux = i0 + i1 * (f - REF_FREQ) / REF_FREQ
            vis[:, c] += flux * np.exp(-2j * np.pi * f / C * (uvw[:, 0] * l + uvw[:, 1] * m))
    return uvw, FREQ.copy(), vis, wgt, pix


@pytest.fixture(scope="module")
def scene():
    uvw, freq, vis, wgt, pix = mfs_scene()
    d = dict(uvw=_t(uvw), freq=_t(freq), vis=_t(vis), wgt=_t(wgt), pix=pix)
    dirty, _ = gridder.device_ms2dirty(d["uvw"], d["freq"], d["vis"], d["wgt"], NPIX, NPIX, pix, pix, normalise=True)
    d["first"] = float(dirty.abs().max())  # the first dirty peak of term 0
    d["threshold"] = 1e-3 * d["first"]
    return d


@pytest.fixture(scope="module")
def two_terms(scene):
    s = scene
    return mfs.device_mfs_major_cycles(s["uvw"], s["freq"], s["vis"], s["wgt"], NPIX, s["pix"], nterms=2,
                                       ref_freq=REF_FREQ, threshold=s["threshold"], do_wstacking=False, **MAJOR)


def test_two_terms_recover_flux_and_slope(scene, two_terms):
    out, threshold = two_terms, scene["threshold"]
    print("peaks", out["peaks"], "components", out["components"], out["stop_reason"])
    print("hessian", out["hessian"].tolist(), "cond", np.linalg.cond(out["hessian"]))
    assert out["stop_reason"] == "threshold"
    assert 1 <= len(out["peaks"]) <= 3 and all(n < MAJOR["niter"] for n in out["components"])
    hinv = out["hinv"]
    residuals = out["residuals"].cpu().numpy()
    principal = hinv[0, 0] * residuals[0] + hinv[0, 1] * residuals[1]
    print("final max |principal solution|", np.abs(principal).max(), "threshold", threshold)
    assert np.abs(principal).max() <= threshold
    models = out["models"].cpu().numpy()
    top = np.argsort(np.abs(models[0]).ravel())[-3:]
    assert {divmod(int(t), NPIX) for t in top} == {pos for pos, _, _ in SOURCES}
    for pos, i0, i1 in SOURCES:
        print(pos, "I0", models[0][pos], "I1", models[1][pos])
    for pos, i0, i1 in SOURCES:
        assert abs(models[0][pos] - i0) <= TOL, (pos, models[0][pos])
        assert abs(models[1][pos] - i1) <= TOL, (pos, models[1][pos])
    assert out["psfs"].shape == (3, NPIX, NPIX) and out["ref_freq"] == REF_FREQ
    assert out["psfs"][0, NPIX // 2, NPIX // 2].item() == pytest.approx(1.0, abs=1e-3)
    hessian = out["hessian"]
    assert hessian.shape == (2, 2) and np.array_equal(hessian, hessian.T)
    assert np.allclose(hinv @ hessian, np.eye(2), atol=1e-9)
    assert hessian[0, 1] == pytest.approx(0.04545, abs=2e-5) and hessian[1, 1] == pytest.approx(0.012397, abs=2e-5)


def test_one_image_leaves_the_spectral_error_the_feature_removes(scene):
    s = scene
    out = deconvolve.device_major_cycles(s["uvw"], s["freq"], s["vis"], s["wgt"], NPIX, s["pix"],
                                         threshold=s["threshold"], do_wstacking=False, **MAJOR)
    got = out["model"][40, 25].item()
    print("single image at (40, 25):", got, "components", out["components"])
    assert abs(got - 1.0) >= 0.03  # 0.9546 on the CPU


def test_driver_equals_the_written_out_loop(scene):
    import torch

    s = scene
    d = [s["uvw"], s["freq"]]
    threshold, first, pix = s["threshold"], s["first"], s["pix"]
    out = mfs.device_mfs_major_cycles(*d, s["vis"], s["wgt"], NPIX, pix, nterms=2, ref_freq=REF_FREQ,
                                      threshold=threshold, cycle_fraction=0.05, do_wstacking=False, **MAJOR)
    kw = dict(do_wstacking=False)
    res, psfs = mfs.device_mfs_invert(*d, s["vis"], s["wgt"], NPIX, pix, nterms=2, ref_freq=REF_FREQ, **kw)
    hessian, hinv = mfs.mfs_hessian(psfs)
    models = torch.zeros_like(res)
    peaks, comps = [], []
    for _ in range(MAJOR["n_major"]):
        peak = float((hinv[0, 0] * res[0] + hinv[0, 1] * res[1]).abs().max())
        if peak <= threshold:
            break
        peaks.append(peak)
        _, _, info = mfs.device_mfs_clean(res, psfs, hinv, gain=MAJOR["gain"], niter=MAJOR["niter"],
                                          threshold=max(threshold, 0.05 * peak), model=models, inplace=True)
        comps.append(info["niter_done"])
        vres = mfs.device_mfs_residual(*d, s["vis"], models, pix, REF_FREQ, **kw)
        res, _ = mfs.device_mfs_invert(*d, vres, s["wgt"], NPIX, pix, nterms=2, ref_freq=REF_FREQ, want_psfs=False,
                                       **kw)
    print("driver", out["peaks"], out["components"], "loop", peaks, comps)
    assert out["components"] == comps and len(out["peaks"]) == len(peaks) >= 2
    gate = 1e-10 * first  # the parity gate of test_gpu_clean.py, relative to the dirty peak
    assert np.abs(np.array(out["peaks"]) - np.array(peaks)).max() <= gate
    assert np.abs(out["hessian"] - hessian).max() <= gate
    for name, mine in (("models", models), ("residuals", res), ("psfs", psfs)):
        assert float((out[name] - mine).abs().max()) <= gate, name


def test_one_term_through_the_new_driver_is_the_narrow_band_loop(scene):
    s = scene
    args = (s["uvw"], s["freq"], s["vis"], s["wgt"], NPIX, s["pix"])
    kw = dict(threshold=s["threshold"], cycle_fraction=0.05, do_wstacking=False, **MAJOR)
    out = mfs.device_mfs_major_cycles(*args, nterms=1, ref_freq=REF_FREQ, **kw)
    old = deconvolve.device_major_cycles(*args, **kw)
    print("mfs", out["peaks"], out["components"], "hogbom", old["peaks"], old["components"])
    assert out["components"] == old["components"] and out["stop_reason"] == old["stop_reason"]
    assert out["models"].shape == (1, NPIX, NPIX) and out["psfs"].shape == (1, NPIX, NPIX)
    gate = 1e-10 * s["first"]
    assert np.abs(np.array(out["peaks"]) - np.array(old["peaks"])).max() <= gate
    for mine, name in ((out["models"][0], "model"), (out["residuals"][0], "residual"), (out["psfs"][0], "psf")):
        assert float((mine - old[name]).abs().max()) <= gate, name


def test_restore_and_spectral_index(scene):
    import torch

    s = scene
    alpha_cut = 0.05
    out = mfs.device_mfs_major_cycles(s["uvw"], s["freq"], s["vis"], s["wgt"], NPIX, s["pix"], nterms=2,
                                      ref_freq=REF_FREQ, threshold=s["threshold"], do_wstacking=False, restore=True,
                                      alpha_cut=alpha_cut, **MAJOR)
    restored, alpha = out["restored"], out["alpha"]
    assert tuple(restored.shape) == (2, NPIX, NPIX) and tuple(alpha.shape) == (NPIX, NPIX)
    assert out["beam"] == restore.device_fit_beam(out["psfs"][0])
    finite = torch.isfinite(alpha)
    assert torch.equal(finite, restored[0].abs() > alpha_cut) and 0 < int(finite.sum()) < NPIX * NPIX
    (i, j), i0, i1 = SOURCES[0][0], SOURCES[0][1], SOURCES[0][2]
    print("alpha at (40, 25):", alpha[i, j].item(), "restored", restored[0, i, j].item(), restored[1, i, j].item())
    assert alpha[i, j].item() * i0 == pytest.approx(i1, abs=1e-2)
    hinv = torch.from_numpy(out["hinv"]).cuda()
    solved = hinv[1, 0] * out["residuals"][0] + hinv[1, 1] * out["residuals"][1]
    want = restore.device_restore(out["models"][1], solved, out["beam"])
    assert float((restored[1] - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_invert_terms_against_the_direct_dft(scene):
    """Term 1 and PSF 2 against oracle/dft_torch.py's direct DFT at the sources,
    the centre, the corners and 24 seeded pixels.
    The bound is the one test_gpu_invert_parity.py asserts for its
    epsilon = 1e-4 case (error over the weight sum < 1e-5, well below epsilon):
    |x| <= 0.19 only shrinks the visibilities these two images are made of."""
    s = scene
    res, psfs = mfs.device_mfs_invert(s["uvw"], s["freq"], s["vis"], s["wgt"], NPIX, s["pix"], nterms=2,
                                      ref_freq=REF_FREQ, do_wstacking=False)
    x = (s["freq"] - REF_FREQ) / REF_FREQ
    pixels = dft_torch.check_pixels(NPIX, NPIX, n_random=24) + [pos for pos, _, _ in SOURCES]
    at = tuple(np.array(pixels).T)
    for name, got, vis in (("term 1", res[1], s["vis"] * x), ("psf 2", psfs[2], (x * x).expand_as(s["vis"]) + 0j)):
        sums, sumw = dft_torch.dft_pixels_dense(s["uvw"], s["freq"], vis.contiguous(), s["wgt"], pixels, NPIX, NPIX,
                                                s["pix"], s["pix"])
        err = np.abs(got.cpu().numpy()[at] - sums / sumw).max()
        print(name, "max |gridded - DFT| / sum w =", err)
        assert err < 1e-5, name
    # the Taylor factor went into the visibilities: every image is over the same weight sum
    assert psfs[0, NPIX // 2, NPIX // 2].item() == pytest.approx(1.0, abs=1e-3)
    assert psfs[2, NPIX // 2, NPIX // 2].item() == pytest.approx(float((s["wgt"] * x * x).sum() / s["wgt"].sum()),
                                                                  abs=1e-5)
