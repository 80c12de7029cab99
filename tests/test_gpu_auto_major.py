"""
GPU tests of the noise-driven major cycles: `auto_threshold` and `auto_mask` on
`deconvolve.device_major_cycles`, `mfs.device_mfs_major_cycles` and
`multiscale.device_ms_major_cycles`.

The scene is `_auto_scene`: the tracks of `_ms_scene` at 256 x 256, its two
point sources (1.0 and 0.5) and seeded visibility noise of 0.02 flux units per
dirty pixel; test_noise_host.py asserts in numpy that the faint source stands at
10 sigma of the first residual or more and that sigma_c > 0 in every cycle. Each driver
is compared, bit for bit, with the same loop written out from
`device_image_noise`, `device_auto_mask`, the minor cycle and the re-invert.
"""

import numpy as np
import pytest

import _auto_scene as au
import _ms_scene as sc
from ska_sdp_cip_amd import _lib, deconvolve, gridder, mfs, multiscale, noise, predict
from ska_sdp_cip_amd.weighting import device_imaging_weights

pytestmark = pytest.mark.gpu

NPIX = au.NPIX
KW = dict(do_wstacking=False)
SEED_S, GROW_S = au.AUTO["auto_mask"]
KINDS = ("hogbom", "mfs", "ms")
PARENT_KEYS = {
    "hogbom": {"model", "residual", "psf"},
    "mfs": {"models", "residuals", "psfs", "hessian", "hinv", "ref_freq"},
    "ms": {"model", "models", "residual", "psf", "cross_psfs", "select_weight", "flux_scale", "widths"},
}
LOOP_KEYS = {"peaks", "components", "stop_reason"}


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def scene():
    import torch

    uvw, freq, pix = sc.tracks()
    vis = au.noisy_visibilities(uvw, freq, pix)
    return dict(uvw=_t(uvw), freq=_t(freq), vis=_t(vis), pix=pix,
                wgt=torch.ones(vis.shape, dtype=torch.float64, device="cuda"))


def _driver(kind, s, vis=None, **extra):
    args = (s["uvw"], s["freq"], s["vis"] if vis is None else vis, s["wgt"], NPIX, s["pix"])
    if kind == "hogbom":
        return deconvolve.device_major_cycles(*args, **au.MAJOR, **extra)
    if kind == "mfs":
        return mfs.device_mfs_major_cycles(*args, nterms=2, **au.MAJOR, **extra)
    return multiscale.device_ms_major_cycles(*args, widths=sc.WIDTHS, **au.MAJOR, **extra)


@pytest.fixture(scope="module")
def auto_runs(scene):
    return {kind: _driver(kind, scene, **au.AUTO) for kind in KINDS}


class _Loop:
    """One driver's pieces, as the driver itself calls them: `image()` is what
    the noise is measured on, `clean(threshold, niter, mask)` the minor cycle
    (niter 0: the probe), `reinvert()` the predict and the invert."""

    def __init__(self, kind, s):
        import torch

        uvw, freq, vis, pix = s["uvw"], s["freq"], s["vis"], s["pix"]
        wgt, _ = device_imaging_weights(uvw, freq, s["wgt"], NPIX, NPIX, pix, pix, weighting="natural", robust=0.0)
        gain = au.MAJOR["gain"]
        self.kind = kind
        if kind == "mfs":
            ref = mfs._mid_band(freq)
            scratch = torch.empty_like(vis)
            residuals, psfs = mfs.device_mfs_invert(uvw, freq, vis, wgt, NPIX, pix, nterms=2, ref_freq=ref,
                                                    scratch=scratch, **KW)
            _, hinv = mfs.mfs_hessian(psfs)
            models = torch.zeros_like(residuals)
            self.image = lambda: residuals[0]
            self.clean = lambda thr, n, mask: mfs.device_mfs_clean(
                residuals, psfs, hinv, gain=gain, threshold=thr, niter=n, mask=mask, model=models if n else None,
                inplace=True)[2]

            def reinvert():
                vres = mfs.device_mfs_residual(uvw, freq, vis, models, pix, ref, reuse_plan=True, scratch=scratch,
                                               **KW)
                mfs.device_mfs_invert(uvw, freq, vres, wgt, NPIX, pix, nterms=2, ref_freq=ref, want_psfs=False,
                                      reuse_plan=True, out=residuals, scratch=scratch, **KW)

            self.reinvert = reinvert
            self.outputs = {"models": models, "residuals": residuals, "psfs": psfs}
            return
        psf, _ = gridder.device_ms2dirty(uvw, freq, None, wgt, NPIX, NPIX, pix, pix, psf=True, normalise=True, **KW)
        residual, _ = gridder.device_ms2dirty(uvw, freq, vis, wgt, NPIX, NPIX, pix, pix, normalise=True,
                                              reuse_plan=True, **KW)
        model = torch.zeros((NPIX, NPIX), dtype=torch.float64, device="cuda")
        self.image = lambda: residual
        self.outputs = {"model": model, "residual": residual, "psf": psf}
        if kind == "hogbom":
            self.clean = lambda thr, n, mask: deconvolve.device_hogbom_clean(
                residual, psf, gain=gain, threshold=thr, niter=n, mask=mask, model=model if n else None,
                inplace=True)[2]
            self.before_reinvert = lambda: None
        else:
            widths = [float(w) for w in sc.WIDTHS]
            cross = multiscale.device_cross_psfs(psf, widths)
            select_weight, flux_scale = multiscale.scale_weights(cross, widths)
            models = torch.zeros((len(widths), NPIX, NPIX), dtype=torch.float64, device="cuda")
            stack = torch.empty_like(models)
            self.outputs["models"] = models

            def clean(thr, n, mask):
                if n == 0:  # the probe opens a cycle: smooth the new residual
                    multiscale.device_scale_residuals(residual, widths, out=stack)
                return multiscale.device_ms_clean(stack, cross, select_weight, flux_scale, gain=gain, threshold=thr,
                                                  niter=n, mask=mask, model=models if n else None, inplace=True)[2]

            self.clean = clean
            self.before_reinvert = lambda: multiscale.device_ms_model(models, widths, out=model)

        def reinvert():
            self.before_reinvert()
            vres = predict.device_residual(uvw, freq, vis, model, pix, None, reuse_plan=True, **KW)
            gridder.device_ms2dirty(uvw, freq, vres, wgt, NPIX, NPIX, pix, pix, normalise=True, reuse_plan=True,
                                    out=residual, **KW)

        self.reinvert = reinvert

    def run(self, auto_threshold, seed_s, grow_s, mask=None, threshold=0.0, cycle_fraction=0.0):
        """The loop of section "Major cycles", written out."""
        import torch

        grown = torch.zeros((NPIX, NPIX), dtype=torch.uint8, device="cuda")
        peaks, comps, sigmas, stop = [], [], [], "n_major"
        for _ in range(au.MAJOR["n_major"]):
            image = self.image()
            sigma = noise.device_image_noise(image)["sigma"]
            sigmas.append(sigma)
            if not (np.isfinite(sigma) and sigma > 0.0):
                stop = "noise"
                break
            noise.device_auto_mask(image, seed_s * sigma, grow_s * sigma, region=mask, base=grown, out=grown)
            floor = max(threshold, auto_threshold * sigma)
            probe = self.clean(floor, 0, grown)
            if probe["stop_reason"] == _lib.CIP_CLEAN_EMPTY:
                stop = "empty"
                break
            peak = abs(probe["peak"])
            if peak <= floor:
                stop = "threshold"
                break
            peaks.append(peak)
            comps.append(self.clean(max(floor, cycle_fraction * peak), au.MAJOR["niter"], grown)["niter_done"])
            self.reinvert()
        return dict(self.outputs, peaks=peaks, components=comps, noise=sigmas, auto_mask=grown, stop_reason=stop)


@pytest.mark.parametrize("kind", KINDS)
def test_driver_equals_the_written_out_loop(kind, scene, auto_runs):
    import torch

    out = auto_runs[kind]
    mine = _Loop(kind, scene).run(au.AUTO["auto_threshold"], SEED_S, GROW_S)
    print(kind, "driver", out["peaks"], out["components"], out["noise"], out["stop_reason"])
    print(kind, "loop  ", mine["peaks"], mine["components"], mine["noise"], mine["stop_reason"])
    assert set(out) == PARENT_KEYS[kind] | LOOP_KEYS | {"noise", "auto_mask"}
    for key in ("peaks", "components", "noise", "stop_reason"):
        assert out[key] == mine[key], key
    for key, value in mine.items():
        if torch.is_tensor(value):
            assert torch.equal(out[key], value), key
    assert len(out["noise"]) == len(out["peaks"]) + (out["stop_reason"] != "n_major") >= 2
    assert all(np.isfinite(s) and s > 0.0 for s in out["noise"])
    assert out["noise"][-1] < out["noise"][0]  # the sources' sidelobes have left the residual


@pytest.mark.parametrize("kind", KINDS)
def test_components_lie_inside_the_mask_and_both_sources_are_masked(kind, auto_runs):
    out = auto_runs[kind]
    grown = out["auto_mask"]
    assert grown.dtype.is_floating_point is False and tuple(grown.shape) == (NPIX, NPIX)
    models = out["models"] if kind in ("mfs", "ms") else out["model"][None]
    placed = (models != 0.0).any(dim=0)
    assert int(placed.sum()) > 0 and bool((grown[placed] == 1).all())
    assert set(np.unique(grown.cpu().numpy())) == {0, 1} and int(grown.sum()) < NPIX * NPIX // 20
    for pos, flux in au.POINTS:
        print(kind, pos, flux, "masked", int(grown[pos]), "model", float(models[:, pos[0], pos[1]].abs().sum()))
        assert int(grown[pos]) == 1


@pytest.mark.parametrize("kind", KINDS)
def test_user_mask_keeps_a_source_out_of_the_auto_mask(kind, scene):
    import torch

    (keep, _), (drop, _) = au.POINTS
    user = torch.ones((NPIX, NPIX), dtype=torch.uint8, device="cuda")
    user[drop[0] - 10:drop[0] + 11, drop[1] - 10:drop[1] + 11] = 0
    out = _driver(kind, scene, mask=user, **au.AUTO)
    grown = out["auto_mask"]
    assert int(grown[drop]) == 0 and int(grown[keep]) == 1
    assert bool((grown[user == 0] == 0).all())  # the auto mask never leaves the user's
    models = out["models"] if kind in ("mfs", "ms") else out["model"][None]
    assert float(models[:, drop[0] - 10:drop[0] + 11, drop[1] - 10:drop[1] + 11].abs().sum()) == 0.0
    mine = _Loop(kind, scene).run(au.AUTO["auto_threshold"], SEED_S, GROW_S, mask=user)
    assert torch.equal(grown, mine["auto_mask"]) and out["peaks"] == mine["peaks"]


@pytest.mark.parametrize("kind", KINDS)
def test_zero_visibilities_stop_on_the_noise(kind, scene):
    import torch

    out = _driver(kind, scene, vis=torch.zeros_like(scene["vis"]), **au.AUTO)
    assert out["stop_reason"] == "noise" and out["noise"] == [0.0]
    assert out["peaks"] == [] and out["components"] == [] and int(out["auto_mask"].sum()) == 0
    only_threshold = _driver(kind, scene, vis=torch.zeros_like(scene["vis"]), auto_threshold=3.0)
    assert only_threshold["stop_reason"] == "noise" and "auto_mask" not in only_threshold


def test_options_alone_and_their_checks(scene):
    only_mask = _driver("hogbom", scene, auto_mask=4.0)  # one number: seed and grow
    assert only_mask["noise"] and "auto_mask" in only_mask and only_mask["stop_reason"] == "n_major"
    mine = _Loop("hogbom", scene).run(0.0, 4.0, 4.0)
    assert only_mask["peaks"] == mine["peaks"] and only_mask["components"] == mine["components"]
    only_threshold = _driver("hogbom", scene, auto_threshold=3.0)
    assert "auto_mask" not in only_threshold and len(only_threshold["noise"]) >= 2
    for bad in (dict(auto_mask=(3.0, 5.0)), dict(auto_mask=(5.0, 0.0)), dict(auto_mask=(5.0, 3.0, 1.0)),
                dict(auto_mask=float("nan")), dict(auto_threshold=-1.0), dict(auto_threshold=float("nan"))):
        with pytest.raises(ValueError, match="auto_"):
            _driver("hogbom", scene, **bad)


def _parent_major_cycles(result, n_major, threshold, cycle_fraction, clean, reinvert, restore):
    """The cycle loop as it stood before the two options, statement for statement."""
    peaks, components = [], []
    stop_reason = "n_major"
    for _cycle in range(int(n_major)):
        start = clean(threshold, True)
        if start["stop_reason"] == _lib.CIP_CLEAN_EMPTY:
            stop_reason = "empty"
            break
        peak = abs(start["peak"])
        if peak <= threshold:
            stop_reason = "threshold"
            break
        peaks.append(peak)
        components.append(clean(max(threshold, cycle_fraction * peak), False)["niter_done"])
        reinvert()
    result.update(peaks=peaks, components=components, stop_reason=stop_reason)
    if restore is not None:
        restore(result)
    return result


@pytest.mark.parametrize("kind", KINDS)
def test_options_off_is_the_parent_loop(kind, scene, monkeypatch):
    import torch

    extra = dict(threshold=0.05, cycle_fraction=0.2)
    out = _driver(kind, scene, **extra)
    assert set(out) == PARENT_KEYS[kind] | LOOP_KEYS and "noise" not in out and "auto_mask" not in out

    def parent(result, n_major, threshold, cycle_fraction, clean, reinvert, restore, *, mask=None, **_unused):
        return _parent_major_cycles(result, n_major, threshold, cycle_fraction, lambda t, probe: clean(t, probe, mask),
                                    reinvert, restore)

    module = {"hogbom": deconvolve, "mfs": mfs, "ms": multiscale}[kind]
    monkeypatch.setattr(module, "_major_cycles", parent)
    old = _driver(kind, scene, **extra)
    print(kind, out["peaks"], out["components"], out["stop_reason"])
    assert set(out) == set(old) and len(out["peaks"]) >= 1
    for key, value in old.items():
        if torch.is_tensor(value):
            assert torch.equal(out[key], value), key
        elif isinstance(value, np.ndarray):
            assert np.array_equal(out[key], value), key
        else:
            assert out[key] == value, key
