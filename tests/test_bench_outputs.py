"""
bench.py's plain run and `--dump-outputs`: a plain run times exactly `--steps`
steps and prints the headline alone (what `--full` adds is absent), and the
dump holds what the timed path returned in its last step - the image of the
same seeded inputs inverted in this process - as float64 .npy files. Images
above `DUMP_MAX_PIXELS` are dumped as a fixed seeded sample (CPU test).
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import bench

ROOT = Path(__file__).resolve().parents[1]


def test_dump_outputs_whole_image_and_fixed_sample(tmp_path):
    small = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    bench.dump_outputs(tmp_path / "s", small, torch.tensor([2.5], dtype=torch.float64))
    got = np.load(tmp_path / "s" / "dirty.npy")
    assert got.dtype == np.float64 and got.shape == (3, 4) and np.array_equal(got, small.numpy())
    assert np.array_equal(np.load(tmp_path / "s" / "sum_weights.npy"), [2.5])
    # one pixel row more than the limit: a sample of DUMP_MAX_PIXELS values, the same at every call
    n = bench.DUMP_MAX_PIXELS // 2048 + 1
    big = torch.arange(n * 2048, dtype=torch.float64).reshape(n, 2048)  # value = flat index
    bench.dump_outputs(tmp_path / "a", big)
    bench.dump_outputs(tmp_path / "b", big)
    a, b = np.load(tmp_path / "a" / "dirty.npy"), np.load(tmp_path / "b" / "dirty.npy")
    assert a.dtype == np.float64 and a.shape == (bench.DUMP_MAX_PIXELS,) and np.array_equal(a, b)
    assert not (tmp_path / "a" / "sum_weights.npy").exists()
    assert a.min() >= 0 and a.max() < n * 2048 and np.all(np.diff(a) >= 0)
    assert np.unique(a).size > 0.5 * a.size  # spread over the image, not one corner
    assert a.nbytes <= 64 * 1000 * 1000


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_image(gpu_device, tmp_path):
    dump = tmp_path / "dump"
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--config", "c1", "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    cfg = bench.CONFIGS["c1"]
    nvis, npix = cfg["rows"] * cfg["nchan"], cfg["npix"]
    assert (res["steps"], res["warmup"], res["n_gpus"]) == (3, 1, 1)
    assert res["unit"] == "Mvis/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["metric"].startswith("Mvis/s gridded (invert)") and "support=8" in res["metric"]
    # value and ms_per_step are the same measurement (both rounded in the line)
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(nvis / res["ms_per_step"] / 1e3, rel=2e-2)
    for key in ("value_sync", "phases_ms", "max_err", "secondary", "parity_reduced"):
        assert key not in res, key
    assert res["roofline"] is None and res["cpu_baseline"] is None
    dirty, sumw = np.load(dump / "dirty.npy"), np.load(dump / "sum_weights.npy")
    assert dirty.dtype == np.float64 and dirty.shape == (npix, npix) and sumw.shape == (1,)
    # the same seeded inputs through the same call here: the same kernels on
    # the same data (fixed-point accumulation), so equal to rounding
    from ska_sdp_cip_amd import gridder

    uvw, freq, vis, wgt, px, _, _ = bench.make_inputs(cfg, 0, 1, gpu_device)
    ref, _ = gridder.device_ms2dirty(uvw, freq, vis, wgt, npix, npix, px, px, support=8, normalise=True)
    ref = ref.cpu().numpy()
    assert sumw[0] == pytest.approx(float(wgt.double().sum()), rel=1e-12)
    assert np.isfinite(dirty).all() and np.abs(ref).max() > 0
    assert np.abs(dirty - ref).max() <= 1e-12 * np.abs(ref).max()
