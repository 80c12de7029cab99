"""
The radix sort's digit histogram (`radix_hist_kernel`, cip_plan.hip: one wave, the counts in registers) at the
pass and run counts where its shape changes.

Path: `device_ms2dirty` (a fresh plan per call, `reuse_plan=False`) against the fp64 oracle at the tolerance
of test_gpu_invert_parity.py for the same call. A wrong histogram misplaces runs in the sorted order, which
changes the image grossly, so image parity detects it. One channel per row and every visibility on the
(periodic) grid: the planner sorts exactly nrow runs.

Pass counts: the sort takes one 8-bit pass per byte of the tile key - 16 tiles (1 pass: the histogram comes
from the place pass alone), 1024 tiles (2) and 1024 uv tiles x >= 65 w layers (3; asserted from the returned
parameters). Run counts at 2 passes: 1, 4095, 4096, 4097 (a 4096-run sub-block, one more and one less) and
8 * 4096 + 1 (one run past pass 0's group of 8 place blocks; the later passes' group is 1 sub-block).
"""

import numpy as np
import pytest

import oracle
from ska_sdp_cip_amd import gridder, synthetic as syn
from ska_sdp_cip_amd.invert import StokesIGridderInput

pytestmark = pytest.mark.gpu

TIGHT = 1e-10  # test_gpu_invert_parity.py: max |GPU - oracle| / sum(w) of a device_ms2dirty call
TILE = 32  # cells per edge of the work tile of grids below 2048^2


def _case(n_rows, w_scale=1.0):
    ms = syn.make_measurement_set(n_rows, 1, n_ant=16, array_radius_m=2000.0, fov_l=0.05, seed=3,
                                  weight_spectrum=True)
    gi = StokesIGridderInput.from_measurement_set_reader(ms)
    uvw = gi.uvw.copy()
    uvw[:, 2] *= w_scale
    # (flagged samples have weight 0: keep every weight positive, one row alone must still have a weight sum)
    w = (np.abs(gi.effective_weights()) + 0.5).astype(np.float32)
    return uvw, gi.channel_frequencies, gi.visibilities, w


def _check(n_rows, npix, wstack=False, w_scale=1.0, fill=0.9):
    import torch

    uvw, f, vis, w = _case(n_rows, w_scale)
    px = syn.pixel_size_for_grid(uvw, f, npix, fill=fill)
    args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (uvw, f, vis, w)]
    gpu, prm = gridder.device_ms2dirty(*args, npix, npix, px, px, support=8, do_wstacking=wstack, reuse_plan=False)
    ref = oracle.ms2dirty(uvw, f, vis, w, npix, npix, px, px, support=8, do_wstacking=wstack)
    err = float(np.abs(gpu.cpu().numpy() - ref).max() / w.astype(np.float64).sum())
    ntiles = -(-prm.nu // TILE) * -(-prm.nv // TILE) * ((prm.nplanes - prm.support + 1) if wstack else 1)
    print(f"rows {n_rows} npix {npix} planes {prm.nplanes} tile keys {ntiles} err {err:.3e}")
    assert err < TIGHT, err
    return ntiles


@pytest.mark.parametrize("n_rows", [1, 4095, 4096, 4097, 8 * 4096 + 1])
def test_two_passes_run_counts(gpu_device, n_rows):
    ntiles = _check(n_rows, 512)
    assert 256 < ntiles <= 65536


def test_one_pass(gpu_device):
    assert _check(4097, 64) <= 256


def test_three_passes(gpu_device):
    # w scaled up: >= 65 w layers over the 1024 uv tiles of a 1024^2 grid
    assert _check(4097, 512, wstack=True, w_scale=1150.0, fill=0.5) > 65536
