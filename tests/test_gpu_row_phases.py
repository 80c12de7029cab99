"""
Row phases of the bank-class order (csrc/cip_grid.hip order_kernel<0, true>,
cip_scatter.h rotate_rows / row_ptr - the default for dense rows): a
visibility of phase 1 adds its footprint rows in the order 1 .. W - 1, 0, so
it occupies the bank pairs of class c + P mod 32, and the order pass moves
each window's excess items of a class to that neighbour. Only the order of the
taps changes: the fixed-point integer sums are the same, and the images equal
those without phases (CIP_ROW_PHASES=0 in a child process, read once per
process) up to the order of the flush's global adds.

Cases (the flush-store and dense-row place tests' builders): cip_ms2dirty in
2-D on the fp64 class (complex64 / complex128 input, 64 / 192 / 256
channels), the reference's w-stacking call (packed class, plane groups), the
PSF, repeated calls, the uv-strip path over ragged row slices (their 64-bit
entries carry the phase in bit 63; like every case here it compares phases on
against phases off) and the chunked accumulating gridder. Weight sums
and the run / work-unit counts must be equal bit for bit.
"""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _all():
    import test_gpu_flush_store as fs
    import test_gpu_place_rows64 as pr

    out = {f"fs_{k}": v for k, v in fs._images().items()}
    out.update({f"pr_{k}": v for k, v in pr._cases().items()})
    return out


CHILD = """
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {orc!r}, {tests!r}]
import numpy as np
import test_gpu_row_phases as t
np.savez({out!r}, **t._all())
"""


def test_row_phases_equal_plain_order(gpu_device, tmp_path):
    mine = _all()
    out = tmp_path / "plain.npz"
    code = CHILD.format(root=str(ROOT), pkg=str(ROOT / "ska-sdp-continuum-imaging-pipeline_amd"),
                        orc=str(ROOT / "oracle"), tests=str(ROOT / "tests"), out=str(out))
    env = dict(os.environ, CIP_ROW_PHASES="0")
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=300)
    ref = np.load(out)
    assert sorted(ref.files) == sorted(mine)
    for k in mine:
        if k.startswith(("pr_sw_", "pr_cnt_", "pr_errs")):
            assert np.array_equal(mine[k], ref[k]), (k, mine[k], ref[k])
        elif k.startswith("pr_img_"):
            scale = float(mine["pr_scale_" + k[7:]][0])
            err = float(np.abs(mine[k] - ref[k]).max()) / scale
            assert err <= (1e-6 if k.startswith("pr_img_refcall") else 1e-13), (k, err)
        elif k.startswith("fs_"):
            peak = float(np.abs(ref[k]).max())
            assert peak > 0, k
            tol = 1e-6 if "refcall" in k else 1e-12
            assert float(np.abs(mine[k] - ref[k]).max()) <= tol * peak, k
