"""
The planner's serial-chain kernels must be resident beside two blocks of the headline scatter: no
LDS, no scratch, and (waves of a block per SIMD) x (allocated VGPRs) within what the scatter leaves free.

Compiles cip_plan.hip, cip_grid.hip and the W = 8 scatter for gfx950 (device only, to assembly: the Makefile's
`asm` target, into a temporary directory; no GPU needed) and runs tools/kernel_residency.py on the result,
which reads the kernels' register and LDS counts from their metadata.
"""

import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ska-sdp-continuum-imaging-pipeline_amd" / "csrc"


def test_serial_chain_kernels_fit_beside_the_scatter(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.fail("hipcc not found: the residency table needs a device compile")
    asm = tmp_path / "asm"
    subprocess.run(["make", "-C", str(CSRC), "-j3", "asm", f"ASM_DIR={asm}", f"HIPCC={hipcc}"], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    res = subprocess.run([sys.executable, str(ROOT / "tools" / "kernel_residency.py"), str(asm), "--check"],
                         capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "| serial |" in res.stdout and "| no |" not in "\n".join(
        line for line in res.stdout.splitlines() if "| serial |" in line)
