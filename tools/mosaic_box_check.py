"""
Is the box cip_mosaic_add launches on ever too tight? Random geometries (and
any given on the command line as files of cases) go through
tools/mosaic_box_check.cpp, a host program around the library's own
`mosaic_args` (build it as its header says), and each box is compared with the
pixels the numpy statement (tests/_mosaic_np.py) gives weight to. No GPU.

  python tools/mosaic_box_check.py path/to/mosaic_box_check [n_random]

Prints one JSON line; exits 1 if a box misses a covered pixel.
"""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "ska-sdp-continuum-imaging-pipeline_amd"), str(ROOT / "oracle")]

import _mosaic_np as mnp  # noqa: E402


def random_cases(n, seed=5):
    """Planes up to 200 pixels and 1.3 rad, facets up to 0.97 from the centre, pixel ratios 0.3 .. 3."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        nx, ny = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        px = rng.uniform(0.01, 1.3) / max(nx, ny)
        py = px * rng.uniform(0.7, 1.4)
        if (nx / 2 * px) ** 2 + (ny / 2 * py) ** 2 >= 0.98:
            continue
        half, trim = int(rng.integers(2, 9)), int(rng.integers(0, 4))
        fnx, fny = (int(rng.integers(2 * (half + trim), 120)) for _ in range(2))
        r, ph = rng.uniform(0, 0.97), rng.uniform(0, 2 * np.pi)
        out.append((nx, ny, px, py, fnx, fny, px * rng.uniform(0.3, 3), py * rng.uniform(0.3, 3), half, trim,
                    r * np.cos(ph), r * np.sin(ph)))
    return out


def main():
    exe, n = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 3000
    cases = random_cases(n)
    with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
        f.write("\n".join(" ".join(repr(float(v)) if isinstance(v, float) else str(v) for v in c) for c in cases) + "\n")
        f.flush()
        run = subprocess.run([exe, f.name], capture_output=True, text=True, check=True)
    lines = run.stdout.strip().split("\n")
    assert len(lines) == len(cases) and not run.stderr, run.stderr
    tight, missed, covered, box_area, true_area = [], 0, 0, 0, 0
    for c, line in zip(cases, lines):
        g = mnp.Geom(*c[:8], c[8], 1.0, c[9], 0.0)
        x, y, q2, _ = mnp.coords(g, c[10], c[11])
        ii, jj = np.nonzero(mnp.weight(g, x, y, q2) > 0)
        if line == "none" or line.startswith("err"):
            missed += 1
            if ii.size or line.startswith("err"):
                tight.append((c, line))
            continue
        i0, i1, j0, j1 = map(int, line.split())
        if ii.size:
            covered += 1
            if ii.min() < i0 or ii.max() > i1 or jj.min() < j0 or jj.max() > j1:
                tight.append((c, line))
            true_area += (ii.max() - ii.min() + 1) * (jj.max() - jj.min() + 1)
            box_area += (i1 - i0 + 1) * (j1 - j0 + 1)
    print(json.dumps({"cases": len(cases), "facets_that_miss": missed, "facets_that_cover": covered,
                      "too_tight": len(tight), "box_area_over_covered_box_area": round(box_area / max(true_area, 1), 3)}))
    for t in tight[:10]:
        print("too tight:", t, file=sys.stderr)
    return 1 if tight else 0


if __name__ == "__main__":
    sys.exit(main())
