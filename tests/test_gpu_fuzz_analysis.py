"""GPU: a short differential fuzz of the analysis and per-point kernels (tools/fuzz_analysis.py): random shapes around the tile
plans, random scenes and operations, every output bit for bit against the restatements in tests/.  Every operation must have run."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["components", "topology", "extrema", "segments", "projection", "query_gradients", "query_points", "gradient"]


@pytest.mark.parametrize("seed", [1, 2])
def test_short_analysis_fuzz(seed):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_analysis.py"), "20", str(seed)], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("fuzz OK"), last
    counts = {k: int(v) for k, v in re.findall(r"'(\w+)': (\d+)", last)}
    assert sorted(counts) == sorted(OPS), last
    assert min(counts.values()) >= 3, last                  # an operation that is silently skipped fails here
