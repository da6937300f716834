"""GPU: a short differential fuzz of Resample (tools/fuzz_resample.py): random shapes, ratios, origins and record sizes on one
red-zoned handle, host and device form, every byte against the restatement (tests/resample_restated.cpp)."""
import ast
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_short_resample_fuzz():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_resample.py"), "5", "1"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    print(last)
    m = re.match(r"fuzz OK: (\d+) scenes .* 0 mismatches; host (\d+), device (\d+); record sizes (\{.*?\});", last)
    assert m, last
    assert int(m.group(1)) >= 50, last
    assert int(m.group(2)) == int(m.group(1)) == int(m.group(3)), last
    assert all(v >= 1 for v in ast.literal_eval(m.group(4)).values()), last
