"""GPU: a short differential fuzz of the batched small-grid build (tools/fuzz_batch.py): random shapes around the changes of P,
batch sizes, mixed scenes, resolutions, borders and entry points on one red-zoned handle, every voxel of every grid as uint32
against oracle.exact_sdf and against its single build.  The tool's fixed prelude runs whatever the time budget is, so the summary
must report every P from 1 to 8, both paths and every entry point: conditions, not measurements."""
import ast
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [1, 2])
def test_short_batch_fuzz(seed):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_batch.py"), "8", str(seed)], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "fuzz OK" in r.stdout
    m = re.search(r"fuzz OK: (\d+) batches, (\d+) grids .*red zones on; entry points (\{.*?\}); P (\{.*?\}); paths (\{.*?\})", r.stdout)
    assert m, r.stdout[-2000:]
    entries, planes, paths = (ast.literal_eval(m.group(k)) for k in (3, 4, 5))
    assert all(planes.get(p, 0) >= 1 for p in range(1, 9)), planes
    assert set(planes) <= set(range(1, 9)), planes
    assert paths["fast"] >= 8 and paths["slow"] >= 1, paths
    assert sorted(entries) == ["device", "gradient", "host", "tagged"] and all(v >= 1 for v in entries.values()), entries
    assert int(m.group(1)) >= 9 and int(m.group(2)) >= int(m.group(1))
