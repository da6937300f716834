"""GPU: a short differential fuzz of the mesh rasteriser and the plane (tools/fuzz_mesh.py): random meshes, poses, grids and origins
on one red-zoned handle, host and device form, with and without accumulation, every bit, byte and id against the restatement
(tests/mesh_raster_restated.py)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_short_mesh_fuzz():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_mesh.py"), "4", "1"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    print(last)
    m = re.match(r"fuzz OK: (\d+) scenes .* 0 mismatches; (\d+) accumulated, (\d+) with a plane; (\d+) triangles, (\d+) filled cells;", last)
    assert m, last
    assert int(m.group(1)) >= 50 and int(m.group(2)) >= 10 and int(m.group(3)) >= 5 and int(m.group(4)) >= 500 and int(m.group(5)) >= 1000, last
