"""GPU: DynamicSpatialHashedCollisionMapGrid::InsertPointCloudRays from C++ (examples/dsh_rays.cpp) and from pysdf_tools, against the
restatement of a frame of sensor rays (tests/dsh_rays_restated.py): the example's frames replayed, its windows and SDFs compared byte
for byte."""
import os
import subprocess

import numpy as np
import pytest

import dsh_restated as R
import dsh_rays_restated as RR
from sdf_tools_amd import build

pytestmark = pytest.mark.gpu

# the numbers of examples/dsh_rays.cpp
CELL, CHUNK, SENSOR, MAX_RANGE = 0.05, (8, 8, 8), (0.025, 1.225, 1.225), 4.0
LOWER, SHAPE = (20, 12, 12), (48, 24, 24)
UNKNOWN, FREE, FILLED = R.record(0.5, 0), R.record(0.0, 0), R.record(1.0, 0)


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    d = tmp_path_factory.mktemp("dsh_rays")
    exe = build.build_example("dsh_rays")
    out = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "dsh_rays example done" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    frames = [np.fromfile(os.path.join(str(d), "frame_%d.f32" % k), np.float32).reshape(-1, 3) for k in range(2)]
    windows = [np.fromfile(os.path.join(str(d), "window_%d.cells" % k), np.uint64).reshape(SHAPE) for k in range(2)]
    sdfs = [np.fromfile(os.path.join(str(d), "window_%d_sdf.f32" % k), np.float32).reshape(SHAPE) for k in range(2)]
    return out.stdout, frames, windows, sdfs


def test_the_example_and_pysdf_tools_against_the_restatement(gpu, example):
    stdout, frames, windows, sdfs = example
    from sdf_tools_amd._bindings import load_pysdf_tools
    P = load_pysdf_tools()
    ref = R.Map(None, CELL, CHUNK, UNKNOWN)
    g = P.DynamicSpatialHashedCollisionMapGrid("world", CELL, 8, 8, 8, P.COLLISION_CELL(0.5))
    face = (30, 24, 24)                                                        # the cell of the example's query on the box's face
    for k, f in enumerate(frames):
        assert len(f) == 48 * 48 and np.isnan(f[:, 0]).sum() == 23
        st, want_counts = RR.insert_rays(ref, SENSOR, f, MAX_RANGE, FREE, FILLED)
        assert want_counts["rays_skipped"] == 23 and want_counts["rays_truncated"] == 0 and want_counts["rays_hit"] == len(f) - 23
        line = [l for l in stdout.splitlines() if l.startswith("frame %d" % k)][0]
        assert "%d hits, 0 beyond the range, 23 without a return, %d cells carved, %d new chunks" % (
            want_counts["rays_hit"], want_counts["cells_carved"], want_counts["new_chunks"]) in line, line
        counts = g.InsertPointCloudRays(f, SENSOR, MAX_RANGE, P.COLLISION_CELL(0.0), P.COLLISION_CELL(1.0))
        assert counts == want_counts and not g.AreComponentsValid()
        want = ref.window(LOWER, SHAPE)
        assert int(want[tuple(np.subtract(face, LOWER))]) == (FILLED if k == 0 else FREE)
        assert np.array_equal(windows[k], want), "the C++ class's window after frame %d" % k
        assert np.array_equal(g.ExtractWindowRecords(LOWER, *SHAPE), want), "the pysdf_tools window after frame %d" % k
        want_sdf, _ = gpu.build_cells(want.view(np.float32), SHAPE, 8, 0, False, CELL, False)
        assert np.array_equal(sdfs[k].view(np.uint32), want_sdf.view(np.uint32)), "the example's SDF after frame %d" % k
        at = tuple(np.subtract(face, LOWER))
        assert (want_sdf[at] < 0) == (k == 0), "the window's SDF shows the box in frame 0 and shows it gone in frame 1"
    assert {FREE, FILLED, UNKNOWN} == set(np.unique(windows[0]).tolist())
    # the refusals reach Python as ValueError (std::invalid_argument), and nothing is written
    before = g.GetCounts()
    for sensor, max_range in [((np.nan, 0.0, 0.0), 1.0), (SENSOR, 0.0), (SENSOR, 65536.5 * CELL)]:
        with pytest.raises(ValueError):
            g.InsertPointCloudRays(frames[0], sensor, max_range, P.COLLISION_CELL(0.0), P.COLLISION_CELL(1.0))
    assert g.GetCounts() == before
    assert g.InsertPointCloudRays(np.zeros((0, 3), np.float32), SENSOR, 1.0, P.COLLISION_CELL(0.0), P.COLLISION_CELL(1.0))["cells_carved"] == 0
    with pytest.raises(RuntimeError):
        P.DynamicSpatialHashedCollisionMapGrid().InsertPointCloudRays(frames[0], SENSOR, 1.0, P.COLLISION_CELL(0.0), P.COLLISION_CELL(1.0))
