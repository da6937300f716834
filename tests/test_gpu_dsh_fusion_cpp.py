"""GPU: DynamicSpatialHashedCollisionMapGrid::FusePointCloudRays from C++ (examples/dsh_fusion.cpp) and from pysdf_tools, against the
restatement of a fused frame of sensor rays (tests/dsh_fusion_restated.py): the example's frames replayed, its windows and SDFs compared
byte for byte, the frame at which it says the box's face fades, and the refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

import dsh_restated as R
import dsh_fusion_restated as F
from sdf_tools_amd import build

pytestmark = pytest.mark.gpu

# the numbers of examples/dsh_fusion.cpp
CELL, CHUNK, SENSOR, MAX_RANGE = 0.05, (8, 8, 8), (0.025, 1.225, 1.225), 4.0
LOWER, SHAPE = (20, 12, 12), (48, 24, 24)
FRAMES, BOX_FRAMES, SPURIOUS_FRAME, PIXELS = 14, 4, 3, 32
FACE, SPURIOUS = (30, 24, 24), (24, 24, 24)                                   # the cells of the example's two watched locations
UNKNOWN = R.record(0.5, 0)


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    d = tmp_path_factory.mktemp("dsh_fusion")
    exe = build.build_example("dsh_fusion")
    out = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "dsh_fusion example done" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    frames = [np.fromfile(os.path.join(str(d), "frame_%d.f32" % k), np.float32).reshape(-1, 3) for k in range(FRAMES)]
    windows = [np.fromfile(os.path.join(str(d), "window_%d.cells" % k), np.uint64).reshape(SHAPE) for k in range(FRAMES)]
    sdfs = [np.fromfile(os.path.join(str(d), "window_%d_sdf.f32" % k), np.float32).reshape(SHAPE) for k in range(FRAMES)]
    return out.stdout, frames, windows, sdfs


def test_the_example_and_pysdf_tools_against_the_restatement(gpu, example):
    stdout, frames, windows, sdfs = example
    from sdf_tools_amd._bindings import load_pysdf_tools
    P = load_pysdf_tools()
    ref = R.Map(None, CELL, CHUNK, UNKNOWN)
    g = P.DynamicSpatialHashedCollisionMapGrid("world", CELL, 8, 8, 8, P.COLLISION_CELL(0.5))
    face, stray = tuple(np.subtract(FACE, LOWER)), tuple(np.subtract(SPURIOUS, LOWER))
    faded, stray_most = None, 0.0
    for k, f in enumerate(frames):
        assert len(f) == PIXELS * PIXELS + (k == SPURIOUS_FRAME) and np.isnan(f[:, 0]).sum() == 10
        st, want_counts = F.fuse_rays(ref, SENSOR, f, MAX_RANGE)
        assert want_counts["rays_skipped"] == 10 and want_counts["rays_truncated"] == 0
        line = [l for l in stdout.splitlines() if l.startswith("frame %d " % k)][0]
        assert "%d hits, %d cells carved, %d new chunks" % (want_counts["rays_hit"], want_counts["cells_carved"], want_counts["new_chunks"]) in line, line
        counts = g.FusePointCloudRays(f, SENSOR, MAX_RANGE)
        assert counts == want_counts and not g.AreComponentsValid()
        want = ref.window(LOWER, SHAPE)
        assert np.array_equal(windows[k], want), "the C++ class's window after frame %d" % k
        assert np.array_equal(g.ExtractWindowRecords(LOWER, *SHAPE), want), "the pysdf_tools window after frame %d" % k
        want_sdf, _ = gpu.build_cells(want.view(np.float32), SHAPE, 8, 0, False, CELL, False)
        assert np.array_equal(sdfs[k].view(np.uint32), want_sdf.view(np.uint32)), "the example's SDF after frame %d" % k
        occ = R.occupancy(want)
        stray_most = max(stray_most, float(occ[stray]))
        if k < BOX_FRAMES:
            assert occ[face] > 0.5 and want_sdf[face] < 0
        elif faded is None and not occ[face] > 0.5:
            faded = k
        assert (want_sdf[face] < 0) == (faded is None), "the window's SDF shows the box's face until it fades, and not after"
    # by hand: four hits leave odds (7/3)^4 = 29.6, each miss multiplies them by 2/3, and 29.6 (2/3)^9 = 0.77 is the first below 1
    assert faded == BOX_FRAMES + 8 == 12
    assert "the box's face crosses 0.5 at frame %d" % faded in stdout
    # the spurious return: three misses (0.229), one hit (0.409), misses again -- never an obstacle
    assert stray_most == float(F.fuse(F.fuse(F.fuse(F.fuse(0.5, 0.4, 0.12, 0.97), 0.4, 0.12, 0.97), 0.4, 0.12, 0.97), 0.7, 0.12, 0.97)) < 0.5
    said = re.search(r"never passes 0.5 \(at most ([0-9.e-]+)\)", stdout)
    assert said and abs(float(said.group(1)) - stray_most) < 1e-5
    # another model, as keywords, beside the restatement
    model = (0.9, 0.45, 0.2, 0.8)
    _, want_counts = F.fuse_rays(ref, SENSOR, frames[0], MAX_RANGE, model)
    assert g.FusePointCloudRays(frames[0], SENSOR, MAX_RANGE, prob_hit=0.9, prob_miss=0.45, clamp_min=0.2, clamp_max=0.8) == want_counts
    assert np.array_equal(g.ExtractWindowRecords(LOWER, *SHAPE), ref.window(LOWER, SHAPE))
    # the refusals reach Python as ValueError (std::invalid_argument), and nothing is written
    before = g.GetCounts()
    for sensor, max_range in [((np.nan, 0.0, 0.0), 1.0), (SENSOR, 0.0), (SENSOR, 65536.5 * CELL)]:
        with pytest.raises(ValueError):
            g.FusePointCloudRays(frames[0], sensor, max_range)
    for bad in [dict(prob_hit=1.0), dict(prob_miss=0.0), dict(clamp_min=0.98), dict(clamp_max=np.nan), dict(prob_hit=np.nan)]:
        with pytest.raises(ValueError):
            g.FusePointCloudRays(frames[0], SENSOR, MAX_RANGE, **bad)
    assert g.GetCounts() == before
    assert np.array_equal(g.ExtractWindowRecords(LOWER, *SHAPE), ref.window(LOWER, SHAPE))
    assert g.FusePointCloudRays(np.zeros((0, 3), np.float32), SENSOR, 1.0)["cells_carved"] == 0
    with pytest.raises(RuntimeError):
        P.DynamicSpatialHashedCollisionMapGrid().FusePointCloudRays(frames[0], SENSOR, 1.0)
