"""GPU: the removal methods of DynamicSpatialHashedCollisionMapGrid from C++ (examples/dsh_sliding.cpp, tests/dsh_remove_class_check.cpp)
and from pysdf_tools, against the restatement (tests/dsh_remove_restated.py, tests/dsh_fusion_restated.py): the example's frames
replayed behind the same RetainBox, its counts, its last window and SDF compared byte for byte, and each method once."""
import os
import re
import subprocess

import numpy as np
import pytest

import dsh_fusion_restated as F
import dsh_remove_restated as X
import dsh_restated as R
from sdf_tools_amd import build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the numbers of examples/dsh_sliding.cpp
CELL, CHUNK, MAX_RANGE, FRAMES, PIXELS = 0.1, (8, 8, 8), 4.0, 16, 24
BEHIND, AHEAD, SIDE = 16, 48, 16
BYTE_LIMIT = 4096 * 12 + 192 * (24 + 8 * 512)
SHAPE = (48, 28, 28)
UNKNOWN = R.record(0.5, 0)


def sensor(k):
    return (0.45 + 0.8 * k, 0.0, 0.0)


def region(k):
    return (4 + 8 * k - BEHIND, -SIDE, -SIDE), (BEHIND + AHEAD, 2 * SIDE, 2 * SIDE)


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    d = tmp_path_factory.mktemp("dsh_sliding")
    exe = build.build_example("dsh_sliding")
    out = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "dsh_sliding example done" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    frames = [np.fromfile(os.path.join(str(d), "frame_%d.f32" % k), np.float32).reshape(-1, 3) for k in range(FRAMES)]
    window = np.fromfile(os.path.join(str(d), "window.cells"), np.uint64).reshape(SHAPE)
    sdf = np.fromfile(os.path.join(str(d), "window_sdf.f32"), np.float32).reshape(SHAPE)
    return out.stdout, frames, window, sdf


def test_the_sliding_example_and_pysdf_tools_against_the_restatement(gpu, example):
    stdout, frames, window, sdf = example
    from sdf_tools_amd._bindings import load_pysdf_tools
    P = load_pysdf_tools()
    ref = R.Map(None, CELL, CHUNK, UNKNOWN)
    g = P.DynamicSpatialHashedCollisionMapGrid(P.Isometry3d(np.eye(4)), "world", CELL, 8, 8, 8, P.COLLISION_CELL(0.5), byte_limit=BYTE_LIMIT)
    assert np.floor(np.float64(sensor(FRAMES - 1)[0]) / np.float64(CELL)) == 4 + 8 * (FRAMES - 1)
    for k, f in enumerate(frames):
        assert len(f) == PIXELS * PIXELS
        lower, extent = region(k)
        forgotten = X.retain_box(ref, lower, extent)
        assert g.RetainBox(lower, *extent) == forgotten and (k < 3 or forgotten > 0)
        _, want_counts = F.fuse_rays(ref, sensor(k), f, MAX_RANGE)
        assert g.FusePointCloudRays(f, sensor(k), MAX_RANGE) == want_counts and not g.AreComponentsValid()
        line = [l for l in stdout.splitlines() if l.startswith("frame %d: " % k)][0]
        assert "%d chunks forgotten, %d new chunks, %d chunks live" % (forgotten, want_counts["new_chunks"], len(ref.chunks)) in line, line
        counts = g.GetCounts()
        assert counts["chunk_filled"] + counts["cell_filled"] == len(ref.chunks) and counts["bytes_held"] <= BYTE_LIMIT == counts["byte_limit"]
        assert "%d bytes held" % counts["bytes_held"] in line, line
    # without RetainBox the example's limited map got stuck; behind the robot nothing is found; the window is the restatement's
    stuck = re.search(r"without RetainBox the limited map was stuck from frame (\d+) on", stdout)
    assert stuck and 3 <= int(stuck.group(1)) < FRAMES and "byte limit" in stdout
    behind = np.array([(sensor(k)[0], 0.05, 0.05) for k in range(8)])
    rec, st = g.GetBatch(behind)
    assert st.tolist() == [0] * 8 == ref.get_batch(behind)[1].tolist() and (rec == np.uint64(UNKNOWN)).all()
    lower = (4 + 8 * (FRAMES - 1) - 8, -14, -14)
    want = ref.window(lower, SHAPE)
    assert np.array_equal(window, want), "the example's window at the robot"
    assert np.array_equal(g.ExtractWindowRecords(lower, *SHAPE), want), "the pysdf_tools window at the robot"
    want_sdf, _ = gpu.build_cells(want.view(np.float32), SHAPE, 8, 0, False, CELL, False)
    assert np.array_equal(sdf.view(np.uint32), want_sdf.view(np.uint32)) and (want_sdf < 0).any() and (want_sdf > 0).any()
    # each method once, beside the restatement
    live = np.array(sorted(ref.chunks))
    centre = lambda c: (np.asarray(c) * 8 + 3.5) * CELL
    assert g.RemoveChunk(*centre(live[0])) is True and g.RemoveChunk(*centre(live[0])) is False and g.RemoveChunk(np.nan, 0.0, 0.0) is False
    assert X.remove_chunks(ref, [centre(live[0])]).tolist() == [1]
    loc = np.array([centre(live[3]), centre(live[3]) + 0.1, (np.inf, 0, 0), centre(live[0]), centre(live[5]), centre((500, 0, 0))])
    got = g.RemoveChunks(loc)
    assert got.dtype == np.uint8 and got.tolist() == X.remove_chunks(ref, loc).tolist() == [1, 0, 0, 0, 1, 0]
    box = ((4 + 8 * (FRAMES - 1), -3, -20), (9, 7, 40))
    assert g.RemoveBox(box[0], *box[1]) == X.retain_box(ref, box[0], box[1], True) > 0
    want = ref.window(lower, SHAPE)
    assert np.array_equal(g.ExtractWindowRecords(lower, *SHAPE), want) and not g.AreComponentsValid()
    before = g.GetCounts()
    g.ShrinkToFit(5)
    after = g.GetCounts()
    plan = X.shrink_plan(len(ref.chunks), 5, before["capacity_chunks"], before["table_capacity"], 512)
    assert (after["capacity_chunks"], after["table_capacity"], after["bytes_held"]) == plan and plan[0] < before["capacity_chunks"]
    assert np.array_equal(g.ExtractWindowRecords(lower, *SHAPE), want)
    _, want_counts = F.fuse_rays(ref, sensor(FRAMES - 1), frames[-1], MAX_RANGE)                # the pool grows again, the marks are made again
    assert g.FusePointCloudRays(frames[-1], sensor(FRAMES - 1), MAX_RANGE) == want_counts
    assert np.array_equal(g.ExtractWindowRecords(lower, *SHAPE), ref.window(lower, SHAPE))
    for lower_bad, extent_bad in [(((1 << 40) + 1, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, -1, 1))]:
        with pytest.raises(ValueError):
            g.RetainBox(lower_bad, *extent_bad)
    with pytest.raises(ValueError):
        g.ShrinkToFit(-1)
    assert g.Clear() == len(ref.chunks) > 0 and g.Clear() == 0
    assert g.GetCounts()["chunk_filled"] + g.GetCounts()["cell_filled"] == 0 and g.GetBatch(loc)[1].tolist() == [0] * 6
    empty = P.DynamicSpatialHashedCollisionMapGrid()
    assert empty.RemoveChunk(0.0, 0.0, 0.0) is False and empty.Clear() == 0
    for call in (lambda: empty.RemoveChunks(loc), lambda: empty.RetainBox((0, 0, 0), 1, 1, 1), lambda: empty.RemoveBox((0, 0, 0), 1, 1, 1), lambda: empty.ShrinkToFit()):
        with pytest.raises(RuntimeError):
            call()


def test_the_removal_methods_of_the_class_on_the_gpu():
    """tests/dsh_remove_class_check.cpp without `cpu`: each method once through the C++ class, hand-worked"""
    tests = os.path.join(ROOT, "tests")
    exe = os.path.join(tests, "dsh_remove_class_check")
    pkg = os.path.join(ROOT, "sdf_tools_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", "-DSDF_TOOLS_VECTOR_ADOPT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(tests, "dsh_remove_class_check.cpp"), "-o", exe, "-L", pkg, "-lsdfgpu", "-Wl,-rpath," + pkg, "-lz"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dsh remove class OK" in r.stdout, r.stdout + r.stderr
