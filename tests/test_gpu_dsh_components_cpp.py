"""GPU: DynamicSpatialHashedCollisionMapGrid::UpdateConnectedComponents / GetNumConnectedComponents / AreComponentsValid from C++
(examples/dsh_components.cpp) and from pysdf_tools, against the restatement (tests/dsh_components_restated.py on a map fused by
tests/dsh_fusion_restated.py): the example's dump compared byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import dsh_components_restated as C
import dsh_frontier_restated as F
import dsh_fusion_restated as FU
import dsh_restated as R
from sdf_tools_amd import build

pytestmark = pytest.mark.gpu

# the numbers of examples/dsh_components.cpp
CELL, CHUNK, RANGE = 0.05, (8, 8, 8), 6.0
UNKNOWN = R.record(0.5, 0)


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dsh_components"))
    exe = build.build_example("dsh_components")
    out = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "dsh_components example done" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    load = lambda name, dtype: np.fromfile(os.path.join(d, name), dtype)
    frames = [load("frame_%d.f32" % k, np.float32).reshape(-1, 3) for k in range(3)]
    return out.stdout, frames, load("sensors.f64", np.float64).reshape(3, 3), load("frontier.i64", np.int64).reshape(-1, 3), load("labels.u32", np.uint32), \
        load("summary.u32", np.uint32)


def label_at(ref, cell):
    record, found = ref.get_cell(tuple(int(v) for v in cell))
    assert found != R.NOT_FOUND
    return record >> 32


def every_record(ref):
    """(the centres of every cell of every live chunk, the records Get must return there)"""
    n = np.array(ref.n)
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in ref.n], indexing="ij"), -1).reshape(-1, 3)
    loc, want = [], []
    for c, (kind, what) in ref.chunks.items():
        loc.append((idx + np.array(c) * n + 0.5) * CELL)
        want.append(np.asarray(what, np.uint64).reshape(-1) if kind == "cells" else np.full(len(idx), what, np.uint64))
    return np.concatenate(loc), np.concatenate(want)


def test_the_example_and_pysdf_tools_against_the_restatement(gpu, example):
    stdout, frames, sensors, frontier, labels, summary = example
    from sdf_tools_amd._bindings import load_pysdf_tools
    P = load_pysdf_tools()
    ref = R.Map(None, CELL, CHUNK, UNKNOWN)
    g = P.DynamicSpatialHashedCollisionMapGrid("world", CELL, 8, 8, 8, P.COLLISION_CELL(0.5))
    assert g.components_info() == (0, 0, False) and g.GetNumConnectedComponents() == (0, False) and not g.AreComponentsValid()
    for frame, sensor in zip(frames, sensors):
        FU.fuse_rays(ref, sensor, frame, RANGE)
        g.FusePointCloudRays(frame, sensor, RANGE)
    assert not g.AreComponentsValid()
    want_frontier = F.frontier_cells(ref, None, 0)
    count = C.apply(ref, C.UNKNOWN_APART)
    robot = label_at(ref, np.floor(sensors[0] / CELL))
    want_labels = np.array([label_at(ref, c) for c in want_frontier], np.uint32)
    reachable = int((want_labels == robot).sum())
    # the example's dump and its printed lines
    assert frontier.tobytes() == want_frontier.tobytes() and labels.tobytes() == want_labels.tobytes()
    assert summary.tolist() == [count, robot, reachable, len(want_labels) - reachable] and reachable > 0 and len(want_labels) > reachable
    assert "%d components; the robot stands in component %d" % (count, robot) in stdout, stdout
    assert "frontier cells: %d, %d in the robot's component, %d elsewhere" % (len(want_labels), reachable, len(want_labels) - reachable) in stdout, stdout
    # the closet's frontier cells all lie behind the room's x = 3 m wall, the robot's in front of it
    assert (frontier[labels == robot][:, 0] < 60).all() and (frontier[labels != robot][:, 0] > 60).all()
    # pysdf_tools: the same labels through GetBatch on every cell of every live chunk, both spellings of the update, and the stored count while the map is valid
    before = {k: v for k, v in g.GetCounts().items() if k != "scratch_bytes"}
    assert g.update_components(1) == count and g.components_info() == (count, 1, True) and g.AreComponentsValid()
    assert g.UpdateConnectedComponents(True) == count and g.GetNumConnectedComponents() == (count, True)
    loc, want_records = every_record(ref)
    records, statuses = g.GetBatch(loc)
    assert records.tobytes() == want_records.tobytes() and (statuses != R.NOT_FOUND).all()
    assert {k: v for k, v in g.GetCounts().items() if k != "scratch_bytes"} == before
    plain = C.apply(ref, 0)                                                    # the other rule: asked for, so computed again
    assert g.UpdateConnectedComponents() == plain < count and g.components_info() == (plain, 0, True)
    assert g.GetBatch(loc)[0].tobytes() == every_record(ref)[1].tobytes()
    # a window as a CollisionMapGrid carries the labels
    lower, shape = (-2, 4, 20), (12, 9, 7)
    assert g.ExtractWindowRecords(lower, *shape).tobytes() == ref.window(lower, shape).tobytes()
    # a change clears the validity; a refused flag is a ValueError; an uninitialised map answers 0
    g.SetCell(0.525, 0.525, 1.225, P.COLLISION_CELL(1.0))
    assert g.components_info() == (plain, 0, False) and not g.AreComponentsValid() and g.GetNumConnectedComponents() == (plain, False)
    with pytest.raises(ValueError):
        g.update_components(2)
    blank = P.DynamicSpatialHashedCollisionMapGrid()
    assert blank.UpdateConnectedComponents() == 0 and blank.update_components() == 0 and blank.components_info() == (0, 0, False)
    assert blank.GetNumConnectedComponents() == (0, False) and not blank.AreComponentsValid()
