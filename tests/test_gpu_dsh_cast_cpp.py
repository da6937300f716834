"""GPU: DynamicSpatialHashedCollisionMapGrid::CastRays / CastSegments / CastRay from C++ (examples/dsh_cast.cpp) and from pysdf_tools,
against the restatement of a ray cast (tests/dsh_cast_restated.py): the example's dumped queries replayed, its results compared field by
field and byte for byte, the distances against the stated host expression."""
import os
import subprocess

import numpy as np
import pytest

import dsh_cast_restated as C
import dsh_restated as R
import dsh_rays_restated as RR
from sdf_tools_amd import build

pytestmark = pytest.mark.gpu

# the numbers of examples/dsh_cast.cpp
CELL, CHUNK, SENSOR, SECOND_SENSOR = 0.05, (8, 8, 8), (0.025, 1.225, 1.225), (0.025, 0.375, 1.875)
FRAME_RANGE, SCAN_RANGE, LOS_RANGE = 4.0, 3.2, 4.0
UNKNOWN, FREE, FILLED = R.record(0.5, 0), R.record(0.0, 0), R.record(1.0, 0)
FIELDS = [("status", np.uint8), ("cell", np.int64), ("record", np.uint64), ("t", np.float64), ("step", np.uint32), ("found", np.uint32), ("distance", np.float64)]
SUFFIX = {np.uint8: "u8", np.int64: "i64", np.uint64: "u64", np.float64: "f64", np.uint32: "u32"}


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dsh_cast"))
    exe = build.build_example("dsh_cast")
    out = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "dsh_cast example done" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    load = lambda name, dtype: np.fromfile(os.path.join(d, name), dtype)
    got = {q: {f: load("%s_%s.%s" % (q, f, SUFFIX[t]), t) for f, t in FIELDS} for q in ("scan", "los", "los_unknown")}
    for q in got.values():
        q["cell"] = q["cell"].reshape(-1, 3)
    return out.stdout, load("frame.f32", np.float32).reshape(-1, 3), load("scan.f32", np.float32).reshape(-1, 3), \
        load("los_starts.f64", np.float64).reshape(-1, 3), load("los_ends.f64", np.float64).reshape(-1, 3), got


def check(what, got, want, starts, ends):
    """a dict of arrays (the example's dump, or pysdf_tools' result) against the restatement's (statuses, hits)"""
    st, hits = want
    assert np.array_equal(got["status"], st), what + ": statuses"
    for f in ("cell", "record", "step", "found"):
        assert np.array_equal(got[f], hits[f]), "%s: %s" % (what, f)
    assert got["t"].tobytes() == hits["t"].tobytes(), what + ": t, byte for byte"
    distance = np.array([0.0 if s == C.CAST_SKIPPED else C.distance(a, b, t) for s, a, b, t in zip(st, starts, ends, hits["t"])])
    assert got["distance"].tobytes() == distance.tobytes(), what + ": distance = t * sqrt((dx dx + dy dy) + dz dz) in double"


def test_the_example_and_pysdf_tools_against_the_restatement(gpu, example):
    stdout, frame, scan, los_starts, los_ends, got = example
    from sdf_tools_amd._bindings import load_pysdf_tools
    P = load_pysdf_tools()
    ref = R.Map(None, CELL, CHUNK, UNKNOWN)
    g = P.DynamicSpatialHashedCollisionMapGrid("world", CELL, 8, 8, 8, P.COLLISION_CELL(0.5))
    RR.insert_rays(ref, SENSOR, frame, FRAME_RANGE, FREE, FILLED)
    g.InsertPointCloudRays(frame, SENSOR, FRAME_RANGE, P.COLLISION_CELL(0.0), P.COLLISION_CELL(1.0))
    counts_of = lambda: {k: v for k, v in g.GetCounts().items() if k != "scratch_bytes"}   # (the host forms' staging may grow)
    before = counts_of()
    # the predicted scan: all four statuses, blockers on the box and on the wall
    want = C.cast_rays(ref, SECOND_SENSOR, scan, SCAN_RANGE, 0)
    counts = [int((want[0] == s).sum()) for s in (C.CAST_BLOCKED, C.CAST_CLEAR, C.CAST_CLEAR_IN_RANGE, C.CAST_SKIPPED)]
    assert counts[0] > 100 and counts[2] > 100 and counts[3] == 17 and set(want[1]["record"][want[0] == C.CAST_BLOCKED].tolist()) == {FILLED}
    assert "scan: %d blocked, %d clear, %d clear in range, %d skipped" % tuple(counts) in stdout, stdout
    sensors = np.tile(np.array(SECOND_SENSOR), (len(scan), 1))
    check("the example's scan", got["scan"], want, sensors, scan.astype(np.float64))
    check("pysdf_tools' scan", g.CastRays(scan, SECOND_SENSOR, SCAN_RANGE, False), want, sensors, scan.astype(np.float64))
    blocked_x = want[1]["cell"][want[0] == C.CAST_BLOCKED][:, 0]
    assert {30, 60} <= set(blocked_x.tolist()), "the scan meets the box's face (x cell 30) and the wall (x cell 60)"
    # line of sight with both skips, unknown space clear and in the way
    for name, unknown in (("los", False), ("los_unknown", True)):
        want = C.cast_segments(ref, los_starts, los_ends, LOS_RANGE, C.SKIP_FIRST | C.SKIP_LAST | (C.UNKNOWN_IS_FILLED if unknown else 0))
        check("the example's " + name, got[name], want, los_starts, los_ends)
        check("pysdf_tools' " + name, g.CastSegments(los_starts, los_ends, LOS_RANGE, unknown, True, True), want, los_starts, los_ends)
        for k in range(len(los_starts)):
            one = g.CastRay(los_starts[k], los_ends[k], LOS_RANGE, unknown, skip_first=True, skip_last=True)
            check("pysdf_tools' CastRay %d" % k, one, (want[0][k:k + 1], want[1][k:k + 1]), los_starts[k:k + 1], los_ends[k:k + 1])
        if not unknown:
            assert want[0].tolist()[:2] == [C.CAST_BLOCKED, C.CAST_CLEAR]
        else:
            assert (want[0] == C.CAST_BLOCKED).sum() > (got["los"]["status"] == C.CAST_BLOCKED).sum(), "unknown space blocks more"
    # the three skip flags reach the kernel one by one
    for kw in ({"skip_first": True}, {"skip_last": True}, {}):
        flags = (C.SKIP_FIRST if kw.get("skip_first") else 0) | (C.SKIP_LAST if kw.get("skip_last") else 0)
        check("flags %d" % flags, g.CastSegments(los_starts, los_ends, LOS_RANGE, False, **kw), C.cast_segments(ref, los_starts, los_ends, LOS_RANGE, flags),
              los_starts, los_ends)
    # nothing was written, components_valid_ included (it is false after the frame and no cast can make it true; info is the witness)
    assert counts_of() == before and not g.AreComponentsValid()
    empty = g.CastRays(np.zeros((0, 3), np.float32), SECOND_SENSOR, 1.0, False)
    assert all(len(v) == 0 for v in empty.values()) and empty["cell"].shape == (0, 3)
    # the refusals reach Python as ValueError (std::invalid_argument); an uninitialised map throws RuntimeError
    for sensor, max_range in [((np.nan, 0.0, 0.0), 1.0), (SECOND_SENSOR, 0.0), (SECOND_SENSOR, 65536.5 * CELL), (SECOND_SENSOR, np.nan)]:
        with pytest.raises(ValueError):
            g.CastRays(scan, sensor, max_range, False)
    for max_range in (0.0, 65536.5 * CELL, np.nan):
        with pytest.raises(ValueError):
            g.CastSegments(los_starts, los_ends, max_range, False)
        with pytest.raises(ValueError):
            g.CastRay(los_starts[0], los_ends[0], max_range, False)
    with pytest.raises(ValueError):
        g.CastSegments(los_starts, los_ends[:-1], 1.0, False)
    assert counts_of() == before
    blank = P.DynamicSpatialHashedCollisionMapGrid()
    with pytest.raises(RuntimeError):
        blank.CastRays(scan, SECOND_SENSOR, 1.0, False)
    with pytest.raises(RuntimeError):
        blank.CastSegments(los_starts, los_ends, 1.0, False)
    with pytest.raises(RuntimeError):
        blank.CastRay(los_starts[0], los_ends[0], 1.0, False)
