"""GPU: DynamicSpatialHashedCollisionMapGrid::ExtractFrontierCells / ExtractFrontierWindowBits / ExtractFrontierClusters from C++
(examples/dsh_frontier.cpp, tests/dsh_frontier_class_check.cpp) and from pysdf_tools, against the restatement
(tests/dsh_frontier_restated.py): the example's dump compared byte for byte, the centroids against the stated host expression."""
import os
import subprocess

import numpy as np
import pytest

import dsh_cast_restated as C
import dsh_frontier_restated as F
import dsh_restated as R
import dsh_rays_restated as RR
from sdf_tools_amd import build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the numbers of examples/dsh_frontier.cpp
CELL, CHUNK, SENSOR, FRAME_RANGE = 0.05, (8, 8, 8), (0.025, 1.225, 1.225), 4.0
LOWER, SHAPE = (-4, 4, 4), (40, 40, 40)
UNKNOWN, FREE, FILLED = R.record(0.5, 0), R.record(0.0, 0), R.record(1.0, 0)


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dsh_frontier"))
    exe = build.build_example("dsh_frontier")
    out = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "dsh_frontier example done" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    load = lambda name, dtype: np.fromfile(os.path.join(d, name), dtype)
    got = {"cells_6": load("cells_6.i64", np.int64).reshape(-1, 3), "cells_26": load("cells_26.i64", np.int64).reshape(-1, 3),
           "bits": load("window_bits.u32", np.uint32), "label": load("cluster_label.u32", np.uint32), "cells": load("cluster_cells.i64", np.int64),
           "lower": load("cluster_lower.i64", np.int64).reshape(-1, 3), "upper": load("cluster_upper.i64", np.int64).reshape(-1, 3),
           "centroid": load("cluster_centroid.f64", np.float64).reshape(-1, 3), "cast_status": load("cast_status.u8", np.uint8),
           "cast_cell": load("cast_cell.i64", np.int64)}
    return out.stdout, load("frame.f32", np.float32).reshape(-1, 3), got


def labels_of(bits):
    """the labels of sdfgpu_components_bits_device restated: 6-connected components of both classes, numbered from 1 in the order a
    x -> y -> z scan meets them"""
    lab = np.zeros(bits.shape, np.uint32)
    k = 0
    for start in zip(*np.nonzero(np.ones(bits.shape, bool))):
        if lab[start]:
            continue
        k += 1
        lab[start] = k
        stack = [start]
        while stack:
            i = stack.pop()
            for d in F.OFFSETS_6:
                j = (i[0] + d[0], i[1] + d[1], i[2] + d[2])
                if all(0 <= j[a] < bits.shape[a] for a in range(3)) and not lab[j] and bits[j] == bits[start]:
                    lab[j] = k
                    stack.append(j)
    return lab


def clusters_of(ref, origin, lower, shape, min_cells, flags, cell=CELL):
    """ExtractFrontierClusters restated: the window's frontier, its components' statistics, and the centroid by the header's expression"""
    bits = F.frontier_window(ref, lower, shape, flags)
    out = {"label": [], "cells": [], "lower": [], "upper": [], "centroid": []}
    for s in F.component_stats(bits, labels_of(bits), shape):
        if s["count"] < min_cells:
            continue
        out["label"].append(s["label"])
        out["cells"].append(s["count"])
        out["lower"].append([lower[a] + s["lo"][a] for a in range(3)])
        out["upper"].append([lower[a] + s["hi"][a] for a in range(3)])
        g = [(np.float64(lower[a]) + (np.float64(s["sum"][a]) / np.float64(s["count"]) + 0.5)) * np.float64(cell) for a in range(3)]
        out["centroid"].append(ref.grid_to_world(origin, g))
    return {"label": np.array(out["label"], np.uint32), "cells": np.array(out["cells"], np.int64), "lower": np.array(out["lower"], np.int64).reshape(-1, 3),
            "upper": np.array(out["upper"], np.int64).reshape(-1, 3), "centroid": np.array(out["centroid"], np.float64).reshape(-1, 3)}


def same_clusters(what, got, want):
    for f in ("label", "cells", "lower", "upper"):
        assert np.array_equal(got[f], want[f]), "%s: %s" % (what, f)
    assert np.asarray(got["centroid"]).tobytes() == want["centroid"].tobytes(), what + ": the centroid, byte for byte"


def test_the_example_and_pysdf_tools_against_the_restatement(gpu, example):
    stdout, frame, got = example
    from sdf_tools_amd._bindings import load_pysdf_tools
    P = load_pysdf_tools()
    ref = R.Map(None, CELL, CHUNK, UNKNOWN)
    g = P.DynamicSpatialHashedCollisionMapGrid("world", CELL, 8, 8, 8, P.COLLISION_CELL(0.5))
    RR.insert_rays(ref, SENSOR, frame, FRAME_RANGE, FREE, FILLED)
    g.InsertPointCloudRays(frame, SENSOR, FRAME_RANGE, P.COLLISION_CELL(0.0), P.COLLISION_CELL(1.0))
    counts_of = lambda: {k: v for k, v in g.GetCounts().items() if k != "scratch_bytes"}
    before = counts_of()
    # the lists of the whole map under both rules
    want = [F.frontier_cells(ref, None, flags) for flags in (0, F.FRONTIER_26)]
    assert 1000 < len(want[0]) < len(want[1])
    assert "frontier cells: %d with an unknown face neighbour, %d with an unknown neighbour among all 26" % (len(want[0]), len(want[1])) in stdout, stdout
    assert got["cells_6"].tobytes() == want[0].tobytes() and got["cells_26"].tobytes() == want[1].tobytes()
    assert g.ExtractFrontierCells().tobytes() == want[0].tobytes() and g.ExtractFrontierCells(use_26=True).tobytes() == want[1].tobytes()
    # the window around the sensor: bits, the list of the same box, clusters
    want_bits = F.frontier_window_bits(ref, LOWER, SHAPE, F.FRONTIER_26)
    assert got["bits"].tobytes() == want_bits.tobytes() and g.ExtractFrontierWindowBits(LOWER, *SHAPE, use_26=True).tobytes() == want_bits.tobytes()
    assert g.ExtractFrontierWindowBits(LOWER, *SHAPE).tobytes() == F.frontier_window_bits(ref, LOWER, SHAPE, 0).tobytes()
    boxed = g.ExtractFrontierCells(LOWER, *SHAPE, True)
    assert boxed.tobytes() == F.frontier_cells(ref, (LOWER, SHAPE), F.FRONTIER_26).tobytes() and len(boxed) == int(np.unpackbits(want_bits.view(np.uint8)).sum())
    origin = np.eye(4)
    want_clusters = clusters_of(ref, origin, LOWER, SHAPE, 1, F.FRONTIER_26)
    assert len(want_clusters["label"]) >= 1 and want_clusters["cells"].sum() == len(boxed)
    same_clusters("the example's clusters", got, want_clusters)
    same_clusters("pysdf_tools' clusters", g.ExtractFrontierClusters(LOWER, *SHAPE), want_clusters)
    same_clusters("under the 6-rule, at least 5 cells", g.ExtractFrontierClusters(LOWER, *SHAPE, min_cells=5, use_26=False), clusters_of(ref, origin, LOWER, SHAPE, 5, 0))
    # the example's ray to the largest cluster's centroid
    largest = int(np.argmax(want_clusters["cells"]))
    st, hits = C.cast_segments(ref, np.array([SENSOR]), want_clusters["centroid"][largest:largest + 1], FRAME_RANGE, C.SKIP_FIRST | C.UNKNOWN_IS_FILLED)
    assert got["cast_status"][0] == st[0] and tuple(got["cast_cell"]) == tuple(hits["cell"][0])
    assert counts_of() == before
    # refusals reach Python as ValueError (std::invalid_argument); an uninitialised map throws RuntimeError
    for call in (lambda: g.ExtractFrontierCells(LOWER, 0, 1, 1), lambda: g.ExtractFrontierWindowBits(LOWER, 1, -1, 1), lambda: g.ExtractFrontierClusters(LOWER, 1 << 16, 1 << 16, 1),
                 lambda: g.ExtractFrontierWindowBits(LOWER, 1 << 16, 1 << 16, 1)):
        with pytest.raises(ValueError):
            call()
    blank = P.DynamicSpatialHashedCollisionMapGrid()
    for call in (lambda: blank.ExtractFrontierCells(), lambda: blank.ExtractFrontierCells(LOWER, 2, 2, 2), lambda: blank.ExtractFrontierWindowBits(LOWER, 2, 2, 2),
                 lambda: blank.ExtractFrontierClusters(LOWER, 2, 2, 2)):
        with pytest.raises(RuntimeError):
            call()
    assert counts_of() == before


def test_a_translated_map_through_pysdf_tools(gpu):
    from sdf_tools_amd._bindings import load_pysdf_tools
    P = load_pysdf_tools()
    t = (0.37, -1.21, 2.5)
    origin, inverse = np.eye(4), np.eye(4)
    origin[:3, 3] = t
    inverse[:3, 3] = [-v for v in t]          # Isometry3d::inverse() of a pure translation: exactly -t
    g = P.DynamicSpatialHashedCollisionMapGrid(P.Isometry3d(origin), "world", 0.25, 3, 2, 5, P.COLLISION_CELL(0.5))
    ref = R.Map(inverse, 0.25, (3, 2, 5), UNKNOWN)
    rng = np.random.default_rng(348)
    loc = (rng.integers(-7, 7, (300, 3)) + 0.5) * 0.25 + np.array(t)
    values = np.array([[FREE, FREE, FILLED, UNKNOWN][k % 4] for k in range(len(loc))], np.uint64)
    assert np.array_equal(g.SetCells(loc, values), ref.set_cells(loc, values))
    lower, shape = (-8, -8, -8), (16, 16, 16)

    want = clusters_of(ref, origin, lower, shape, 2, F.FRONTIER_26, cell=0.25)
    assert len(want["label"]) >= 3
    same_clusters("a translated origin", g.ExtractFrontierClusters(lower, *shape, min_cells=2), want)
    assert g.ExtractFrontierCells(lower, *shape).tobytes() == F.frontier_cells(ref, (lower, shape), 0).tobytes()


def test_the_frontier_methods_of_the_class_on_the_gpu(tmp_path):
    """tests/dsh_frontier_class_check.cpp without `cpu`: each method once through the C++ class, hand-worked"""
    tests = os.path.join(ROOT, "tests")
    exe = str(tmp_path / "dsh_frontier_class_check")
    pkg = os.path.join(ROOT, "sdf_tools_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", "-DSDF_TOOLS_VECTOR_ADOPT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(tests, "dsh_frontier_class_check.cpp"), "-o", exe, "-L", pkg, "-lsdfgpu", "-Wl,-rpath," + pkg, "-lz"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dsh frontier class OK" in r.stdout, r.stdout + r.stderr
