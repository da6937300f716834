"""The display methods of SignedDistanceField, CollisionMapGrid and TaggedObjectCollisionMapGrid through pysdf_tools (numpy forms:
(points float64 [n, 3], colors float32 [n, 4]), the Separate / UniqueNs forms [(ns, points, colors)]) against the restatement
(tests/display_restated.py), bit for bit: which cells, in which order, where, in which colour; what every method fills besides the
elements (header, ns, id, type, action, pose, scale); marker order and pruning of the UniqueNs forms; the palette's id 0.  And
examples/display_export.cpp, client code written like the reference's, built as tests/test_cpp_example.py builds its own."""
import math
import os
import subprocess

import numpy as np
import pytest

import display_cases as C
import display_restated as R
import stream_harness as H
from sdf_tools_amd._bindings import load_pysdf_tools

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (9, 7, 33)
RES = 0.1
CELL = (RES, RES, RES)
# a quarter turn about z and a translation: orientation (0, 0, sin 45, cos 45)
ORIGIN = [[0.0, -1.0, 0.0, 1.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.25], [0.0, 0.0, 0.0, 1.0]]
RED, GREEN, BLUE, NONE = (1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 0.5), (0.0, 0.0, 1.0, 0.25), (0.3, 0.3, 0.3, 0.0)
NS = "tagged_object_collision_map_display"


def _same(what, got, idx, colors):
    pts, col = got
    assert pts.dtype == np.float64 and col.dtype == np.float32, what
    assert pts.tobytes() == R.points(idx, SHAPE, CELL).tobytes(), "%s: points differ (%d got, %d expected)" % (what, len(pts), len(idx))
    assert col.tobytes() == np.ascontiguousarray(colors, np.float32).reshape(-1, 4).tobytes(), "%s: colours differ" % what


def _info(info, ns):
    assert info["frame_id"] == "display_frame" and info["ns"] == ns
    assert (info["id"], info["type"], info["action"], info["lifetime"], info["frame_locked"]) == (1, 6, 0, 0.0, False)   # CUBE_LIST, ADD
    assert info["position"] == (1.5, -2.0, 0.25) and info["scale"] == (RES, RES, RES)
    assert np.allclose(info["orientation"], (0.0, 0.0, math.sqrt(0.5), math.sqrt(0.5)), atol=1e-15)


@pytest.fixture(scope="module")
def m():
    return load_pysdf_tools()


@pytest.fixture(scope="module")
def occ():
    return np.random.default_rng(21).choice(C.OCC_VALUES, size=SHAPE)


@pytest.fixture(scope="module")
def grid(m, occ):
    g = m.CollisionMapGrid(m.Isometry3d(ORIGIN), "display_frame", RES, *SHAPE, m.COLLISION_CELL(0.0))
    g.SetOccupancyFromNumpy(occ)
    return g


def _palette(m, ids, alpha=1.0):
    table = {int(i): m.TaggedObjectCollisionMapGrid.GenerateComponentColor(int(i), alpha) for i in np.unique(ids)}
    return np.array([table[int(i)] for i in ids], np.float32).reshape(-1, 4)


def test_the_palette(m):
    gen = m.TaggedObjectCollisionMapGrid.GenerateComponentColor
    assert gen(0) == (0.0, 0.0, 0.0, 0.0) and gen(0, 0.7) == (0.0, 0.0, 0.0, 0.0), "id 0 has alpha 0: never drawn"
    seen = set()
    for i in range(1, 200):
        c = gen(i, 0.5)
        assert c[3] == 0.5 and max(c[:3]) == 1.0 and min(c[:3]) == 0.0 and c[:3] not in seen
        seen.add(c[:3])


@pytest.mark.parametrize("colors", [(RED, GREEN, BLUE), (RED, NONE, BLUE), (NONE, GREEN, NONE), (NONE, NONE, NONE)])
def test_collision_map_occupancy_exports(m, grid, occ, colors):
    table = np.array(colors, np.float32)
    mask = sum(1 << k for k in range(3) if colors[k][3] > 0)
    for surf, single, separate, names in ((False, grid.ExportForDisplay, grid.ExportForSeparateDisplay, ("collision_only", "free_only", "unknown_only")),
                                         (True, grid.ExportSurfacesForDisplay, grid.ExportSurfacesForSeparateDisplay,
                                          ("collision_surfaces_only", "free_surfaces_only", "unknown_surfaces_only"))):
        idx, keys = R.select_occupancy(occ, mask, surf)
        _same("single marker, surfaces %s" % surf, single(*colors), idx, table[keys])
        markers = separate(*colors)
        assert [ns for ns, _, _ in markers] == list(names)
        for k, (ns, pts, col) in enumerate(markers):                # (an invisible class keeps its marker, empty)
            _same(ns, (pts, col), idx[keys == k], table[keys[keys == k]])
    _info(grid.ExportForDisplayInfo(*colors), "collision_map_display")


def test_collision_map_components_export(m, grid, occ):
    assert grid.UpdateConnectedComponents() > 1
    comp = grid.GetRawCellsNumpy().view(np.uint32)[..., 1].reshape(-1)
    want = _palette(m, comp)
    _same("every component coloured", grid.ExportConnectedComponentsForDisplay(True), np.arange(occ.size, dtype=np.uint32), want)
    want[(occ == np.float32(0.5)).reshape(-1)] = (0.5, 0.5, 0.5, 1.0)      # (NaN != 0.5: coloured)
    _same("unknown grey", grid.ExportConnectedComponentsForDisplay(False), np.arange(occ.size, dtype=np.uint32), want)


def test_sdf_exports(m, grid):
    sdf, _ = grid.ExtractSignedDistanceField(1e6, True, False)
    d = sdf.GetRawDataNumpy().reshape(SHAPE)
    for alpha in (0.5, 7.0):
        pts, col = sdf.ExportForDisplay(alpha)
        assert pts.tobytes() == R.points(np.arange(d.size), SHAPE, CELL).tobytes()
        assert H.same_or_nan(col.reshape(SHAPE + (4,)), R.sdf_colors(d, alpha))
    pts, col = sdf.ExportForDisplayCollisionOnly(0.25)
    assert pts.tobytes() == R.points(R.select_sdf(d)[0], SHAPE, CELL).tobytes() and col.shape == (0, 4) and len(pts) > 0
    _info(sdf.ExportForDisplayInfo(0.5, False), "sdf_display")
    info = sdf.ExportForDisplayInfo(0.25, True)
    _info(info, "sdf_display")
    assert info["color"] == (1.0, 0.0, 0.0, 0.25) and info["colors"] == 0


@pytest.fixture(scope="module")
def tagged(m, occ):
    rng = np.random.default_rng(22)
    objects = rng.choice(np.array([0, 3, 7, 300, 70000], np.uint32), size=SHAPE)
    objects[0, 0, :4] = (300, 7, 0, 70000)                          # first appearance in the scan: 300, 7, 70000, then 3 somewhere
    objects[0, 0, 4:] = 300
    segments = rng.integers(0, 4, size=SHAPE).astype(np.uint32)
    rec = np.zeros(SHAPE + (4,), np.uint32)
    rec[..., 0] = occ.view(np.uint32)
    rec[..., 2] = objects
    rec[..., 3] = segments
    g = m.TaggedObjectCollisionMapGrid(m.Isometry3d(ORIGIN), "display_frame", RES, *SHAPE, m.TAGGED_OBJECT_COLLISION_CELL(0.0, 0))
    g.SetRawCellsNumpy(rec.view(np.uint8).reshape(SHAPE + (16,)))
    return g, objects, segments


def _first_appearance(objects):
    flat = objects.reshape(-1)
    ids, first = np.unique(flat, return_index=True)
    return [int(i) for i in ids[np.argsort(first)] if i != 0]


def test_tagged_exports_by_object(m, tagged, occ):
    g, objects, _ = tagged
    info = g.DefaultMarker()
    _info(info, "")
    for alpha, draw in ((1.0, []), (0.5, [7]), (0.5, [70000, 3, 0, 11])):
        idx, keys = R.select_key_field(objects, occ, draw or None, False)
        _same("ExportForDisplay %s" % draw, g.ExportForDisplay(alpha, draw), idx, _palette(m, keys, alpha))
    assert len(g.ExportForDisplay(0.0)[0]) == 0, "alpha 0: nothing is visible"
    # UniqueNs: the listed objects first, in list order (absent ones and id 0 pruned; a repeated id keeps its last place); all objects in
    # the order of their first cell when the list is empty
    for draw, order in (([], _first_appearance(objects)), ([7, 11, 3, 0, 300], [7, 3, 300]), ([3, 7, 3], [7, 3]), ([11], [])):
        markers = g.ExportForDisplayUniqueNs(0.5, draw)
        assert [ns for ns, _, _ in markers] == ["%s_%d" % (NS, i) for i in order], draw
        for i, (ns, pts, col) in zip(order, markers):
            idx = np.flatnonzero(objects.reshape(-1) == i).astype(np.uint32)
            _same(ns, (pts, col), idx, _palette(m, np.full(len(idx), i), 0.5))
    assert _first_appearance(objects)[:3] == [300, 7, 70000]


def test_tagged_exports_by_color_map(m, tagged, occ):
    g, objects, _ = tagged
    flat = objects.reshape(-1)
    for cmap in ({}, {7: RED, 300: NONE}, {0: GREEN, 70000: BLUE, 11: RED}):
        def color(i):
            return cmap[i] if i in cmap else m.TaggedObjectCollisionMapGrid.GenerateComponentColor(i)
        visible = [i for i in (0, 3, 7, 300, 70000) if color(i)[3] > 0]
        idx = np.flatnonzero(np.isin(flat, visible)).astype(np.uint32)
        _same("ExportForDisplay(color_map %s)" % sorted(cmap), g.ExportForDisplay(cmap), idx, np.array([color(int(i)) for i in flat[idx]], np.float32))
        order = [i for i in sorted(cmap) if i in visible] + [i for i in _first_appearance(objects) if i not in cmap and i in visible]
        markers = g.ExportForDisplayUniqueNs(cmap)
        assert [ns for ns, _, _ in markers] == ["%s_%d" % (NS, i) for i in order], sorted(cmap)
        for i, (ns, pts, col) in zip(order, markers):
            idx = np.flatnonzero(flat == i).astype(np.uint32)
            _same(ns, (pts, col), idx, np.tile(np.float32(color(i)), (len(idx), 1)))


def test_tagged_occupancy_components_segments_and_surface(m, tagged, occ):
    g, objects, segments = tagged
    table = np.array((RED, NONE, BLUE), np.float32)
    idx, keys = R.select_occupancy(occ, 5, False)
    _same("ExportForDisplayOccupancyOnly", g.ExportForDisplayOccupancyOnly(RED, NONE, BLUE), idx, table[keys])
    g.UpdateConnectedComponents()
    comp = g.GetRawCellsNumpy().view(np.uint32)[..., 1].reshape(-1)
    want = _palette(m, comp)
    want[(occ == np.float32(0.5)).reshape(-1)] = (0.5, 0.5, 0.5, 1.0)
    _same("components", g.ExportConnectedComponentsForDisplay(False), np.arange(occ.size, dtype=np.uint32), want)
    for obj, seg in ((7, 2), (300, 0), (11, 1), (0, 3)):
        idx = np.flatnonzero((objects.reshape(-1) == obj) & (segments.reshape(-1) == seg)).astype(np.uint32)
        _same("segment %d of object %d" % (seg, obj), g.ExportConvexSegmentForDisplay(obj, seg), idx, _palette(m, np.full(len(idx), seg)))
    cells = [(0, 0, 0), (8, 6, 32), (4, 3, 7)]
    pts, col = g.ExportSurfaceForDisplay(cells, GREEN)
    want = {tuple(RES * (np.array(c) + 0.5)) for c in cells}
    assert {tuple(p) for p in pts} == want and (col == np.float32(GREEN)).all() and len(pts) == 3


def test_cpp_display_example():
    from sdf_tools_amd import build as b
    exe = b.build_example("display_export")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = []
    for line in r.stdout.splitlines():
        name, rest = line.split(" ", 1)
        rows.append((name, dict(kv.split("=", 1) for kv in rest.split(" "))))
    for name, f in rows:
        assert f["frame"] == "tutorial_frame" and (f["id"], f["type"], f["action"]) == ("1", "6", "0") and float(f["scale"]) == 0.25, name
        assert [float(v) for v in f["pose"].split(",")] == [-5.0, -5.0, -5.0, 0.0, 0.0, 0.0, 1.0], name
    by = {}
    for name, f in rows:
        by.setdefault(name, []).append(f)
    occ = np.zeros((40, 40, 40), np.float32)
    occ[:20, :20, :20] = 1.0
    occ[39, 39, 39] = 0.5

    def check(f, idx, ns, colors=None):
        p = R.points(idx, (40, 40, 40), (0.25,) * 3)
        assert f["ns"] == ns and int(f["points"]) == len(idx) and int(f["colors"]) == (len(idx) if colors is None else colors), ns
        if len(idx):
            assert [float(v) for v in f["first"].split(",")] == p[0].tolist(), ns
            assert math.isclose(float(f["sum"]), float(p.sum()), rel_tol=1e-9), ns
    check(by["map"][0], R.select_occupancy(occ, 5)[0], "collision_map_display")
    idx, keys = R.select_occupancy(occ, 7, True)
    check(by["surfaces"][0], idx, "collision_map_display")
    for k, ns in enumerate(("collision_surfaces_only", "free_surfaces_only", "unknown_surfaces_only")):
        check(by["separate"][k], idx[keys == k], ns)
    check(by["components"][0], np.arange(64000), "connected_components_display")
    check(by["sdf"][0], np.arange(64000), "sdf_display")
    assert by["sdf_collision"][0]["ns"] == "sdf_display" and int(by["sdf_collision"][0]["points"]) == 8000 + 1 and by["sdf_collision"][0]["colors"] == "0"
    assert [f["ns"] for f in by["unique"]] == [NS + "_3", NS + "_7"] and [f["ns"] for f in by["listed"]] == [NS + "_7", NS + "_3"]
    assert by["tagged"][0]["ns"] == NS and by["tagged"][0]["points"] == "16" and all(f["points"] == "8" for f in by["unique"] + by["listed"])
