"""TaggedObjectCollisionMapGrid::ExportContourOnlyForDisplay and its three kin through pysdf_tools, against a Python loop written as the
reference writes it (tagged_object_collision_map.cpp:917-1180): MakeAllObjectSDFs(True, False) / MakeObjectSDFs(ids, True, False), the
threshold `dist < 0.0 && dist > float(-1.9 * resolution)`, the colour's alpha.  Points and colours bit for bit; the marker fields;
ascending UniqueNs order and pruning; id 0; hidden and missing colour-map ids; alpha <= 0; the exception on non-uniform cells."""
import math
import struct

import numpy as np
import pytest

import display_cases as C
import display_restated as R
from sdf_tools_amd._bindings import load_pysdf_tools

pytestmark = pytest.mark.gpu

SHAPE = (9, 7, 33)
RES = 0.1
CELL = (RES, RES, RES)
ORIGIN = [[0.0, -1.0, 0.0, 1.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.25], [0.0, 0.0, 0.0, 1.0]]
RED, BLUE, NONE = (1.0, 0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 0.25), (0.3, 0.3, 0.3, 0.0)
NS = "tagged_object_collision_map_display"
IDS = (0, 3, 7, 300, 70000)


@pytest.fixture(scope="module")
def m():
    return load_pysdf_tools()


def _grid(m, occ, objects, res=RES):
    rec = np.zeros(occ.shape + (4,), np.uint32)
    rec[..., 0] = occ.view(np.uint32)
    rec[..., 1] = 0x7B7B7B7B                                        # (component and segment words: not read)
    rec[..., 2] = objects
    rec[..., 3] = 5
    g = m.TaggedObjectCollisionMapGrid(m.Isometry3d(ORIGIN), "display_frame", res, *occ.shape, m.TAGGED_OBJECT_COLLISION_CELL(0.0, 0))
    g.SetRawCellsNumpy(rec.view(np.uint8).reshape(occ.shape + (16,)))
    return g


@pytest.fixture(scope="module")
def scene(m):
    """mostly filled blocks of five ids (interiors that are not drawn), noise occupancies among them, id 70000 in one column only"""
    rng = np.random.default_rng(31)
    occ = np.where(rng.random(SHAPE) < 0.85, np.float32(1.0), rng.choice(C.OCC_VALUES, size=SHAPE)).astype(np.float32)
    objects = np.zeros(SHAPE, np.uint32)
    objects[:5, :, :16], objects[:5, :, 16:], objects[5:, :4, :], objects[5:, 4:, :] = 300, 3, 7, 0
    objects[8, 6, :] = 70000
    occ[8, 6, :] = 1.0
    return _grid(m, occ, objects), occ, objects


def _reference_loop(g, objects, sdfs, color_of):
    """the reference's triple loop, vectorised per object: -> {id: (indices, colour)} of the objects that have an SDF"""
    bdy = np.float32(-1.9 * g.GetResolution())
    out = {}
    for o, sdf in sdfs.items():
        dist = sdf.GetRawDataNumpy()
        drawn = (objects == o) & (dist.astype(np.float64) < 0.0) & (dist > bdy)
        color = color_of(o)
        out[o] = (np.flatnonzero(drawn.reshape(-1)).astype(np.uint32) if color[3] > 0.0 else np.zeros(0, np.uint32), color)
    return out


def _single(per_object):
    """one marker: the drawn cells of all objects in scan order"""
    idx = np.concatenate([v[0] for v in per_object.values()] + [np.zeros(0, np.uint32)])
    col = np.concatenate([np.tile(np.float32(v[1]), (len(v[0]), 1)) for v in per_object.values()] + [np.zeros((0, 4), np.float32)])
    order = np.argsort(idx, kind="stable")
    return idx[order], col[order]


def _same(what, got, idx, colors, shape=SHAPE, cell=CELL):
    pts, col = got
    assert pts.dtype == np.float64 and col.dtype == np.float32, what
    assert pts.tobytes() == R.points(idx, shape, cell).tobytes(), "%s: points differ (%d got, %d expected)" % (what, len(pts), len(idx))
    assert col.tobytes() == np.ascontiguousarray(colors, np.float32).reshape(-1, 4).tobytes(), "%s: colours differ" % what


def _check_unique_ns(what, markers, per_object):
    order = [o for o in sorted(per_object) if len(per_object[o][0])]                      # ascending id; empty markers pruned
    assert [ns for ns, _, _ in markers] == ["%s_%d" % (NS, o) for o in order], what
    for o, (ns, pts, col) in zip(order, markers):
        _same("%s, %s" % (what, ns), (pts, col), per_object[o][0], np.tile(np.float32(per_object[o][1]), (len(per_object[o][0]), 1)))
    return order


def test_alpha_forms(m, scene):
    g, occ, objects = scene
    gen = m.TaggedObjectCollisionMapGrid.GenerateComponentColor
    for alpha, draw in ((1.0, []), (0.5, [7]), (0.5, [70000, 3, 0, 11]), (0.25, [300, 3]), (0.5, [11])):
        sdfs = g.MakeObjectSDFs(draw, True, False) if draw else g.MakeAllObjectSDFs(True, False)
        assert sorted(sdfs) == (sorted(set(draw)) if draw else [3, 7, 300, 70000])
        per_object = _reference_loop(g, objects, sdfs, lambda o: gen(o, alpha))
        idx, col = _single(per_object)
        assert (len(idx) > 0) == (draw != [11])
        _same("ExportContourOnlyForDisplay(%s, %s)" % (alpha, draw), g.ExportContourOnlyForDisplay(alpha, draw), idx, col)
        order = _check_unique_ns("UniqueNs(%s, %s)" % (alpha, draw), g.ExportContourOnlyForDisplayUniqueNs(alpha, draw), per_object)
        assert 0 not in order and order == sorted(order)
        if not draw:
            assert order == [3, 7, 300, 70000]
            filled = (occ >= 0.5)
            assert len(idx) < int((filled & (objects != 0)).sum()), "interiors are not drawn"
            assert not np.isin(idx, np.flatnonzero((objects == 0).reshape(-1))).any(), "id 0 is never drawn"
    # the defaults are the reference's: alpha 1, every object
    a, b = g.ExportContourOnlyForDisplay(), g.ExportContourOnlyForDisplay(1.0, [])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[0]) > 0
    assert [ns for ns, _, _ in g.ExportContourOnlyForDisplayUniqueNs()] == ["%s_%d" % (NS, o) for o in (3, 7, 300, 70000)]
    for alpha in (0.0, -1.0, float("nan")):
        pts, col = g.ExportContourOnlyForDisplay(alpha)
        assert pts.shape == (0, 3) and col.shape == (0, 4)
        assert g.ExportContourOnlyForDisplayUniqueNs(alpha, [3]) == []


def test_color_map_forms(m, scene):
    g, occ, objects = scene
    gen = m.TaggedObjectCollisionMapGrid.GenerateComponentColor
    sdfs = g.MakeAllObjectSDFs(True, False)
    assert sorted(sdfs) == [3, 7, 300, 70000]
    for cmap in ({}, {7: RED, 300: NONE}, {0: RED, 70000: BLUE, 11: RED}, {3: NONE, 7: NONE, 300: NONE, 70000: NONE}):
        per_object = _reference_loop(g, objects, sdfs, lambda o: cmap[o] if o in cmap else gen(o))
        idx, col = _single(per_object)
        _same("ExportContourOnlyForDisplay(%s)" % sorted(cmap), g.ExportContourOnlyForDisplay(cmap), idx, col)
        order = _check_unique_ns("UniqueNs(%s)" % sorted(cmap), g.ExportContourOnlyForDisplayUniqueNs(cmap), per_object)
        assert order == [o for o in (3, 7, 300, 70000) if (cmap[o] if o in cmap else gen(o))[3] > 0]
        assert not np.isin(idx, np.flatnonzero((objects == 0).reshape(-1))).any(), "id 0 is never drawn, even when the map makes it visible"
        if 300 in cmap:
            assert 300 not in order and not np.isin(idx, np.flatnonzero((objects == 300).reshape(-1))).any()      # hidden by the map


def test_marker_fields(m, scene):
    g, _, _ = scene
    info = g.ExportContourOnlyForDisplayInfo(0.5)
    assert info["frame_id"] == "display_frame" and info["ns"] == NS
    assert (info["id"], info["type"], info["action"], info["lifetime"], info["frame_locked"]) == (1, 6, 0, 0.0, False)       # CUBE_LIST, ADD
    assert info["position"] == (1.5, -2.0, 0.25) and info["scale"] == (RES, RES, RES)
    assert np.allclose(info["orientation"], (0.0, 0.0, math.sqrt(0.5), math.sqrt(0.5)), atol=1e-15)
    assert info["points"] == info["colors"] == len(g.ExportContourOnlyForDisplay(0.5)[0]) > 0


def test_resolutions_of_every_reach(m):
    """one resolution per reach value: the class takes its reach from GetResolution()"""
    from sdf_tools_amd import capi
    rng = np.random.default_rng(32)
    shape = (6, 7, 8)
    occ = np.where(rng.random(shape) < 0.9, np.float32(1.0), np.float32(0.0)).astype(np.float32)
    objects = np.where(np.arange(6)[:, None, None] < 3, 4, 9).astype(np.uint32) * np.ones(shape, np.uint32)
    counts = []
    for res, reach in ((0.05, 3), (2.0 ** -149, 2), (1.5 * 2.0 ** 127, 1), (2.0 ** -160, 0)):
        assert capi.display_contour_reach(res) == reach
        g = _grid(m, occ, objects, res)
        with np.errstate(over="ignore", under="ignore"):
            per_object = _reference_loop(g, objects, g.MakeAllObjectSDFs(True, False), lambda o: RED)
        idx, col = _single(per_object)
        _same("resolution %g" % res, g.ExportContourOnlyForDisplay({4: RED, 9: RED}), idx, col, shape, (res, res, res))
        counts.append(len(idx))
    assert counts[0] > counts[1] > counts[2] > counts[3] == 0


def test_non_uniform_cells_throw(m, scene):
    g, _, _ = scene
    raw = g.SerializeSelf()
    sizes = struct.pack("<6d", RES, RES, RES, 1.0 / RES, 1.0 / RES, 1.0 / RES)
    at = raw.rfind(sizes)
    assert at > 0
    bad = m.TaggedObjectCollisionMapGrid.Deserialize(raw[:at] + struct.pack("<6d", RES, 2 * RES, RES, 1.0 / RES, 0.5 / RES, 1.0 / RES) + raw[at + 48:])
    assert bad.GetNumXCells() == SHAPE[0]
    want = None
    try:
        bad.MakeObjectSDFs([3], True, False)
    except Exception as e:                                      # noqa: BLE001
        want = e
    assert want is not None and "uniform resolution" in str(want)
    for call in (lambda: bad.ExportContourOnlyForDisplay(1.0, []), lambda: bad.ExportContourOnlyForDisplayUniqueNs(0.5, [3]),
                 lambda: bad.ExportContourOnlyForDisplay({3: RED}), lambda: bad.ExportContourOnlyForDisplayUniqueNs({}),
                 lambda: bad.ExportContourOnlyForDisplay(0.0, [])):
        with pytest.raises(type(want)) as e:
            call()
        assert str(e.value) == str(want)
