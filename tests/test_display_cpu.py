"""tests/display_restated.py against a naive transcription of the same rules (one Python loop per axis, the 26 neighbours one by
one), on grids of at most 6 x 5 x 4, and against hand-built cases.  No GPU."""
import math

import numpy as np
import pytest

import display_restated as R

# (tests/test_gpu_component_surfaces.py OCC_VALUES)
OCC_VALUES = np.array([0.0, 0.25, 0.5, 0.50000006, 0.75, 1.0, -10000.0, np.nan], np.float32)
SHAPES = [(1, 1, 1), (1, 1, 4), (1, 5, 1), (6, 1, 1), (2, 2, 2), (3, 3, 3), (6, 5, 4), (4, 1, 3)]


def _class(o):
    o = float(o)
    if o > 0.5:
        return "F"
    if o < 0.5:
        return "E"
    if o == 0.5:
        return "U"
    return "N"


def _naive_surface(occ, x, y, z):
    nx, ny, nz = occ.shape
    c = _class(occ[x, y, z])
    for xx in range(max(x - 1, 0), min(x + 1, nx - 1) + 1):
        for yy in range(max(y - 1, 0), min(y + 1, ny - 1) + 1):
            for zz in range(max(z - 1, 0), min(z + 1, nz - 1) + 1):
                if (xx, yy, zz) == (x, y, z):
                    continue
                o = _class(occ[xx, yy, zz])
                if c == "E" and o in ("F", "U"):
                    return True
                if c == "F" and o in ("E", "U"):
                    return True
                if c == "U" and o in ("F", "E", "N"):
                    return True
    return False


def _naive(occ, keys, rule, class_mask=7, surface_only=False, draw_keys=None, draw_zero=True):
    nx, ny, nz = occ.shape
    idx, out_keys = [], []
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                ckey = {"F": 0, "E": 1, "U": 2, "N": 2}[_class(occ[x, y, z])]
                in_class = bool((class_mask >> ckey) & 1)
                if rule == "occupancy":
                    key = ckey
                    drawn = in_class and (not surface_only or _naive_surface(occ, x, y, z))
                elif rule == "key":
                    key = int(keys[x, y, z])
                    drawn = (draw_keys is None or key in draw_keys) and (draw_zero or key != 0) and in_class
                else:
                    key = 0
                    drawn = bool(occ[x, y, z] <= 0.0)
                if drawn:
                    idx.append((x * ny + y) * nz + z)
                    out_keys.append(key)
    return np.array(idx, np.uint32), np.array(out_keys, np.uint32)


def _eq(got, want):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("shape", SHAPES)
def test_occupancy_rule_against_the_triple_loop(shape):
    rng = np.random.default_rng(sum(shape) * 7 + len(shape))
    for _ in range(3):
        occ = rng.choice(OCC_VALUES, size=shape)
        for mask in range(8):
            for surf in (False, True):
                _eq(R.select_occupancy(occ, mask, surf), _naive(occ, None, "occupancy", mask, surf))


@pytest.mark.parametrize("shape", SHAPES)
def test_key_rule_against_the_triple_loop(shape):
    rng = np.random.default_rng(sum(shape) * 11)
    occ = rng.choice(OCC_VALUES, size=shape)
    keys = rng.choice(np.array([0, 1, 2, 7, 300, 2 ** 32 - 1], np.uint32), size=shape)
    for draw_keys in (None, [], [7], [0, 2, 300, 2 ** 32 - 1], [5]):
        for draw_zero in (False, True):
            for mask in (7, 1, 6, 0):
                want = _naive(occ, keys, "key", mask, False, draw_keys, draw_zero)
                _eq(R.select_key_field(keys, occ, draw_keys, draw_zero, mask), want)


@pytest.mark.parametrize("shape", SHAPES)
def test_sdf_rule_against_the_triple_loop(shape):
    rng = np.random.default_rng(sum(shape) * 13)
    d = rng.choice(np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 1.5, -2.5, 1e-45, -1e-45], np.float32), size=shape)
    with np.errstate(invalid="ignore"):
        _eq(R.select_sdf(d), _naive(d, None, "sdf"))


def _grid(centre, others=None, fill=np.nan):
    g = np.full((3, 3, 3), fill, np.float32)
    g[1, 1, 1] = centre
    for pos, v in (others or {}).items():
        g[pos] = v
    return g


def test_nan_cells_are_never_a_surface_and_unknown_sees_nan():
    centre = (1 * 3 + 1) * 3 + 1
    # N surrounded by every class: never a surface
    g = _grid(np.nan, {(0, 0, 0): 1.0, (2, 2, 2): 0.0, (0, 1, 1): 0.5})
    assert centre not in R.select_occupancy(g, 7, True)[0]
    # U next to N only: a surface (and drawn with UNKNOWN); the N cells around it are not
    g = _grid(0.5)
    idx, keys = R.select_occupancy(g, 7, True)
    assert idx.tolist() == [centre] and keys.tolist() == [2]
    # F next to N only, E next to N only: not a surface
    for v in (1.0, 0.0):
        assert len(R.select_occupancy(_grid(v), 7, True)[0]) == 0
    # U next to U only: not a surface; F among U: every cell is one (U asks for F, E or N; F asks for E or U)
    g = _grid(0.5, fill=0.5)
    assert len(R.select_occupancy(g, 7, True)[0]) == 0
    g = _grid(1.0, fill=0.5)
    assert len(R.select_occupancy(g, 7, True)[0]) == 27
    # a corner neighbour counts (26-neighbourhood), a cell two steps away does not
    g = np.zeros((3, 3, 4), np.float32)
    g[0, 0, 0] = 1.0
    idx = R.select_occupancy(g, 7, True)[0]
    assert (1 * 3 + 1) * 4 + 1 in idx and (1 * 3 + 1) * 4 + 2 not in idx
    # without surface_only NaN is drawn with UNKNOWN's key
    idx, keys = R.select_occupancy(_grid(np.nan), 4, False)
    assert len(idx) == 27 and set(keys.tolist()) == {2}
    # 0.50000006 is F
    assert R.select_occupancy(np.full((1, 1, 1), 0.50000006, np.float32), 1)[0].tolist() == [0]


def test_grouped_form_is_the_lexsort():
    rng = np.random.default_rng(4)
    for keyset in ([3], [0, 1, 2], [0, 5, 2 ** 32 - 1, 2 ** 31, 70000], []):
        n = 0 if not keyset else 500
        idx = np.sort(rng.choice(5000, size=n, replace=False)).astype(np.uint32)
        keys = rng.choice(np.array(keyset or [0], np.uint32), size=n)
        gi, gk, group_keys, offsets = R.grouped(idx, keys)
        order = np.lexsort((idx, keys))
        assert np.array_equal(gi, idx[order]) and np.array_equal(gk, keys[order])
        assert np.array_equal(group_keys, np.unique(keys))
        assert offsets[0] == 0 and offsets[-1] == n and len(offsets) == len(group_keys) + 1
        for g, k in enumerate(group_keys):
            assert (gk[offsets[g]:offsets[g + 1]] == k).all() and offsets[g + 1] > offsets[g]


def test_points_are_the_cell_centres():
    shape = (3, 4, 5)
    idx = np.arange(60, dtype=np.uint32)
    cells = (0.1, 0.25, 3.0)
    p = R.points(idx, shape, cells)
    for i in range(60):
        x, y, z = i // 20, (i // 5) % 4, i % 5
        assert p[i].tolist() == [0.1 * (x + 0.5), 0.25 * (y + 0.5), 3.0 * (z + 0.5)]
    c = R.table_colors(np.array([0, 2, 3, 2 ** 32 - 1], np.uint32), np.arange(12, dtype=np.float32).reshape(3, 4), (9, 9, 9, 0.5))
    assert c.tolist() == [[0, 1, 2, 3], [8, 9, 10, 11], [9, 9, 9, 0.5], [9, 9, 9, 0.5]]


def test_sdf_colors_on_special_values():
    d = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0, -3.0], np.float32).reshape(1, 1, 7)
    assert R.sdf_extrema(d) == (-math.inf, math.inf)
    c = R.sdf_colors(d, 0.75).reshape(7, 4)
    assert (c[:, 3] == 0.75).all()
    assert c[0].tolist() == [0, 0, 1, 0.75] and c[1].tolist() == [0, 0, 1, 0.75] and c[4].tolist() == [0, 0, 1, 0.75]
    assert np.isnan(c[2, 1]) and c[2, 0] == 0 and c[2, 2] == 0           # inf / inf
    assert np.isnan(c[3, 0]) and c[3, 1] == 0
    assert c[5].tolist() == [0, np.float32(0.2), 0, 0.75] and c[6].tolist() == [np.float32(0.2), 0, 0, 0.75]   # finite / inf = 0
    d = np.array([1.0, 4.0, -2.0, -0.5, 0.0], np.float32).reshape(5, 1, 1)
    assert R.sdf_extrema(d) == (-2.0, 4.0)
    c = R.sdf_colors(d, 7.0).reshape(5, 4)
    assert (c[:, 3] == 1.0).all()
    assert c[0, 1] == np.float32(0.25 * 0.8 + 0.2) and c[1, 1] == np.float32(1.0 * 0.8 + 0.2)
    assert c[2, 0] == np.float32(1.0 * 0.8 + 0.2) and c[3, 0] == np.float32(0.25 * 0.8 + 0.2) and c[4].tolist() == [0, 0, 1, 1]
    assert R.sdf_colors(d, -1.0)[..., 3].max() == 0.0


def test_sdf_colors_on_an_all_zero_field():
    d = np.zeros((2, 3, 4), np.float32)
    assert R.sdf_extrema(d) == (0.0, 0.0)
    c = R.sdf_colors(d, 0.5)                                     # min = max = 0: no voxel divides
    assert (c == np.array([0, 0, 1, 0.5], np.float32)).all()
    assert R.sdf_extrema(np.full((2, 2, 2), np.nan, np.float32)) == (0.0, 0.0)
