"""CPU: the solid fill of closed meshes without a GPU.

  - the exact orientation sign of sdfgpu_mesh_solid.hpp (built for the host, tests/mesh_solid_host.cpp) against fractions.Fraction
    on random inputs and on adversarial ones: near-collinear points at 1 ulp, huge and tiny magnitudes, exact zeros
  - the host text bit-equal to the numpy restatement (mesh_solid_restated.py) on every scene of mesh_solid_cases.py and on 100
    random scenes; once more under -fsanitize=address,undefined (a stand-alone program)
  - the restatement equal to the exact judge (mesh_solid_judge.py); the only cells excused are those mesh_judge calls ambiguous,
    and the scenes are chosen so that there are none; the dyadic scenes with no allowance at all
  - the restatement for a window of columns (inside_at_columns) equal to the whole
  - the merge word by word (mesh_solid_words.py): without a fault it is the parity; with one, every grid of stack_scene on which
    that fault can act gives another bit field than the true one; the cells that stack_scene and slot_scene are built for exist
  - the culling (ms_column_box, ms_tiles; mesh_solid_host cull) against the restatement's coverage over all columns
  - the closedness check; the ABI"""
import ctypes
import functools
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mesh_raster_restated as R
import mesh_solid_cases as SC
import mesh_solid_judge as SJ
import mesh_solid_restated as S
import mesh_solid_words as MW
from sdf_tools_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = SC.cases()
DYADIC = SC.dyadic_cases()
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]


def _build_host(d, extra=()):
    exe = str(d / ("mesh_solid_host" + ("_san" if extra else "")))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unknown-pragmas", *extra, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "sdf_tools_amd", "csrc"), os.path.join(ROOT, "tests", "mesh_solid_host.cpp"), "-o", exe])
    return exe


def _run_orient(exe, d, tag, cases):
    cases = np.ascontiguousarray(cases, np.float64).reshape(-1, 6)
    fin, fout = str(d / ("orient_in%s" % tag)), str(d / ("orient_out%s" % tag))
    with open(fin, "wb") as f:
        f.write(np.array([len(cases)], np.int64).tobytes())
        f.write(cases.tobytes())
    subprocess.check_call([exe, "orient", fin, fout])
    return np.fromfile(fout, np.int8).reshape(-1, 2)


def _run_fill(exe, d, tag, meshes, vertices, triangles, origin, res, grid):
    fin, fout = str(d / ("fill_in%s" % tag)), str(d / ("fill_out%s" % tag))
    meshes = np.ascontiguousarray(meshes, capi.MESH_DTYPE)
    vertices = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    with open(fin, "wb") as f:
        f.write(np.array([len(meshes), len(vertices), len(triangles), *grid], np.int64).tobytes())
        f.write(np.array([res], np.float64).tobytes())
        f.write(np.ascontiguousarray(origin, np.float64).tobytes())
        for a in (meshes, vertices, triangles):
            f.write(a.tobytes())
    subprocess.check_call([exe, "fill", fin, fout])
    raw = open(fout, "rb").read()
    return int(np.frombuffer(raw, np.int64, 1)[0]), np.frombuffer(raw, np.uint32, int(np.prod(grid)), 8).reshape(grid)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_solid_host")
    return _build_host(d), d


# ---- the exact orientation sign --------------------------------------------------------------------------------------------------------
def _exact(row):
    px, py, qx, qy, cx, cy = (Fraction(float(v)) for v in row)
    d = (px - cx) * (qy - cy) - (py - cy) * (qx - cx)
    return (d > 0) - (d < 0)


def orient_inputs():
    rng = np.random.default_rng(11)
    rows = [rng.normal(size=(300, 6)), rng.normal(size=(100, 6)) * 1e150, rng.normal(size=(100, 6)) * 1e-150,
            rng.normal(size=(100, 6)) * 10.0 ** rng.integers(-140, 140, (100, 6))]
    # near-collinear: C on the segment from P to Q up to rounding, then moved by single ulps
    near = []
    for _ in range(400):
        p, q = rng.normal(size=2) * 10.0 ** rng.integers(-3, 4), rng.normal(size=2) * 10.0 ** rng.integers(-3, 4)
        t = rng.random()
        c = p + t * (q - p)
        for _ in range(int(rng.integers(0, 3))):
            k = int(rng.integers(0, 2))
            c[k] = np.nextafter(c[k], rng.choice([-np.inf, np.inf]))
        near.append(np.concatenate([p, q, c]))
    rows.append(np.array(near))
    rows.append(np.array(near) * 2.0 ** 900)
    rows.append(np.array(near) * 2.0 ** -900)
    # exact zeros: collinear lattice points, coincident points, all zero, points on the axes
    zeros = [(0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 5, -3), (1, 2, 3, 4, 1, 2), (0, 0, 4, 6, 2, 3), (0.5, 0.5, 1.5, 1.5, 1e10, 1e10), (3, 0, -7, 0, 1e-300, 0),
             (0.1, 0.1, 0.1, 0.1, 0.1, 0.1), (0, 0, 0.3, 0.9, 0.1, 0.3), (-0.0, 0.0, 1.0, 1.0, 2.0, 2.0), (1e300, 1e300, -1e300, -1e300, 0, 0),
             (5e-324, 0, 0, 5e-324, 0, 0), (1e308, 0, 0, 1e308, 1e308, 1e308)]
    rows.append(np.array(zeros, np.float64))
    p, step = rng.integers(-9, 10, (300, 2)), rng.integers(-4, 5, (300, 2))
    line = np.concatenate([p, p + step * rng.integers(-5, 6, (300, 1)), p + step * rng.integers(-5, 6, (300, 1))], 1).astype(np.float64)
    rows.append(line)                                                        # collinear lattice points: exactly 0
    rows.append(line * 0.375 * 2.0 ** 700)
    ints = rng.integers(-5, 6, (300, 6)).astype(np.float64)
    rows.append(ints)
    rows.append(ints * 0.1)
    return np.concatenate(rows)


def test_the_exact_orientation_sign_equals_fraction(host):
    exe, d = host
    rows = orient_inputs()
    got = _run_orient(exe, d, "", rows)
    want = np.array([_exact(r) for r in rows])
    assert np.array_equal(got[:, 0], want), "expansion arithmetic: %d of %d signs differ" % (int((got[:, 0] != want).sum()), len(rows))
    assert np.array_equal(got[:, 1], want), "filter and fallback: %d of %d signs differ" % (int((got[:, 1] != want).sum()), len(rows))
    assert (want == 0).sum() > 100 and (want > 0).sum() > 300 and (want < 0).sum() > 300
    # the restatement's filter agrees too
    for r in rows[::7]:
        s, _ = S.orient(r[0:2], r[2:4], r[None, 4:6])
        assert s[0] == _exact(r)


# ---- the host text against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES) + list(DYADIC))
def test_the_host_text_is_bit_equal_to_the_restatement(host, name):
    exe, d = host
    scene = (CASES.get(name) or DYADIC[name])
    bad, ids = _run_fill(exe, d, name, *scene)
    _, want, _ = S.restated(*scene)
    assert bad == -1 and np.array_equal(ids, want), (name, int((ids != want).sum()))


def test_the_host_text_is_bit_equal_to_the_restatement_on_random_scenes(host):
    exe, d = host
    cells = inside = 0
    for seed in range(100):
        scene = SC.random_scene(seed)
        bad, ids = _run_fill(exe, d, "r%d" % seed, *scene)
        mask, want, _ = S.restated(*scene)
        surface, _, _ = R.restated(*scene)
        assert bad == -1 and np.array_equal(ids, want), (seed, scene[5], int((ids != want).sum()))
        cells += mask.size
        inside += int(mask.sum()) - int(surface.sum())
    assert cells > 20000 and inside > 500, (cells, inside)


def test_the_host_text_is_clean_under_the_sanitizers(tmp_path):
    """a stand-alone program: AddressSanitizer and UndefinedBehaviorSanitizer on the predicate text"""
    exe = _build_host(tmp_path, SANITIZE)
    rows = orient_inputs()
    got = _run_orient(exe, tmp_path, "san", rows)
    assert np.array_equal(got[:, 0], np.array([_exact(r) for r in rows]))
    for name in ("torus", "poking-out-of-all-faces", "cube-in-cube-one-mesh", "outside"):
        bad, ids = _run_fill(exe, tmp_path, name, *CASES[name])
        assert bad == -1 and np.array_equal(ids, S.restated(*CASES[name])[1])
    singular = np.eye(4)
    singular[2, 2] = 0.0
    assert _run_fill(exe, tmp_path, "singular", *CASES["torus"][:3], singular, 0.05, (3, 3, 3))[0] == -2
    for k, (G, res, nx, ny) in enumerate(cull_edge_inputs()):
        _check_cull(exe, tmp_path, "san%d" % k, G, res, nx, ny)
    _check_cull(exe, tmp_path, "san-slot", _grid_triangles(SC.slot_scene()), SC.RES, *SC.SLOT_GRID[:2])


@pytest.mark.parametrize("name", ["slot-" + v for v in SC.SLOT_VARIANTS] + ["stack-%d" % g[2] for g in SC.STACK_GRIDS if g[2] <= 530])
def test_the_host_text_is_bit_equal_to_the_restatement_on_the_slot_and_stack_scenes(host, name):
    exe, d = host
    scene = SC.slot_scene(name[5:]) if name.startswith("slot-") else SC.stack_scene((12, 6, int(name[6:])))
    bad, ids = _run_fill(exe, d, name, *scene)
    want = _restated(name)[1]
    assert bad == -1 and np.array_equal(ids, want), (name, int((ids != want).sum()))


# ---- the windowed restatement ------------------------------------------------------------------------------------------------------------
def _mesh_triangles(scene):
    """the world triangles [n, 3, 3] of every record that has some, in record order"""
    meshes, vertices, triangles = scene[:3]
    return [W for W in (R.world_triangles([m], vertices, triangles)[1] for m in meshes) if len(W)]


@pytest.mark.parametrize("name", list(CASES))
def test_the_windowed_parity_equals_the_whole(name):
    scene = CASES[name]
    origin, res, (nx, ny, nz) = scene[3:]
    for W in _mesh_triangles(scene):
        whole = S.parity_of(W, origin, res, (nx, ny, nz))
        assert np.array_equal(S.inside_at_columns(W, origin, res, (nx, ny, nz), np.arange(nx), np.arange(ny)), whole)
        toggles = S.toggles_of(W, origin, res, (nx, ny, nz))
        assert toggles.shape == (nx, ny, nz + 1) and not (toggles.sum(2) & 1).any(), "every column is crossed an even number of times"
        for xs, ys in (([nx // 2], [ny // 3]), (np.arange(nx // 3, nx - 2), np.arange(1, ny // 2 + 1)), ([nx - 1, 0, 3], [ny - 1, 2, 0, 5])):
            got = S.inside_at_columns(W, origin, res, (nx, ny, nz), xs, ys)
            assert got.shape == (len(xs), len(ys), nz) and np.array_equal(got, whole[np.ix_(xs, ys)]), (name, xs, ys)


# ---- the word model: the scenes tell a faulty merge from the truth -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _named(name):
    kind, _, arg = name.partition("-")
    return {"stack": lambda: SC.stack_scene((12, 6, int(arg))), "slot": lambda: SC.slot_scene(arg),
            "grid": lambda: SC.grid_scene(tuple(int(v) for v in arg.split("x")))}[kind]()


@functools.lru_cache(maxsize=None)
def _restated(name):
    return S.restated(*_named(name))


@functools.lru_cache(maxsize=None)
def _toggles(name):
    scene = _named(name)
    return [S.toggles_of(W, *scene[3:]) for W in _mesh_triangles(scene)]


WORD_SCENES = ["stack-%d" % nz for nz in SC.STACK_NZ] + ["slot-trailing"] + ["grid-" + "x".join(map(str, g)) for g in SC.GRIDS]


@pytest.mark.parametrize("name", WORD_SCENES)
def test_the_word_model_without_a_fault_is_the_parity(name):
    nz = _named(name)[5][2]
    for toggles in _toggles(name):
        parity = (np.cumsum(toggles[:, :, :nz], axis=2) & 1).astype(np.uint8)
        assert np.array_equal(MW.parity_bits(toggles), S.pack_bits(parity)), name
    # and the union with the surface is the whole result
    bits = R.restated(*_named(name))[2].copy()
    for toggles in _toggles(name):
        bits |= MW.parity_bits(toggles)
    assert np.array_equal(bits, _restated(name)[2])


def fault_can_act(fault, grid):
    nx, ny, nz = grid
    sh = (np.arange(nx * ny, dtype=np.int64) * nz) & 31                        # where each column starts within a word
    shifted = bool(sh.any())
    # The spill word holds cells of the column only where the last word's nz % 32 bits, moved up by sh, pass bit 31.  sh is a multiple
    # of gcd(nz, 32), so on nz = 130, 1000, 2081 and 4100 (nz % 32 = 2, 8, 1, 4) no column has one: there the kernel's spill store
    # never runs with a bit to write, and no scene on that grid can tell a merge without it from the truth.
    spills = bool((nz % 32 + sh > 32).any())
    return {"no-chunk-carry": nz > 2048, "no-prev-across-chunks": nz > 2048 and shifted, "no-word-carry": (nz + 31) // 32 >= 2,
            "no-tail-mask": nz % 32 != 0, "no-spill-word": shifted and spills}[fault]


@pytest.mark.parametrize("fault", MW.FAULTS)
@pytest.mark.parametrize("nz", SC.STACK_NZ)
def test_every_stack_grid_tells_every_fault_that_can_act_from_the_truth(nz, fault):
    """the faulty model's parity bits ORed with the surface bits against the true bit field: they differ wherever the fault can act
    (so a kernel with that fault fails test_gpu_mesh_solid.py on that grid), and are the truth where it cannot"""
    name = "stack-%d" % nz
    bits = R.restated(*_named(name))[2].copy()
    for toggles in _toggles(name):
        bits |= MW.parity_bits(toggles, fault)
    assert np.array_equal(bits, _restated(name)[2]) != fault_can_act(fault, (12, 6, nz)), (name, fault)


def test_the_stack_grids_take_every_path_of_the_merge():
    groups, full, over = set(), set(), set()
    for nz in SC.STACK_NZ:
        wz = (nz + 31) // 32
        group = min(64, 1 << (wz - 1).bit_length())
        groups.add(group)
        (full if wz % group == 0 else over).add(group)
    assert groups == {1, 2, 4, 8, 16, 32, 64} and full >= {1, 2, 8, 16, 32, 64} and over >= {4, 8, 16, 32, 64}
    assert {(nz + 31) // 32 for nz in SC.STACK_NZ} >= {64, 66, 129} and any(nz % 32 == 0 for nz in SC.STACK_NZ)
    assert SC.stack_boundaries(4128) == [2048, 4096] and SC.stack_boundaries(2081) == [1056, 2048] and SC.stack_boundaries(32) == []


@pytest.mark.parametrize("nz", SC.STACK_NZ)
def test_the_stack_scene_has_its_cells_at_every_boundary(nz):
    """from the restatement alone: at every boundary B some column of P has cells B - 1 and B inside by parity and met by no probe; some
    column of Q has cells B - 8 and B + 9 likewise and cells B - 1 and B empty in the whole scene; P's parity is 1 where the column ends"""
    name = "stack-%d" % nz
    scene = _named(name)
    mask = _restated(name)[0].astype(bool)
    surface = R.restated(*scene)[0].astype(bool)
    p, q = ((np.cumsum(t[:, :, :nz], axis=2) & 1).astype(bool) & ~surface for t in _toggles(name)[:2])
    assert [int(m["object_id"]) for m in scene[0]] == [4, 2, 7]
    assert p[:, :, nz - 1].any(), "no column of P is inside, by parity alone, at the last cell"
    assert not q[:, :, nz - 1].any() and not q[:, :, 0].any()
    for b in SC.stack_boundaries(nz):
        assert (p[:, :, b - 1] & p[:, :, b]).any(), (nz, b)
        assert (q[:, :, b - 8] & q[:, :, b + 9] & ~mask[:, :, b - 1] & ~mask[:, :, b]).any(), (nz, b)
    assert int(mask.sum()) > int(surface.sum()) + 10 * nz


def test_the_slot_scene_is_laid_out_against_the_work_distribution(host):
    exe, d = host
    for variant in SC.SLOT_VARIANTS:
        meshes, vertices, triangles, origin, res, grid = SC.slot_scene(variant)
        counts = [int(m["n_triangles"]) for m in meshes]
        assert counts[:6] == [1280, 0, 12, 0, 12, 24] and sum(counts[:6]) == 1328 and capi.check_closed_meshes(meshes, vertices, triangles) is None
        assert R.mesh_refusal(meshes, vertices, triangles) is None
        if variant == "trailing":
            assert len(triangles) == 1328 + 40 and len(meshes) == 6
        else:
            assert len(meshes) == 7 and all(int(meshes[6][k]) == int(meshes[5][k]) for k in ("first_triangle", "n_triangles", "first_vertex", "n_vertices"))
            assert int(meshes[6]["object_id"]) < int(meshes[5]["object_id"]) and sum(counts) <= len(triangles)
        tiles = _run_cull(exe, d, "slot-" + variant, _grid_triangles((meshes, vertices, triangles, origin, res, grid)), res, grid[0], grid[1])[:, 6]
        first = np.concatenate([[0], np.cumsum(counts)])
        assert (tiles[:1280] > 0).sum() > 1024 and (tiles[1024:1280] > 0).any(), "slots with work past the first scan block of 1024"
        assert not tiles[first[2]:first[3]].any(), "the box outside: every slot has zero tiles"
        assert (tiles[first[4]:first[5]] == 25).any(), "the slab: more tiles in a slot than a chunk of 16 holds"
        six = tiles[first[5]:first[6]]
        inner = np.flatnonzero(six > 0)
        assert len(inner) == 12 and (np.diff(inner) > 1).sum() >= 3, "zero-tile slots between the others"
        mask = _restated("slot-" + variant)[0]
        # (the flattened icosahedron stands over some 2400 columns, most with a cell between the probes of its two sheets)
        assert int(mask.sum()) > int(R.restated(meshes, vertices, triangles, origin, res, grid)[0].sum()) + 2000


# ---- the culling -----------------------------------------------------------------------------------------------------------------------
def _grid_triangles(scene):
    """every triangle of the scene in grid coordinates: [n, 3, 3]"""
    meshes, vertices, triangles, origin = scene[:4]
    W = R.world_triangles(meshes, vertices, triangles)[1]
    return S.grid_vertices(S.inverse(origin), origin, W)


def _run_cull(exe, d, tag, G, res, nx, ny):
    """int64 [n, 7]: lo[0], lo[1], hi[0], hi[1], per[0], per[1], count"""
    G = np.ascontiguousarray(G, np.float64).reshape(-1, 9)
    fin, fout = str(d / ("cull_in%s" % tag)), str(d / ("cull_out%s" % tag))
    with open(fin, "wb") as f:
        f.write(np.array([len(G), nx, ny], np.int64).tobytes())
        f.write(np.array([res], np.float64).tobytes())
        f.write(G.tobytes())
    subprocess.check_call([exe, "cull", fin, fout])
    return np.fromfile(fout, np.int64).reshape(-1, 7)


def _reach(gmin, gmax, res, n):
    """the columns k of an axis with t_min - 1 <= k + 1/2 <= t_max + 1, t = g / res as a double, compared exactly: those whose centres lie
    within the triangle's extent, one column further each way (sdfgpu_mesh_solid.hpp "culling").  None: there is none."""
    t0, t1 = Fraction(float(np.float64(gmin) / np.float64(res))), Fraction(float(np.float64(gmax) / np.float64(res)))
    lo, hi = max(0, math.ceil(t0 - Fraction(3, 2))), min(n - 1, math.floor(t1 + Fraction(1, 2)))
    return (lo, hi) if lo <= hi else None


def _check_cull(exe, d, tag, G, res, nx, ny):
    """ms_column_box and ms_tiles of every triangle G [n, 3, 3] (grid coordinates) against the restatement's coverage over ALL columns:
    every covered column lies in the box; the box holds every column within reach and is clipped to the grid; it is empty (lo > hi on
    an axis) exactly when an axis has no column within reach; count is the product of per, per the 16-column tiles of the box.
    Returns (triangles with an empty box, covered columns seen)"""
    G = np.asarray(G, np.float64).reshape(-1, 3, 3)
    out = _run_cull(exe, d, tag, G, res, nx, ny)
    assert len(out) == len(G)
    X, Y = (a.reshape(-1) for a in np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"))
    C = np.stack([res * (X.astype(np.float64) + 0.5), res * (Y.astype(np.float64) + 0.5)], 1)
    empty = seen = 0
    for j, (g, row) in enumerate(zip(G, out.tolist())):
        lo, hi, per, count = row[0:2], row[2:4], row[4:6], row[6]
        covered, _ = S.crossing([[float(v) for v in r] for r in g], C)
        seen += int(covered.sum())
        reach = [_reach(g[:, k].min(), g[:, k].max(), res, n) for k, n in ((0, nx), (1, ny))]
        assert count == per[0] * per[1] and all(per[k] == (0 if hi[k] < lo[k] else (hi[k] - lo[k]) // 16 + 1) for k in range(2)), (tag, j, row)
        for k, n in ((0, nx), (1, ny)):
            assert (lo[k] > hi[k]) == (reach[k] is None), (tag, j, k, row, reach)
            if reach[k] is not None:
                assert 0 <= lo[k] <= reach[k][0] and reach[k][1] <= hi[k] <= n - 1, (tag, j, k, row, reach)
        if count == 0:
            empty += 1
            assert not covered.any(), (tag, j, row)
        else:
            assert ((X[covered] >= lo[0]) & (X[covered] <= hi[0]) & (Y[covered] >= lo[1]) & (Y[covered] <= hi[1])).all(), (tag, j, row)
    return empty, seen


def cull_edge_inputs():
    """[(G [n, 3, 3], res, nx, ny)]: triangles with a vertex exactly on the centre of column 0 and of column n - 1, triangles one column
    outside each side of the grid (within reach of the outermost column, and just out of it), and grid coordinates of +-1e300"""
    out = []
    for res in (1e-3, 0.05, 7.0):
        nx, ny = 9, 7
        first, last = (res * 0.5, res * 0.5), (res * (nx - 0.5), res * (ny - 0.5))
        rows = [[(*first, 0.0), (res * 3.3, res * 1.2, 1.0), (res * 1.1, res * 4.4, 2.0)],          # a vertex on the centre of column (0, 0)
                [(*last, 0.0), (res * 3.3, res * 1.2, 1.0), (res * 1.1, res * 4.4, 2.0)],           # ... of column (nx - 1, ny - 1)
                [(*first, 0.0), (*last, 1.0), (first[0], last[1], 2.0)], [(*first, 0.0), (*last, 1.0), (last[0], first[1], 2.0)],
                [(*first, 0.0), (res * -2.0, res * 0.5, 0.0), (res * 0.5, res * -3.0, 0.0)],        # the centre of column 0 is its only column
                [(*last, 0.0), (res * (nx + 2.0), last[1], 0.0), (last[0], res * (ny + 3.0), 0.0)]]
        for axis in range(2):
            n = (nx, ny)[axis]
            for a, b in ((-0.9, -0.6), (-0.4, -0.1), (n + 0.1, n + 0.4), (n + 0.6, n + 0.9), (-1.4, -1.1), (n + 1.1, n + 1.4)):
                tri = np.array([(a, 2.2, 0.0), (b, 3.1, 1.0), (0.5 * (a + b), 5.7, 2.0)]) * res
                rows.append(tri[:, [1, 0, 2]] if axis else tri)
        big = 1e300
        rows += [[(-big, -big, 0.0), (big, -big, 1.0), (0.0, big, 2.0)], [(big, big, 0.0), (big, 0.9 * big, 1.0), (0.9 * big, big, 2.0)],
                 [(-big, res * 2.2, 0.0), (big, res * 2.4, 1.0), (res, res * 4.9, big)], [(-big, -big, -big), (-big, res, big), (res, -big, 0.0)]]
        out.append((np.array(rows, np.float64), res, nx, ny))
    return out


def test_the_culling_keeps_every_covered_column(host):
    exe, d = host
    scenes = {**CASES, **DYADIC, **{"slot-" + v: SC.slot_scene(v) for v in SC.SLOT_VARIANTS}, **{"stack-%d" % g[2]: SC.stack_scene(g) for g in SC.STACK_GRIDS}}
    scenes.update({"random-%d" % seed: SC.random_scene(seed) for seed in range(200)})
    scenes.update({"tall-%d" % seed: SC.random_tall_scene(seed) for seed in range(12)})
    triangles = empty = seen = 0
    for name, scene in scenes.items():
        G = _grid_triangles(scene)
        e, s = _check_cull(exe, d, name, G, scene[4], scene[5][0], scene[5][1])
        triangles, empty, seen = triangles + len(G), empty + e, seen + s
    print("%d triangles, %d with an empty box, %d covered columns" % (triangles, empty, seen))
    # (the slab's two faces of 63 x 61 columns and the two sheets of the flattened icosahedron, in both slot scenes, are 24 000 alone)
    assert triangles > 10000 and empty > 100 and seen > 20000


def test_the_culling_at_the_edges_of_the_grid_and_of_the_doubles(host):
    exe, d = host
    for k, (G, res, nx, ny) in enumerate(cull_edge_inputs()):
        empty, seen = _check_cull(exe, d, "edge%d" % k, G, res, nx, ny)
        assert empty >= 5 and seen > 0
        out = _run_cull(exe, d, "edge%d" % k, G, res, nx, ny)
        assert out[0, 0] == 0 and out[0, 1] == 0 and out[1, 2] == nx - 1 and out[1, 3] == ny - 1
        assert out[-4].tolist() == [0, 0, nx - 1, ny - 1, 1, 1, 1], "a triangle over +-1e300 reaches every column"

# ---- the restatement against the exact judge -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_exact_judge(name):
    meshes, vertices, triangles, origin, res, grid = CASES[name]
    mask, _, _ = S.restated(meshes, vertices, triangles, origin, res, grid)
    surface, _, _ = R.restated(meshes, vertices, triangles, origin, res, grid)
    judged, ambiguous = SJ.check(mask, *SJ.verdict(meshes, vertices, triangles, origin, res, grid))
    print("%s: %d filled (%d by the surface) of %d judged, %d ambiguous" % (name, int(mask.sum()), int(surface.sum()), judged, ambiguous))
    assert ambiguous == 0, "the scene was chosen to have no cell the surface judge calls ambiguous"
    assert not (surface & ~mask).any()
    if name == "outside":
        assert not mask.any()
    elif name == "cube-in-cube-one-mesh":
        c = tuple(int(v) for v in np.round(np.asarray(grid) * np.array([0.47, 0.553, 0.46]) - 0.5))
        assert not mask[c], "the hollow"
        assert int(mask.sum()) > int(surface.sum())
    elif name == "two-overlapping":
        one = [S.restated(meshes[i:i + 1], vertices, triangles, origin, res, grid)[0] for i in range(2)]
        assert np.array_equal(mask, one[0] | one[1]) and (one[0] & one[1]).any(), "a union, not an XOR"
    elif name == "poking-out-of-all-faces":
        assert mask.all()
    else:
        assert int(mask.sum()) > int(surface.sum()), "no interior cell: the scene tests nothing"
    if "flipped" in name or name == "soup":
        assert np.array_equal(mask, S.restated(*CASES["icosahedron-generic"])[0]), "orientation and vertex sharing play no part"


@pytest.mark.parametrize("name", list(DYADIC))
def test_dyadic_box_resolves_every_tie_consistently(name):
    meshes, vertices, triangles, origin, res, grid = DYADIC[name]
    mask, _, _ = S.restated(meshes, vertices, triangles, origin, res, grid)
    ratio, inside, on_surface = SJ.verdict(meshes, vertices, triangles, origin, res, grid)
    SJ.check(mask, ratio, inside, on_surface, ties_as_hits=True)             # no allowance: every cell, ties counted as hits
    assert int(on_surface.sum()) > 50, "centres exactly on the faces: the scene has its ties"
    want = np.zeros(grid, bool)
    want[1:7, 2:6, 1:6] = True                                               # centres 0.1875 .. 0.8125, 0.3125 .. 0.6875, 0.1875 .. 0.6875
    assert np.array_equal(mask.astype(bool), want), "no streak along z, no cell lost on the outline"


# ---- the closedness check --------------------------------------------------------------------------------------------------------------
def test_closed_meshes_pass():
    eye = np.eye(4)
    ico, tor = SC.icosahedron(1.0), SC.torus(2.0, 0.5)
    items = [(1, *ico, eye), (2, *tor, SC._local(SC.GENERIC_Q, (0.3, -2.0, 5.0))), (3, *SC.soup(*ico), SC._local(SC.GENERIC_Q, (1.0, 2.0, 3.0))),
             (4, *SC.subdivide(*tor), eye), (5, *SC.joined([SC.box_triangles((1, 2, 3)), SC.box_triangles((0.1, 0.2, 0.3))]), eye),
             (6, ico[0], SC.flipped(ico[1], np.arange(0, 20, 3)), eye), (7, np.zeros((0, 3)), np.zeros((0, 3), np.uint32), eye)]
    assert capi.check_closed_meshes(*capi.make_meshes(items)) is None
    # -0 and 0 are one position
    v, t = SC.soup(*SC.box_triangles((2.0, 2.0, 2.0)))
    v = v + 1.0                                                              # corners at 0 and 2
    v[::2][v[::2] == 0.0] = -0.0
    assert capi.check_closed_meshes(*capi.make_meshes([(1, v, t, eye)])) is None


def test_zero_area_triangles_do_not_open_a_mesh():
    v, t = SC.icosahedron(1.0)
    # a T-junction closed by the zero-area triangle that fills it: the edge (a, b) of one triangle is split at its midpoint
    a, b, c = (int(i) for i in t[0])
    v2 = np.vstack([v, 0.5 * (v[a] + v[b])])
    m = len(v)
    t2 = np.vstack([t[1:], [(a, m, c), (m, b, c), (a, b, m)], [(a, a, b), (c, c, c)]]).astype(np.uint32)
    assert capi.check_closed_meshes(*capi.make_meshes([(1, v2, t2, np.eye(4))])) is None
    assert capi.check_closed_meshes(*capi.make_meshes([(1, v2, t2[:-3], np.eye(4))])) is not None, "without it: a T-junction"


def test_open_meshes_are_refused_with_mesh_and_triangle():
    eye = np.eye(4)
    v, t = SC.icosahedron(1.0)
    good = (1, v, t, eye)
    # triangle 7 removed: its three neighbours have an edge used once; the lowest of them is reported
    removed = np.delete(t, 7, 0)
    gone = {frozenset((int(t[7][i]), int(t[7][(i + 1) % 3]))) for i in range(3)}
    first = min(j for j, tri in enumerate(removed) if any(frozenset((int(tri[i]), int(tri[(i + 1) % 3]))) in gone for i in range(3)))
    assert capi.check_closed_meshes(*capi.make_meshes([good, (2, v, removed, eye)])) == (1, first)
    # a T-junction: one triangle's edge split at its midpoint, the neighbour's not
    a, b, c = (int(i) for i in t[3])
    users = [j for j, tri in enumerate(t) if {a, b} <= {int(i) for i in tri}]  # the two triangles on edge (a, b): 3 and its neighbour
    assert len(users) == 2 and 3 in users
    v2 = np.vstack([v, 0.5 * (v[a] + v[b])])
    t2 = t.copy().tolist()
    t2[3] = (a, len(v), c)
    t2.append((len(v), b, c))
    # odd edges: (a, b) of the neighbour, (a, m) of triangle 3, (m, b) of triangle 20: the lowest of 3 and the neighbour is reported
    assert capi.check_closed_meshes(*capi.make_meshes([good, good, (3, v2, np.array(t2, np.uint32), eye)])) == (2, min(users))
    # an edge used three times: a fin on edge (a, b)
    v3 = np.vstack([v, 2.0 * (v[a] + v[b])])
    t3 = np.vstack([t, [(a, b, len(v))]]).astype(np.uint32)
    # edge (a, b) has a run of three records, of triangles min(users), max(users) and 20, and the fin's other two edges one each (20):
    # the run's lowest triangle is the answer, whichever order the triangles come in
    assert capi.check_closed_meshes(*capi.make_meshes([(1, v3, t3, eye), good])) == (0, min(users))
    order = np.r_[20, np.arange(19, -1, -1)]                                   # the fin first, the others reversed
    lowest = min(int(np.flatnonzero(order == j)[0]) for j in users + [20])
    assert lowest == 0 and capi.check_closed_meshes(*capi.make_meshes([good, (1, v3, t3[order], eye)])) == (1, 0)
    fin_last_users_late = np.r_[[j for j in range(20) if j not in users], users[::-1], 20]
    assert capi.check_closed_meshes(*capi.make_meshes([(1, v3, t3[fin_last_users_late], eye)])) == (0, 18)
    # a refused record, a vertex index out of range
    meshes, vv, tt = capi.make_meshes([good, good])
    meshes = meshes.copy()
    meshes["n_triangles"][1] = 21
    assert capi.check_closed_meshes(meshes, vv, tt) == (1, -1)
    t4 = t.copy()
    t4[5, 1] = 12
    assert capi.check_closed_meshes(*capi.make_meshes([good, (2, v, t4, eye)])) == (1, 5)


def test_the_closedness_check_is_not_quadratic():
    import time
    v, t = SC.torus(2.0, 0.5, 300, 200)                                      # 120 000 triangles
    t0 = time.time()
    assert capi.check_closed_meshes(*capi.make_meshes([(1, v, t, np.eye(4))])) is None
    assert time.time() - t0 < 5.0


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_exported_and_declared():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "sdfgpu.h")).read()
    for name in ("sdfgpu_rasterize_solid_meshes_device", "sdfgpu_rasterize_solid_meshes", "sdfgpu_check_closed_meshes"):
        assert name in capi.EXPORTS and hasattr(lib, name)
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert re.search(r"^#define SDFGPU_MAX_SOLID_MESHES %d$" % capi.MAX_SOLID_MESHES, header, re.M)
    data = open(os.path.join(ROOT, "sdf_tools_amd", "libsdfgpu.so"), "rb").read()
    for kernel in (b"k_ms_setup", b"k_ms_scatter", b"k_ms_merge"):
        assert kernel in data, kernel
    for method in ("rasterize_solid_meshes", "rasterize_solid_meshes_device"):
        assert hasattr(capi.SdfGpu, method)


def test_arguments_are_refused_before_a_device_is_needed():
    lib = capi.load_library()
    origin = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    out = (ctypes.c_uint32 * 4)()
    assert lib.sdfgpu_rasterize_solid_meshes(None, None, 0, None, 0, None, 0, origin, 0.1, 2, 2, 2, out, None, None) == -1
    assert lib.sdfgpu_rasterize_solid_meshes_device(None, None, 0, None, 0, None, 0, origin, 0.1, 2, 2, 2, out, None, None, 0, None, None) == -1
    assert lib.sdfgpu_check_closed_meshes(None, -1, None, 0, None, 0, None, None) != 0
    assert lib.sdfgpu_check_closed_meshes(None, 0, None, 0, None, 0, None, None) == 0


# ---- the C++ layer ---------------------------------------------------------------------------------------------------------------------
def test_the_solid_example_compiles():
    from sdf_tools_amd import build
    assert os.path.exists(build.build_example("sdf_builder_solid", force=True))            # -Wall -Wextra, against include/ and the in-tree library


@pytest.mark.parametrize("sanitized", [False, True])
def test_sdf_builder_solid_exceptions_in_a_stand_alone_program(tmp_path, sanitized):
    """tests/sdf_builder_solid_exceptions.cpp: an open mesh under MESH_FILL_SOLID is refused by name before the GPU is touched; once
    more under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program)"""
    exe = str(tmp_path / "sdf_builder_solid_exceptions")
    pkg = os.path.join(ROOT, "sdf_tools_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-DSDF_TOOLS_VECTOR_ADOPT", *(SANITIZE if sanitized else []),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sdf_builder_solid_exceptions.cpp"), "-o", exe,
                           "-L", pkg, "-lsdfgpu", "-Wl,-rpath," + pkg, "-lz"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert out.stdout.count("ok   ") >= 7


def test_pysdf_tools_binds_the_mesh_fill_modes():
    from sdf_tools_amd._bindings import load_pysdf_tools
    m = load_pysdf_tools()
    assert m.MESH_FILL_SURFACE == 0 and m.MESH_FILL_SOLID == 1
    for name in ("SetMeshFill", "SetObjectMeshFill"):
        assert hasattr(m.SDF_Builder, name), name
