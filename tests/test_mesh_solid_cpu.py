"""CPU: the solid fill of closed meshes without a GPU.

  - the exact orientation sign of sdfgpu_mesh_solid.hpp (built for the host, tests/mesh_solid_host.cpp) against fractions.Fraction
    on random inputs and on adversarial ones: near-collinear points at 1 ulp, huge and tiny magnitudes, exact zeros
  - the host text bit-equal to the numpy restatement (mesh_solid_restated.py) on every scene of mesh_solid_cases.py and on 100
    random scenes; once more under -fsanitize=address,undefined (a stand-alone program)
  - the restatement equal to the exact judge (mesh_solid_judge.py); the only cells excused are those mesh_judge calls ambiguous,
    and the scenes are chosen so that there are none; the dyadic scenes with no allowance at all
  - the closedness check; the ABI"""
import ctypes
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
