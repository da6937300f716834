"""CPU: the mesh rasteriser's and the plane's decision procedure without a GPU.

  - the numpy restatement (mesh_raster_restated.py) against the exact judge (mesh_judge.py) on every scene of mesh_cases.py; the
    share of ambiguous cells is printed per case and capped at frame_judge.AMBIGUITY_CAP; the dyadic contact scenes must equal
    the judge with ties counted as hits, no allowance, and must have contacts
  - cross-checks: the cells of a box given as 12 triangles are among the cells of the same box as a primitive; under an unrotated
    origin no empty cell contains a point sampled on a triangle; zero-area triangles are decided and fill cells
  - the text the kernels compile (sdfgpu_mesh.hpp) built for the host: bit-equal to the restatement, also under
    -fsanitize=address,undefined
  - struct sdfgpu_mesh against capi.MESH_DTYPE; the new symbols exported and declared; a null handle refused
  - tests/sdf_builder_mesh_exceptions.cpp, also under the sanitizers"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import frame_judge
import mesh_cases as MC
import mesh_judge as J
import mesh_raster_restated as R
import scene_raster_restated as SR
from sdf_tools_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = MC.cases()
PLANES = MC.plane_cases()
DYADIC = MC.dyadic_cases()
DYADIC_PLANES = MC.dyadic_plane_cases()
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]


def _build_host_predicate(d, extra=()):
    exe = str(d / ("mesh_predicate_host" + ("_san" if extra else "")))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", *extra, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "sdf_tools_amd", "csrc"), os.path.join(ROOT, "tests", "mesh_predicate_host.cpp"), "-o", exe])
    return exe


def _run_host_predicate(exe, d, tag, meshes, vertices, triangles, shapes, centres, h):
    fin, fout = str(d / ("in%s" % tag)), str(d / ("out%s" % tag))
    meshes = np.ascontiguousarray(meshes, capi.MESH_DTYPE)
    vertices = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    shapes = np.ascontiguousarray(shapes, capi.SHAPE_DTYPE)
    centres = np.ascontiguousarray(centres, np.float64)
    with open(fin, "wb") as f:
        f.write(np.array([len(meshes), len(vertices), len(triangles), len(shapes), len(centres)], np.int64).tobytes())
        f.write(np.array([h], np.float64).tobytes())
        for a in (meshes, vertices, triangles, shapes, centres):
            f.write(a.tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    n = len(centres)
    return (int(np.frombuffer(raw, np.int64, 1)[0]), np.frombuffer(raw, np.uint32, n, 8), np.frombuffer(raw, np.uint32, n, 8 + 4 * n),
            np.frombuffer(raw, np.uint8, len(shapes), 8 + 8 * n))


@pytest.fixture(scope="module")
def host_predicate(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_host")
    exe = _build_host_predicate(d)
    counter = [0]

    def run(meshes, vertices, triangles, shapes, centres, h):
        counter[0] += 1
        return _run_host_predicate(exe, d, counter[0], meshes, vertices, triangles, shapes, centres, h)

    return run


NO_MESH = capi.make_meshes([])
NO_SHAPES = capi.make_shapes([])


# ---- restatement against the exact judge ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_agrees_with_the_exact_judge(name):
    meshes, vertices, triangles, origin, res, grid = CASES[name]
    mask, _, _ = R.restated(meshes, vertices, triangles, origin, res, grid)
    judged, ambiguous = J.check(mask, J.mesh_ratio(meshes, vertices, triangles, origin, res, grid))
    print("%s: %d filled of %d judged, ambiguous share %.5f" % (name, int(mask.sum()), judged, ambiguous / judged))
    assert ambiguous <= frame_judge.AMBIGUITY_CAP * judged, (name, ambiguous, judged)
    if "outside" in name:
        assert not mask.any()
    elif "tiny" not in name and "point" not in name:
        assert 0 < int(mask.sum()) < mask.size
    if name.startswith("floor-64x8x64"):
        layer = mask.reshape(grid).any(axis=(0, 1))
        assert int(layer.sum()) == 1 and mask.reshape(grid)[:, :, layer].all(), "the floor fills exactly one whole z layer"


@pytest.mark.parametrize("name", list(PLANES))
def test_plane_restatement_agrees_with_the_exact_judge(name):
    shapes, origin, res, grid = PLANES[name]
    mask, ids, _ = R.restated_shapes(shapes, origin, res, grid)
    ratio = np.full(mask.size, -np.inf)
    for rec in shapes:
        if int(rec["type"]) == R.PLANE:
            ratio = np.maximum(ratio, J.plane_ratio(rec, origin, res, grid))
        else:
            import scene_judge
            ratio = np.maximum(ratio, scene_judge.ratios(rec, origin, res, grid, np.arange(mask.size)))
    judged, ambiguous = J.check(mask, ratio)
    print("%s: %d filled of %d judged, ambiguous share %.5f" % (name, int(mask.sum()), judged, ambiguous / judged))
    assert ambiguous <= frame_judge.AMBIGUITY_CAP * judged
    if "outside" in name:
        assert not mask.any()
    else:
        assert 0 < int(mask.sum()) < mask.size or min(grid) == 1
    if "plane-and-box" in name:
        assert set(np.unique(ids)) == {0, 2, 4}, "the box comes first in the list and keeps its cells"


@pytest.mark.parametrize("name", list(DYADIC))
def test_dyadic_contact_scenes_equal_the_judge_with_ties_as_hits(name):
    meshes, vertices, triangles, origin, res, grid = DYADIC[name]
    mask, _, _ = R.restated(meshes, vertices, triangles, origin, res, grid)
    ratio = J.mesh_ratio(meshes, vertices, triangles, origin, res, grid)
    J.check(mask, ratio, ties_only=True)
    assert int((ratio == 0).sum()) > 0, "the scene has no contact: it tests nothing"
    # a triangle lying in the face z = 0.5 = 4 res fills the layers on both sides of it
    assert mask[:, :, 3].any() and mask[:, :, 4].any()


@pytest.mark.parametrize("name", list(DYADIC_PLANES))
def test_dyadic_plane_in_a_voxel_face_fills_both_layers(name):
    shapes, origin, res, grid = DYADIC_PLANES[name]
    mask, _, _ = R.restated_shapes(shapes, origin, res, grid)
    ratio = J.plane_ratio(shapes[0], origin, res, grid)
    J.check(mask, ratio, ties_only=True)
    assert int((ratio == 0).sum()) == 2 * grid[0] * grid[1]
    assert mask[:, :, 3:5].all() and int(mask.sum()) == 2 * grid[0] * grid[1]


# ---- cross-checks --------------------------------------------------------------------------------------------------------------------
def test_zero_area_triangles_are_decided_and_fill_their_cells():
    """an axis that degenerates to 0 never separates: a segment and a point given as triangles fill the cells they pass through"""
    for name, (meshes, vertices, triangles, origin, res, grid) in CASES.items():
        if name.split("-")[0] in ("segment", "point") and name.endswith("identity"):
            mask, _, _ = R.restated(meshes, vertices, triangles, origin, res, grid)
            # under an unrotated origin the probe cubes tile the grid's volume, so something is hit
            assert mask.any(), name
            assert int(mask.sum()) < 60, (name, int(mask.sum()))
            if name.startswith("segment"):
                assert int(mask.sum()) >= 5


@pytest.mark.parametrize("origin", list(MC.origins()))
def test_the_cells_of_a_box_as_triangles_are_cells_of_the_box_as_a_primitive(origin):
    o = MC.origins()[origin]
    (meshes, vertices, triangles), shapes = MC.box_pair(MC.GRIDS[0], o)
    surface, _, _ = R.restated(meshes, vertices, triangles, o, MC.RES, MC.GRIDS[0])
    solid, _, _ = SR.restated(shapes, o, MC.RES, MC.GRIDS[0])
    assert surface.any() and not (surface & ~solid).any()
    assert int(solid.sum()) > int(surface.sum()), "a probe wholly inside the closed mesh is not filled"


@pytest.mark.parametrize("name", [n for n in CASES if n.endswith("identity") or n.endswith("translation")])
def test_no_empty_cell_contains_a_point_sampled_on_a_triangle(name):
    meshes, vertices, triangles, origin, res, grid = CASES[name]
    mask, _, _ = R.restated(meshes, vertices, triangles, origin, res, grid)
    _, W = R.world_triangles(meshes, vertices, triangles)
    rng = np.random.default_rng(5)
    b = rng.dirichlet((1.0, 1.0, 1.0), 4000)                                              # barycentric samples, the same for every triangle
    pts = np.einsum("sb,tbk->tsk", b, W).reshape(-1, 3)
    g = (pts - np.asarray(origin)[:3, 3]) / res                                           # unrotated: the grid frame is a shift away
    idx = np.floor(g).astype(np.int64)
    frac = g - idx
    inside = np.all((idx >= 0) & (idx < np.asarray(grid)), axis=1) & np.all((frac > 1e-6) & (frac < 1 - 1e-6), axis=1)
    idx = idx[inside]
    assert mask[idx[:, 0], idx[:, 1], idx[:, 2]].all()


# ---- the kernels' own text on the host -------------------------------------------------------------------------------------------------
def _host_scenes():
    scenes = list(CASES.values()) + list(DYADIC.values()) + [MC.random_scene(s) for s in range(50)]
    planes = list(PLANES.values()) + list(DYADIC_PLANES.values()) + [MC.random_plane_scene(s) for s in range(50)]
    return scenes, planes


def test_the_kernels_text_on_the_host_is_bit_equal_to_the_restatement(host_predicate):
    scenes, planes = _host_scenes()
    cells = 0
    for meshes, vertices, triangles, origin, res, grid in scenes:
        c = R.centres(origin, res, grid)
        bad, ids, _, _ = host_predicate(meshes, vertices, triangles, NO_SHAPES, c, res * 0.5)
        assert bad == -1
        _, want, _ = R.restated(meshes, vertices, triangles, origin, res, grid)
        assert np.array_equal(ids, want.reshape(-1)), (grid, int((ids != want.reshape(-1)).sum()))
        cells += len(c)
    for shapes, origin, res, grid in planes:
        c = R.centres(origin, res, grid)
        _, _, first, valid = host_predicate(*NO_MESH, shapes, c, res * 0.5)
        assert valid.all()
        _, want, _ = R.restated_shapes(shapes, origin, res, grid)
        got = np.where(first > 0, shapes["object_id"][np.maximum(first, 1) - 1], 0).astype(np.uint32)
        assert np.array_equal(got, want.reshape(-1)), (grid, int((got != want.reshape(-1)).sum()))
        cells += len(c)
    assert cells > 500000


def test_the_host_text_is_clean_under_the_sanitizers(tmp_path):
    """a stand-alone program: AddressSanitizer and UndefinedBehaviorSanitizer on the predicate text and its validation"""
    exe = _build_host_predicate(tmp_path, SANITIZE)
    for i, name in enumerate(["icosahedron-generic-24x20x17-general", "segment-24x20x17-general", "huge-24x20x17-identity"]):
        meshes, vertices, triangles, origin, res, grid = CASES[name]
        c = R.centres(origin, res, grid)
        bad, ids, _, _ = _run_host_predicate(exe, tmp_path, i, meshes, vertices, triangles, PLANES["plane-generic-24x20x17-general"][0], c, res * 0.5)
        _, want, _ = R.restated(meshes, vertices, triangles, origin, res, grid)
        assert bad == -1 and np.array_equal(ids, want.reshape(-1))
    meshes, vertices, triangles = capi.make_meshes([(1, np.zeros((2, 3)), [(0, 1, 2)], np.eye(4))])      # an index out of range
    assert _run_host_predicate(exe, tmp_path, "bad", meshes, vertices, triangles, NO_SHAPES, np.zeros((1, 3)), 0.5)[0] == 0


def refusals():
    """name -> (meshes, vertices, triangles, the refused mesh index with ids asked for, the same without)"""
    good_v, good_t = MC.icosahedron(0.2)
    eye = np.eye(4)
    out = {}

    def three(middle, ids=(1, 2, 3)):
        return capi.make_meshes([(ids[0], good_v, good_t, eye), middle, (ids[2], good_v, good_t, eye)])

    bad_pose = np.eye(4)
    bad_pose[2, 1] = np.inf
    out["pose"] = three((2, good_v, good_t, bad_pose)) + (1, 1)
    v = good_v.copy()
    v[7, 1] = np.nan
    out["vertex"] = three((2, v, good_t, eye)) + (1, 1)
    t = good_t.copy()
    t[13, 2] = 12
    out["index"] = three((2, good_v, t, eye)) + (1, 1)
    out["id-zero"] = three((0, good_v, good_t, eye)) + (1, None)
    out["id-all-ones"] = three((0xFFFFFFFF, good_v, good_t, eye)) + (1, None)
    m, vv, tt = three((2, good_v, good_t, eye))
    m = m.copy()
    m["n_triangles"][2] = 21
    out["triangle-range"] = (m, vv, tt, 2, 2)
    m = m.copy()
    m["n_triangles"][2] = 20
    m["first_vertex"][0] = -1
    out["vertex-range"] = (m, vv, tt, 0, 0)
    m = three((2, good_v, good_t, eye))[0].copy()
    m["first_triangle"][2] = 0                                                            # 20 + 20 + 20 triangles named, but the sum may
    out["shared-run-is-fine"] = (m, vv, tt, None, None)                                   # not pass the array's 60: it does not
    m = m.copy()
    m["n_triangles"][2] = 21
    out["sum-past-the-array"] = (m, vv, tt, 2, 2)
    huge_pose = np.eye(4) * 1e200
    vbig = good_v * 1e200
    out["world-overflow"] = three((2, vbig, good_t, huge_pose)) + (1, 1)
    unused = np.vstack([good_v, [[np.nan, 0.0, 0.0]]])                                     # a vertex no triangle names is not read
    out["unused-vertex-is-fine"] = three((2, unused, good_t, eye)) + (None, None)
    return out


def test_refused_meshes_on_the_host(host_predicate):
    for name, (meshes, vertices, triangles, with_ids, without) in refusals().items():
        bad, _, _, _ = host_predicate(meshes, vertices, triangles, NO_SHAPES, np.zeros((1, 3)), 0.5)
        assert bad == (-1 if with_ids is None else with_ids), name
        assert R.mesh_refusal(meshes, vertices, triangles, ids=True) == with_ids, name
        assert R.mesh_refusal(meshes, vertices, triangles, ids=False) == without, name


def test_refused_planes_on_the_host(host_predicate):
    pose, bad_pose = np.eye(4), np.eye(4)
    bad_pose[0, 0] = np.nan
    items = [(capi.SHAPE_PLANE, 1, (0.0, 0.0, 1.0), pose), (capi.SHAPE_PLANE, 1, (-1.0, -2.0, -3.0), pose), (capi.SHAPE_PLANE, 1, (0.0, 0.0, 0.0), pose),
             (capi.SHAPE_PLANE, 1, (0.0, np.inf, 1.0), pose), (capi.SHAPE_PLANE, 1, (np.nan, 0.0, 1.0), pose), (capi.SHAPE_PLANE, 1, (0.0, 0.0, 1.0), bad_pose),
             (0, 1, (1.0,), pose), (4, 1, (1.0, 1.0), pose), (9, 1, (1.0,), pose), (77, 1, (1.0,), pose)]
    shapes = capi.make_shapes(items)
    _, _, _, valid = host_predicate(*NO_MESH, shapes, np.zeros((1, 3)), 0.5)
    assert valid.tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert [R.plane_valid(s["dims"], s["pose"]) for s in shapes[:6]] == [True, True, False, False, False, False]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_the_numpy_record(tmp_path):
    fields = ["object_id", "reserved", "first_triangle", "n_triangles", "first_vertex", "n_vertices", "pose"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdfgpu.h"\nint main(void) { printf("%zu ' + "%zu " * len(fields) + '%d %d %d\\n", '
                   "sizeof(sdfgpu_mesh), " + ", ".join("offsetof(sdfgpu_mesh, %s)" % f for f in fields) +
                   ", SDFGPU_SHAPE_PLANE, SDFGPU_MAX_MESHES, SDFGPU_MAX_TRIANGLES); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    dt = capi.MESH_DTYPE
    assert got == [dt.itemsize] + [dt.fields[f][1] for f in fields] + [capi.SHAPE_PLANE, capi.MAX_MESHES, capi.MAX_TRIANGLES]
    assert dt.itemsize == 168 and capi.SHAPE_PLANE == 5 == R.PLANE and capi.MAX_MESHES == 65536 and capi.MAX_TRIANGLES == 2 ** 24


def test_the_new_symbols_are_exported_and_declared():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "sdfgpu.h")).read()
    for name in ("sdfgpu_rasterize_meshes_device", "sdfgpu_rasterize_meshes"):
        assert name in capi.EXPORTS and hasattr(lib, name)
        assert re.search(r"^int %s\(" % name, header, re.M), name
    data = open(os.path.join(ROOT, "sdf_tools_amd", "libsdfgpu.so"), "rb").read()
    for kernel in (b"k_mr_meshes", b"k_mr_setup", b"k_mr_scan_blocks", b"k_mr_scan_top", b"k_mr_scatter", b"k_sc_raster"):
        assert kernel in data, kernel


def test_arguments_are_refused_before_a_device_is_needed():
    """a null handle is the one refusal that needs no context; the rest are tested on the GPU"""
    lib = capi.load_library()
    origin = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    out = (ctypes.c_uint32 * 4)()
    assert lib.sdfgpu_rasterize_meshes(None, None, 0, None, 0, None, 0, origin, 0.1, 2, 2, 2, out, None, None) == -1
    assert lib.sdfgpu_rasterize_meshes_device(None, None, 0, None, 0, None, 0, origin, 0.1, 2, 2, 2, out, None, None, 0, None, None) == -1


# ---- the C++ layer ---------------------------------------------------------------------------------------------------------------------
def test_the_mesh_example_compiles():
    from sdf_tools_amd import build
    assert os.path.exists(build.build_example("sdf_builder_mesh", force=True))             # -Wall -Wextra, against include/ and the in-tree library


@pytest.mark.parametrize("sanitized", [False, True])
def test_sdf_builder_mesh_exceptions_in_a_stand_alone_program(tmp_path, sanitized):
    """tests/sdf_builder_mesh_exceptions.cpp: the texts of the mesh and plane refusals, all thrown before the GPU is touched; once
    more under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program)"""
    exe = str(tmp_path / "sdf_builder_mesh_exceptions")
    pkg = os.path.join(ROOT, "sdf_tools_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-DSDF_TOOLS_VECTOR_ADOPT", *(SANITIZE if sanitized else []),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sdf_builder_mesh_exceptions.cpp"), "-o", exe,
                           "-L", pkg, "-lsdfgpu", "-Wl,-rpath," + pkg, "-lz"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert out.stdout.count("ok   ") >= 12


def test_pysdf_tools_binds_meshes_and_planes():
    from sdf_tools_amd._bindings import load_pysdf_tools
    m = load_pysdf_tools()
    for name in ("Mesh", "MeshTriangle", "Plane"):
        assert hasattr(m, name), name
    o = m.CollisionObject()
    for field in ("meshes", "mesh_poses", "planes", "plane_poses"):
        assert hasattr(o, field), field
    mesh = m.Mesh()
    mesh.set_vertices(np.zeros((4, 3)))
    mesh.set_triangles(np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    assert len(mesh.vertices) == 4 and len(mesh.triangles) == 2 and list(mesh.triangles[1].vertex_indices) == [0, 2, 3]
    p = m.Plane()
    p.coef = [0.0, 0.0, 1.0, -0.5]
    assert list(p.coef) == [0.0, 0.0, 1.0, -0.5]
