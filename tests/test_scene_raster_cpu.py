"""CPU: the shape rasteriser's decision procedure without a GPU.

  - the numpy restatement (scene_raster_restated.py) against the exact judge (scene_judge.py) on every scene of scene_cases.py;
    the share of ambiguous cells is printed per case and capped at frame_judge.AMBIGUITY_CAP; the dyadic contact scenes must
    equal the judge with ties counted as hits, no allowance
  - a sampling cross-check: no cell the restatement calls empty holds one of 9^3 samples of its probe cube inside a shape
  - the text the kernels compile (sdfgpu_scene.hpp) built for the host and run on the same scenes: bit-equal to the restatement
  - struct sdfgpu_shape against capi.SHAPE_DTYPE; the new symbols exported and declared; the limit refused on the host"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import frame_judge
import scene_cases as SC
import scene_judge as J
import scene_raster_restated as R
from sdf_tools_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = SC.cases()
DYADIC = SC.dyadic_cases()


@pytest.fixture(scope="module")
def host_predicate(tmp_path_factory):
    """tests/scene_predicate_host.cpp built without FMA contraction; returns run(shapes, centres, h) -> (first hit + 1, valid, extents)"""
    d = tmp_path_factory.mktemp("scene_host")
    exe = str(d / "scene_predicate_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "sdf_tools_amd", "csrc"), os.path.join(ROOT, "tests", "scene_predicate_host.cpp"), "-o", exe])
    counter = [0]

    def run(shapes, centres, h):
        counter[0] += 1
        fin, fout = str(d / ("in%d" % counter[0])), str(d / ("out%d" % counter[0]))
        shapes = np.ascontiguousarray(shapes, capi.SHAPE_DTYPE)
        centres = np.ascontiguousarray(centres, np.float64)
        with open(fin, "wb") as f:
            f.write(np.array([len(shapes), len(centres)], np.int64).tobytes())
            f.write(np.array([h], np.float64).tobytes())
            f.write(shapes.tobytes())
            f.write(centres.tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
        n, s = len(centres), len(shapes)
        return np.frombuffer(raw, np.uint32, n), np.frombuffer(raw, np.uint8, s, 4 * n), np.frombuffer(raw[4 * n + s:], np.float64).reshape(s, 3)

    return run


# ---- restatement against the exact judge ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_agrees_with_the_exact_judge(name):
    shapes, origin, res, grid = CASES[name]
    mask, _, _ = R.restated(shapes, origin, res, grid)
    judged, ambiguous = J.check(mask, J.scene_ratio(shapes, origin, res, grid))
    print("%s: %d filled of %d judged, ambiguous share %.5f" % (name, int(mask.sum()), judged, ambiguous / judged))
    assert ambiguous <= frame_judge.AMBIGUITY_CAP * judged, (name, ambiguous, judged)
    if "outside" in name:
        assert not mask.any()
    elif "contains-grid" in name:
        assert mask.all()
    elif "tiny" not in name and "degenerate" not in name:
        assert 0 < int(mask.sum()) < mask.size or min(grid) == 1


@pytest.mark.parametrize("name", list(DYADIC))
def test_dyadic_contact_scenes_equal_the_judge_with_ties_as_hits(name):
    shapes, origin, res, grid = DYADIC[name]
    mask, _, _ = R.restated(shapes, origin, res, grid)
    ratio = J.scene_ratio(shapes, origin, res, grid)
    J.check(mask, ratio, ties_only=True)
    assert int((ratio == 0).sum()) > 0, "the scene has no contact: it tests nothing"


def test_degenerate_and_tiny_shapes_still_fill_their_cells():
    for name, (shapes, origin, res, grid) in CASES.items():
        if ("degenerate" in name or "tiny" in name) and "24x20x17-identity" in name:
            mask, _, _ = R.restated(shapes, origin, res, grid)
            # a point, a segment, a disc: under an unrotated origin the probe cubes tile the grid's volume, so something is hit
            # (under a rotated origin they do not tile it, and a point may fall between them: the reference's behaviour, kept)
            assert mask.any(), name
            assert int(mask.sum()) < 400, (name, int(mask.sum()))


# ---- sampling ------------------------------------------------------------------------------------------------------------------------
def _inside(rec, pts):
    pose = np.asarray(rec["pose"], np.float64).reshape(4, 4)
    q = (pts - pose[:3, 3]) @ np.linalg.inv(pose[:3, :3]).T
    d, kind = rec["dims"], int(rec["type"])
    if kind == R.BOX:
        return np.all(np.abs(q) <= d[:3] * 0.5, axis=-1)
    if kind == R.SPHERE:
        return (q * q).sum(-1) <= d[0] * d[0]
    return (np.abs(q[..., 2]) <= d[0] * 0.5) & (q[..., 0] ** 2 + q[..., 1] ** 2 <= d[1] * d[1])


@pytest.mark.parametrize("name", [n for n in CASES if "contains-grid" not in n and "64x8x64" not in n])
def test_no_empty_cell_holds_a_sample_inside_a_shape(name):
    shapes, origin, res, grid = CASES[name]
    mask, _, _ = R.restated(shapes, origin, res, grid)
    empty = np.flatnonzero(mask.reshape(-1) == 0)
    c = R.centres(origin, res, grid)[empty]
    # samples strictly inside the cube (a sample on the cube's face inside a shape by rounding alone proves nothing)
    k = np.linspace(-0.499, 0.499, 9) * res
    offsets = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    for rec in shapes:
        t = np.asarray(rec["pose"], np.float64).reshape(4, 4)[:3, 3]
        reach = float(np.abs(rec["dims"]).sum()) + res
        near = np.all(np.abs(c - t) <= reach, axis=1)
        pts = c[near][:, None, :] + offsets[None]
        bad = _inside(rec, pts).any(axis=1)
        assert not bad.any(), (name, int(bad.sum()), empty[near][bad][:5])


# ---- the kernels' own text on the host -------------------------------------------------------------------------------------------------
def test_the_kernels_text_on_the_host_is_bit_equal_to_the_restatement(host_predicate):
    scenes = list(CASES.values()) + list(DYADIC.values()) + [SC.random_scene(s) for s in range(50)]
    scenes.append((SC.octomap_boxes(65, SC.GRIDS[0], SC.origins()["general"]), SC.origins()["general"], SC.RES, SC.GRIDS[0]))
    cells = 0
    for shapes, origin, res, grid in scenes:
        c = R.centres(origin, res, grid)
        first, valid, extents = host_predicate(shapes, c, res * 0.5)
        assert valid.all()
        _, ids, _ = R.restated(shapes, origin, res, grid)
        got_ids = np.where(first > 0, shapes["object_id"][np.maximum(first, 1) - 1], 0).astype(np.uint32)
        assert np.array_equal(got_ids, ids.reshape(-1)), (grid, int((got_ids != ids.reshape(-1)).sum()))
        for rec, e in zip(shapes, extents):
            assert np.array_equal(e, R.half_extents(int(rec["type"]), [float(v) for v in rec["dims"]], rec["pose"]))
        cells += len(c)
    assert cells > 500000


def test_refused_shapes_on_the_host(host_predicate):
    pose = np.eye(4)
    bad_pose = np.eye(4)
    bad_pose[1, 3] = np.nan
    items = [(SC.BOX, 1, (1.0, 1.0, 1.0), pose), (4, 1, (1.0, 1.0), pose), (0, 1, (1.0,), pose), (SC.SPHERE, 1, (-1.0,), pose),
             (SC.CYLINDER, 1, (1.0, np.inf), pose), (SC.BOX, 1, (1.0, np.nan, 1.0), pose), (SC.SPHERE, 1, (1.0,), bad_pose),
             (SC.SPHERE, 1, (1.0, -5.0, np.nan), pose)]                                   # (dims a sphere does not use are not read)
    shapes = capi.make_shapes(items)
    _, valid, _ = host_predicate(shapes, np.zeros((1, 3)), 0.5)
    want = [1, 0, 0, 0, 0, 0, 0, 1]
    assert valid.tolist() == want
    assert [R.shape_valid(int(s["type"]), s["dims"], s["pose"]) for s in shapes] == [bool(v) for v in want]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_the_numpy_record(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdfgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", '
                   "sizeof(sdfgpu_shape), offsetof(sdfgpu_shape, type), offsetof(sdfgpu_shape, object_id), offsetof(sdfgpu_shape, dims), "
                   "offsetof(sdfgpu_shape, pose), SDFGPU_SHAPE_BOX, SDFGPU_SHAPE_SPHERE, SDFGPU_SHAPE_CYLINDER, SDFGPU_MAX_SHAPES); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    dt = capi.SHAPE_DTYPE
    assert got == [dt.itemsize, dt.fields["type"][1], dt.fields["object_id"][1], dt.fields["dims"][1], dt.fields["pose"][1],
                   capi.SHAPE_BOX, capi.SHAPE_SPHERE, capi.SHAPE_CYLINDER, capi.MAX_SHAPES]
    assert dt.itemsize == 160 and (R.BOX, R.SPHERE, R.CYLINDER) == (1, 2, 3) == (J.BOX, J.SPHERE, J.CYLINDER)


def test_the_new_symbols_are_exported_and_declared():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "sdfgpu.h")).read()
    for name in ("sdfgpu_rasterize_shapes_device", "sdfgpu_rasterize_shapes"):
        assert name in capi.EXPORTS and hasattr(lib, name)
        assert re.search(r"^int %s\(" % name, header, re.M), name
    data = open(os.path.join(ROOT, "sdf_tools_amd", "libsdfgpu.so"), "rb").read()
    assert b"k_sc_raster" in data and b"k_sc_coarse" in data and b"k_sc_prepare" in data


def test_arguments_are_refused_before_a_device_is_needed():
    """a null handle is the one refusal that needs no context; the rest are tested on the GPU"""
    lib = capi.load_library()
    origin = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    out = (ctypes.c_uint32 * 4)()
    assert lib.sdfgpu_rasterize_shapes(None, None, 0, origin, 0.1, 2, 2, 2, out, None, None) == -1
    assert lib.sdfgpu_rasterize_shapes_device(None, None, 0, origin, 0.1, 2, 2, 2, out, None, None, None, None) == -1


# ---- the C++ layer ---------------------------------------------------------------------------------------------------------------------
def test_the_example_and_the_headers_compile(tmp_path):
    from sdf_tools_amd import build
    exe = build.build_example("sdf_builder", force=True)                       # -Wall -Wextra, against include/ and the in-tree library
    assert os.path.exists(exe)
    for header in ("sdf_tools/planning_scene.hpp", "sdf_tools/sdf_builder.hpp"):   # each on its own: a header includes what it uses
        unit = tmp_path / (os.path.basename(header) + ".cpp")
        unit.write_text('#include "%s"\nint main() { return 0; }\n' % header)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(unit)])


def test_sdf_builder_exceptions_in_a_stand_alone_program(tmp_path):
    """tests/sdf_builder_exceptions.cpp: the reference's exception texts and the refusals, all thrown before the GPU is touched"""
    exe = str(tmp_path / "sdf_builder_exceptions")
    pkg = os.path.join(ROOT, "sdf_tools_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-DSDF_TOOLS_VECTOR_ADOPT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "sdf_builder_exceptions.cpp"), "-o", exe, "-L", pkg, "-lsdfgpu", "-Wl,-rpath," + pkg, "-lz"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "0 failures" in out.stdout and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert out.stdout.count("ok   ") == 23


def test_pysdf_tools_binds_the_builder_and_its_messages():
    from sdf_tools_amd._bindings import load_pysdf_tools
    m = load_pysdf_tools()
    for name in ("SDF_Builder", "PlanningScene", "PlanningSceneWorld", "CollisionObject", "SolidPrimitive", "Pose", "OctomapBoxesWithPose"):
        assert hasattr(m, name), name
    assert (m.USE_CACHED, m.USE_ONLY_OCTOMAP, m.USE_ONLY_COLLISION_OBJECTS, m.USE_FULL_PLANNING_SCENE) == (0, 1, 2, 3)
    assert (m.SolidPrimitive.BOX, m.SolidPrimitive.SPHERE, m.SolidPrimitive.CYLINDER, m.SolidPrimitive.CONE) == (1, 2, 3, 4)
    b = m.SDF_Builder("world", 1.0, 1.0, 1.0, 0.1, 100.0)
    with pytest.raises(ValueError, match="No planning scene available"):
        b.UpdateSDF(m.USE_FULL_PLANNING_SCENE)
    with pytest.raises(ValueError, match="No cached SDF available"):
        b.GetCachedSDF()
