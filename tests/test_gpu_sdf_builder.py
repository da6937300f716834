"""GPU: sdf_tools::SDF_Builder (include/sdf_tools/sdf_builder.hpp) through pysdf_tools and through the C++ example (examples/sdf_builder.cpp).

The scene of the example is repeated here as capi shape records (the poses through resample_restated.quaternion_origin, which states
the products of sdf_tools::PoseToMatrix).  UpdateCollisionMap equals the restatement (tests/scene_raster_restated.py); UpdateSDF is
bit-equal to sdfgpu_build on that mask; the modes select the right parts of the scene; the cached getters return what the updates
returned; the exceptions are the reference's; the tagged map carries the 1-based object index and one more id for the octomap."""
import math
import subprocess

import numpy as np
import pytest

import resample_restated
import scene_raster_restated as R
from sdf_tools_amd import build, capi
from sdf_tools_amd._bindings import load_pysdf_tools

pytestmark = pytest.mark.gpu
m = load_pysdf_tools()

ORIGIN_POSE = ((-0.37, -1.33, -0.02), (0.83, -0.21, 0.4, 0.32))                  # position, quaternion w x y z
SIZE, RES, OOB = (1.6, 1.4, 1.8), 0.04, 1e6
TABLE_Q, OCTOMAP_POSE = (0.9, 0.1, -0.2, 0.3), ((-0.3, 0.2, 0.3), (0.8, -0.3, 0.1, 0.2))


def _matrix(position, q):
    return resample_restated.quaternion_origin(q, position)


def _octomap():
    centers = np.array([[0.05 * (i % 8), 0.05 * (i // 8), 0.1 * ((i * 7) % 3)] for i in range(40)])
    sizes = np.array([0.1 if i % 5 == 0 else 0.05 for i in range(40)])
    return centers, sizes


def _records(objects=True, octomap=True):
    """the example's scene as shape records, in SDF_Builder's order and with its ids"""
    items = []
    if objects:
        items += [(capi.SHAPE_BOX, 1, (0.9, 0.6, 0.1), _matrix((0.1, -0.05, -0.3), TABLE_Q)),
                  (capi.SHAPE_CYLINDER, 1, (0.5, 0.06), _matrix((0.1, -0.05, -0.55), TABLE_Q)),
                  (capi.SHAPE_SPHERE, 2, (0.17,), _matrix((0.2, 0.1, -0.12), (1.0, 0.0, 0.0, 0.0)))]
    if octomap:
        frame = _matrix(*OCTOMAP_POSE)
        oid = 3 if objects else 1
        for c, s in zip(*_octomap()):
            local = np.eye(4)
            local[:3, 3] = c
            # SDF_Builder::Multiply: rows of frame against columns of local, sums left to right
            pose = np.array([[frame[i, 0] * local[0, j] + frame[i, 1] * local[1, j] + frame[i, 2] * local[2, j] + frame[i, 3] * local[3, j]
                              for j in range(4)] for i in range(4)])
            items.append((capi.SHAPE_BOX, oid, (s, s, s), pose))
    return capi.make_shapes(items)


def _pose(position, q):
    w, x, y, z = q
    return m.Pose(list(position), [x, y, z, w])


def _scene():
    scene = m.PlanningScene()
    table, ball = m.CollisionObject(), m.CollisionObject()
    table.id, ball.id = "table", "ball"
    table.primitives = [m.SolidPrimitive(m.SolidPrimitive.BOX, [0.9, 0.6, 0.1]), m.SolidPrimitive(m.SolidPrimitive.CYLINDER, [0.5, 0.06])]
    table.primitive_poses = [_pose((0.1, -0.05, -0.3), TABLE_Q), _pose((0.1, -0.05, -0.55), TABLE_Q)]
    ball.primitives = [m.SolidPrimitive(m.SolidPrimitive.SPHERE, [0.17])]
    ball.primitive_poses = [_pose((0.2, 0.1, -0.12), (1.0, 0.0, 0.0, 0.0))]
    world = m.PlanningSceneWorld()
    world.collision_objects = [table, ball]
    octomap = m.OctomapBoxesWithPose()
    octomap.origin = _pose(*OCTOMAP_POSE)
    octomap.SetBoxesNumpy(*_octomap())
    world.octomap = octomap
    scene.world = world
    return scene


ORIGIN = _matrix(*ORIGIN_POSE)
GRID = tuple(int(math.ceil(s / RES)) for s in SIZE)


@pytest.fixture(scope="module")
def want():
    """mode name -> (mask, ids, bits) of the restatement"""
    parts = {"full": (True, True), "objects": (True, False), "octomap": (False, True)}
    return {k: R.restated(_records(*v), ORIGIN, RES, GRID) for k, v in parts.items()}


def _builder(source=None):
    return m.SDF_Builder(m.Isometry3d(ORIGIN), "world", SIZE[0], SIZE[1], SIZE[2], RES, OOB, source)


def test_pose_matrix_is_the_quaternion_products_of_the_tests():
    for position, q in (ORIGIN_POSE, OCTOMAP_POSE, ((0.1, -0.05, -0.3), TABLE_Q)):
        assert np.array_equal(_pose(position, q).matrix(), _matrix(position, q))


def test_collision_map_and_sdf_in_every_mode(gpu, want):
    asked = []

    def source(mode):
        asked.append(mode)
        return _scene()

    b = _builder(source)
    modes = {"full": m.USE_FULL_PLANNING_SCENE, "objects": m.USE_ONLY_COLLISION_OBJECTS, "octomap": m.USE_ONLY_OCTOMAP}
    for name, mode in modes.items():
        mask, _, _ = want[name]
        assert 0 < int(mask.sum()) < mask.size
        got = b.UpdateCollisionMap(mode)
        assert got.shape == GRID and np.array_equal(got, mask), (name, int((got != mask).sum()))
        assert np.array_equal(b.GetCachedCollisionMap(), mask)
        sdf = b.UpdateSDF(mode)
        field, _ = gpu.build(mask, RES, False)
        got_field = np.asarray(sdf.GetRawDataNumpy()).reshape(GRID)
        assert np.array_equal(got_field.view(np.uint32), field.view(np.uint32)), name
        assert np.array_equal(np.asarray(b.GetCachedSDF().GetRawDataNumpy()).reshape(GRID), got_field)
        assert (sdf.GetNumXCells(), sdf.GetNumYCells(), sdf.GetNumZCells()) == GRID and sdf.GetFrame() == "world"
        # the cached mode works on what the last fetch kept
        assert np.array_equal(b.UpdateCollisionMap(m.USE_CACHED), mask)
    assert asked == [3, 3, 2, 2, 1, 1]
    assert not np.array_equal(want["full"][0], want["objects"][0]) and not np.array_equal(want["full"][0], want["octomap"][0])
    assert np.array_equal(want["full"][0], want["objects"][0] | want["octomap"][0])


def test_message_tagged_map_and_device_field(gpu, want):
    b = _builder()
    b.UpdatePlanningSceneFromMessage(_scene())
    mask, ids, _ = want["full"]
    assert np.array_equal(b.UpdateCollisionMap(m.USE_CACHED), mask)
    tagged = b.UpdateTaggedCollisionMap(m.USE_CACHED)
    cells = np.asarray(tagged.GetRawCellsNumpy()).reshape(-1, 16)
    got_ids = cells[:, 8:12].copy().view(np.uint32).reshape(GRID)
    occupancy = cells[:, 0:4].copy().view(np.float32).reshape(GRID)
    assert np.array_equal(got_ids, ids) and set(np.unique(ids)) == {0, 1, 2, 3}
    assert np.array_equal(occupancy, mask.astype(np.float32))
    device = b.UpdateSDFDevice(m.USE_CACHED)
    field, extrema = gpu.build(mask, RES, False)
    assert np.array_equal(np.asarray(device.Host().GetRawDataNumpy()).reshape(GRID).view(np.uint32), field.view(np.uint32))
    assert tuple(device.GetExtrema()) == extrema


def test_exceptions(gpu):
    b = _builder()
    for call in (lambda: b.UpdateSDF(m.USE_CACHED), lambda: b.UpdateCollisionMap(m.USE_FULL_PLANNING_SCENE), lambda: b.UpdateSDF(m.USE_ONLY_OCTOMAP)):
        with pytest.raises(ValueError, match="No planning scene available"):
            call()
    with pytest.raises(ValueError, match="Invalid update mode"):
        b.UpdateSDF(4)
    with pytest.raises(ValueError, match="No cached SDF available"):
        b.GetCachedSDF()
    with pytest.raises(ValueError, match="No cached Collision Map available"):
        b.GetCachedCollisionMap()
    with pytest.raises(ValueError, match="has not been initialized"):
        m.SDF_Builder().UpdateSDF(m.USE_CACHED)
    scene = _scene()
    world = scene.world
    objects = world.collision_objects
    objects[1].primitives = [m.SolidPrimitive(m.SolidPrimitive.CONE, [0.2, 0.1])]
    world.collision_objects = objects
    scene.world = world
    b.UpdatePlanningSceneFromMessage(scene)
    with pytest.raises(ValueError, match="'ball' has a cone"):
        b.UpdateCollisionMap(m.USE_CACHED)
    with pytest.raises(ValueError, match="No cached Collision Map available"):
        b.GetCachedCollisionMap()                                             # a refused update caches nothing


def test_the_cpp_example(gpu, want, tmp_path):
    exe = build.build_example("sdf_builder")
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "the scene was fetched 6 times" in out.stdout and "refused: Collision object 'ball' has a cone" in out.stdout
    assert "sdf_builder example done" in out.stdout
    for name in ("full", "objects", "octomap", "cached"):
        mask = want["octomap" if name == "cached" else name][0]              # (the cached mode follows the octomap-only fetch)
        got = np.fromfile(tmp_path / ("collision_map_%s.u8" % name), np.uint8).reshape(GRID)
        assert np.array_equal(got, mask), name
        field, _ = gpu.build(mask, RES, False)
        assert np.array_equal(np.fromfile(tmp_path / ("sdf_%s.f32" % name), np.uint32), field.view(np.uint32).reshape(-1)), name
    assert np.array_equal(np.fromfile(tmp_path / "tagged_ids.u32", np.uint32).reshape(GRID), want["full"][1])
    field, _ = gpu.build(want["full"][0], RES, False)
    assert np.array_equal(np.fromfile(tmp_path / "device_sdf.f32", np.uint32), field.view(np.uint32).reshape(-1))
