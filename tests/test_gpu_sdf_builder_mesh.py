"""GPU: sdf_tools::SDF_Builder on a scene with a primitive, a mesh and planes, through pysdf_tools.

The scene is repeated here as capi records (poses through resample_restated.quaternion_origin, the plane's frame through the products
of SDF_Builder::Multiply).  UpdateCollisionMap equals the restatements (shapes and planes first in list order, meshes accumulated);
the tagged map's ids match; UpdateSDF equals the exact oracle on the restated mask; UpdateSDFDevice gives the same field; a scene
without meshes still goes the way it went."""
import math

import numpy as np
import pytest

import mesh_cases as MC
import mesh_raster_restated as R
import resample_restated
from oracle import oracle as O
from sdf_tools_amd import capi
from sdf_tools_amd._bindings import load_pysdf_tools

pytestmark = pytest.mark.gpu
m = load_pysdf_tools()

ORIGIN_POSE = ((-0.37, -1.33, -0.02), (0.83, -0.21, 0.4, 0.32))                  # position, quaternion w x y z
SIZE, RES, OOB = (1.2, 1.0, 1.4), 0.04, 1e6
ORIGIN = resample_restated.quaternion_origin(ORIGIN_POSE[1], ORIGIN_POSE[0])
GRID = tuple(int(math.ceil(s / RES)) for s in SIZE)
BOX_POSE = ((-0.1, -0.4, -0.37), (0.9, 0.1, -0.2, 0.3))
MESH_POSE = ((-0.05, -0.28, 0.14), (0.7, -0.3, 0.2, 0.4))
PLANE_POSE = ((-0.28, -0.58, -0.37), (0.95, 0.2, 0.1, -0.1))
PLANE_COEF = (0.2, -0.1, 1.0, 0.15)
WALL_COEF = (1.0, 0.0, 0.0, 0.3)                                                    # a second plane, in the second object


def _matrix(position, q):
    return resample_restated.quaternion_origin(q, position)


def _pose(position, q):
    w, x, y, z = q
    return m.Pose(list(position), [x, y, z, w])


def _plane_record(oid, coef, pose):
    """SDF_Builder's plane: frame = PoseToMatrix(pose) * translate(p0), p0 = (-d / (a^2 + b^2 + c^2)) (a, b, c), dims = (a, b, c)"""
    a, b, c, d = coef
    scale = -d / (a * a + b * b + c * c)
    frame, local = _matrix(*pose), np.eye(4)
    local[:3, 3] = (scale * a, scale * b, scale * c)
    full = np.array([[frame[i, 0] * local[0, j] + frame[i, 1] * local[1, j] + frame[i, 2] * local[2, j] + frame[i, 3] * local[3, j]
                      for j in range(4)] for i in range(4)])
    return (capi.SHAPE_PLANE, oid, (a, b, c), full)


def _mesh_arrays():
    return MC.icosahedron(0.21)


def _records():
    shapes = capi.make_shapes([(capi.SHAPE_BOX, 1, (0.3, 0.2, 0.25), _matrix(*BOX_POSE)), _plane_record(1, PLANE_COEF, PLANE_POSE),
                               _plane_record(2, WALL_COEF, PLANE_POSE)])
    meshes = capi.make_meshes([(2, *_mesh_arrays(), _matrix(*MESH_POSE)), (2, *MC.box_triangles((0.2, 0.3, 0.1)), _matrix(*BOX_POSE))])
    return shapes, meshes


def _scene(with_meshes=True):
    scene, world = m.PlanningScene(), m.PlanningSceneWorld()
    first, second = m.CollisionObject(), m.CollisionObject()
    first.id, second.id = "box and floor", "meshes and wall"
    first.primitives, first.primitive_poses = [m.SolidPrimitive(m.SolidPrimitive.BOX, [0.3, 0.2, 0.25])], [_pose(*BOX_POSE)]
    first.planes, first.plane_poses = [m.Plane(list(PLANE_COEF))], [_pose(*PLANE_POSE)]
    second.planes, second.plane_poses = [m.Plane(list(WALL_COEF))], [_pose(*PLANE_POSE)]
    if with_meshes:
        ico, box = m.Mesh(), m.Mesh()
        v, t = _mesh_arrays()
        ico.set_vertices(v)                                                    # numpy arrays ...
        ico.set_triangles(t)
        v, t = MC.box_triangles((0.2, 0.3, 0.1))
        box.set_vertices(v)
        box.triangles = [m.MeshTriangle([int(i) for i in tri]) for tri in t]   # ... and the message's own lists
        second.meshes, second.mesh_poses = [ico, box], [_pose(*MESH_POSE), _pose(*BOX_POSE)]
    world.collision_objects = [first, second]
    scene.world = world
    return scene


@pytest.fixture(scope="module")
def want():
    shapes, meshes = _records()
    smask, sids, _ = R.restated_shapes(shapes, ORIGIN, RES, GRID)
    mask, ids, bits = R.restated(*meshes, ORIGIN, RES, GRID, onto=(smask, sids))
    assert (mask > smask).any(), "the meshes add nothing to the shapes"
    return {"shapes": (smask, sids), "all": (mask, ids, bits)}


def _builder():
    return m.SDF_Builder(m.Isometry3d(ORIGIN), "world", SIZE[0], SIZE[1], SIZE[2], RES, OOB, None)


def _tagged(tagged):
    cells = np.asarray(tagged.GetRawCellsNumpy()).reshape(-1, 16)
    return cells[:, 8:12].copy().view(np.uint32).reshape(GRID), cells[:, 0:4].copy().view(np.float32).reshape(GRID)


def test_collision_map_tagged_map_and_sdf_of_a_scene_with_a_mesh_and_planes(gpu, want):
    b = _builder()
    b.UpdatePlanningSceneFromMessage(_scene())
    mask, ids, _ = want["all"]
    got = b.UpdateCollisionMap(m.USE_CACHED)
    assert got.shape == GRID and np.array_equal(got, mask), int((np.asarray(got) != mask).sum())
    got_ids, occupancy = _tagged(b.UpdateTaggedCollisionMap(m.USE_CACHED))
    assert np.array_equal(got_ids, ids) and set(np.unique(ids)) == {0, 1, 2}
    assert np.array_equal(occupancy, mask.astype(np.float32))
    exact, extrema, _ = O.exact_sdf(mask, RES, False)
    field = np.asarray(b.UpdateSDF(m.USE_CACHED).GetRawDataNumpy()).reshape(GRID)
    assert np.array_equal(field.view(np.uint32), exact.view(np.uint32))
    device = b.UpdateSDFDevice(m.USE_CACHED)
    assert np.array_equal(np.asarray(device.Host().GetRawDataNumpy()).reshape(GRID).view(np.uint32), exact.view(np.uint32))
    assert tuple(device.GetExtrema()) == extrema
    # a probe inside the closed icosahedron is empty: the field is positive at its centre
    centre = np.linalg.inv(ORIGIN) @ np.append(MESH_POSE[0], 1.0)
    i = tuple(int(v) for v in np.floor(centre[:3] / RES))
    assert mask[i] == 0 and field[i] > 0


def test_a_scene_with_planes_and_no_meshes(gpu, want):
    b = _builder()
    b.UpdatePlanningSceneFromMessage(_scene(with_meshes=False))
    smask, sids = want["shapes"]
    assert np.array_equal(b.UpdateCollisionMap(m.USE_CACHED), smask)
    got_ids, _ = _tagged(b.UpdateTaggedCollisionMap(m.USE_CACHED))
    assert np.array_equal(got_ids, sids) and set(np.unique(sids)) == {0, 1, 2}
    exact, _, _ = O.exact_sdf(smask, RES, False)
    assert np.array_equal(np.asarray(b.UpdateSDF(m.USE_CACHED).GetRawDataNumpy()).reshape(GRID).view(np.uint32), exact.view(np.uint32))


def test_refusals_reach_python_as_value_errors(gpu):
    b = _builder()
    scene = _scene()
    world = scene.world
    objects = world.collision_objects
    objects[1].mesh_poses = objects[1].mesh_poses[:1]
    world.collision_objects = objects
    scene.world = world
    b.UpdatePlanningSceneFromMessage(scene)
    with pytest.raises(ValueError, match=r"'meshes and wall' has meshes without a pose each \(2 meshes, 1 mesh poses\)"):
        b.UpdateSDF(m.USE_CACHED)
    objects[1].mesh_poses = [_pose(*MESH_POSE), _pose(*BOX_POSE)]
    objects[0].planes = [m.Plane([0.0, 0.0, 0.0, 1.0])]
    world.collision_objects = objects
    scene.world = world
    b.UpdatePlanningSceneFromMessage(scene)
    with pytest.raises(ValueError, match="'box and floor' has a plane with a zero or non-finite normal"):
        b.UpdateCollisionMap(m.USE_CACHED)

