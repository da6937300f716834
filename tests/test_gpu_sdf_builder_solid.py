"""GPU: sdf_tools::SDF_Builder with MESH_FILL_SOLID, through pysdf_tools.

A box given as 12 triangles, filled as a solid, gives the SDF of the same box as a primitive, field for field, and a negative
distance at its centre; the default mode gives what the builder always gave (the surface path called directly); a per-object
override mixes the two modes in one scene; an open mesh is a ValueError naming the object; a scene with more solid meshes than
SDFGPU_MAX_SOLID_MESHES is split into several calls and equals the restatement."""
import math

import numpy as np
import pytest

import mesh_cases as MC
import mesh_raster_restated as R
import mesh_solid_restated as S
import resample_restated
from sdf_tools_amd import capi
from sdf_tools_amd._bindings import load_pysdf_tools

pytestmark = pytest.mark.gpu
m = load_pysdf_tools()

ORIGIN_POSE = ((-0.37, -1.33, -0.02), (0.83, -0.21, 0.4, 0.32))                  # position, quaternion w x y z
SIZE, RES, OOB = (1.2, 1.0, 1.4), 0.04, 1e6
ORIGIN = resample_restated.quaternion_origin(ORIGIN_POSE[1], ORIGIN_POSE[0])
GRID = tuple(int(math.ceil(s / RES)) for s in SIZE)
BOX_DIMS = (0.3, 0.24, 0.34)
BOX_POSE = ((-0.1, -0.4, -0.37), (0.9, 0.1, -0.2, 0.3))
ICO_POSE = ((-0.05, -0.28, 0.14), (0.7, -0.3, 0.2, 0.4))


def _matrix(position, q):
    return resample_restated.quaternion_origin(q, position)


def _pose(position, q):
    w, x, y, z = q
    return m.Pose(list(position), [x, y, z, w])


def _mesh(v, t):
    mesh = m.Mesh()
    mesh.set_vertices(np.asarray(v, np.float64))
    mesh.set_triangles(np.asarray(t, np.uint32))
    return mesh


def _scene(objects):
    """objects: [(id, [(v, t, pose)], [(dims, pose)])] -> a PlanningScene of collision objects with meshes and box primitives"""
    scene, world, out = m.PlanningScene(), m.PlanningSceneWorld(), []
    for name, meshes, boxes in objects:
        o = m.CollisionObject()
        o.id = name
        o.meshes, o.mesh_poses = [_mesh(v, t) for v, t, _ in meshes], [_pose(*p) for _, _, p in meshes]
        o.primitives, o.primitive_poses = [m.SolidPrimitive(m.SolidPrimitive.BOX, list(d)) for d, _ in boxes], [_pose(*p) for _, p in boxes]
        out.append(o)
    world.collision_objects = out
    scene.world = world
    return scene


def _builder(size=SIZE, res=RES):
    return m.SDF_Builder(m.Isometry3d(ORIGIN), "world", size[0], size[1], size[2], res, OOB, None)


def _field(sdf, grid=GRID):
    return np.asarray(sdf.GetRawDataNumpy()).reshape(grid)


def _cell(position):
    centre = np.linalg.inv(ORIGIN) @ np.append(position, 1.0)
    return tuple(int(v) for v in np.floor(centre[:3] / RES))


def test_a_solid_box_mesh_gives_the_sdf_of_the_box_primitive(gpu):
    as_mesh, as_box = _builder(), _builder()
    as_mesh.UpdatePlanningSceneFromMessage(_scene([("box", [(*MC.box_triangles(BOX_DIMS), BOX_POSE)], [])]))
    as_box.UpdatePlanningSceneFromMessage(_scene([("box", [], [(BOX_DIMS, BOX_POSE)])]))
    as_mesh.SetMeshFill(m.MESH_FILL_SOLID)
    solid, primitive = _field(as_mesh.UpdateSDF(m.USE_CACHED)), _field(as_box.UpdateSDF(m.USE_CACHED))
    assert np.array_equal(solid.view(np.uint32), primitive.view(np.uint32)), int((solid != primitive).sum())
    assert solid[_cell(BOX_POSE[0])] < 0
    assert np.array_equal(as_mesh.UpdateCollisionMap(m.USE_CACHED), as_box.UpdateCollisionMap(m.USE_CACHED))
    device = as_mesh.UpdateSDFDevice(m.USE_CACHED)
    assert np.array_equal(_field(device.Host()).view(np.uint32), primitive.view(np.uint32))
    as_mesh.SetMeshFill(m.MESH_FILL_SURFACE)
    assert _field(as_mesh.UpdateSDF(m.USE_CACHED))[_cell(BOX_POSE[0])] > 0


def test_the_default_mode_is_the_surface_path(gpu):
    b = _builder()
    v, t = MC.box_triangles(BOX_DIMS)
    b.UpdatePlanningSceneFromMessage(_scene([("box", [(v, t, BOX_POSE)], [])]))
    meshes = capi.make_meshes([(1, v, t, _matrix(*BOX_POSE))])
    direct = gpu.rasterize_meshes(*meshes, ORIGIN, RES, GRID, bits=False, mask=True)["mask"]
    assert np.array_equal(b.UpdateCollisionMap(m.USE_CACHED), direct)
    assert np.array_equal(direct, R.restated(*meshes, ORIGIN, RES, GRID)[0])


def test_a_per_object_override_mixes_the_two_modes(gpu):
    box, ico = MC.box_triangles(BOX_DIMS), MC.icosahedron(0.21)
    scene = _scene([("shell", [(*box, BOX_POSE)], []), ("solid", [(*ico, ICO_POSE)], [])])
    b = _builder()
    b.UpdatePlanningSceneFromMessage(scene)
    b.SetObjectMeshFill("solid", m.MESH_FILL_SOLID)
    surface = R.restated(*capi.make_meshes([(1, *box, _matrix(*BOX_POSE))]), ORIGIN, RES, GRID)
    want, ids, _ = S.restated(*capi.make_meshes([(2, *ico, _matrix(*ICO_POSE))]), ORIGIN, RES, GRID, onto=(surface[0], surface[1]))
    got = np.asarray(b.UpdateCollisionMap(m.USE_CACHED))
    assert np.array_equal(got, want), int((got != want).sum())
    assert want[_cell(ICO_POSE[0])] == 1 and want[_cell(BOX_POSE[0])] == 0
    cells = np.asarray(b.UpdateTaggedCollisionMap(m.USE_CACHED).GetRawCellsNumpy()).reshape(-1, 16)
    assert np.array_equal(cells[:, 8:12].copy().view(np.uint32).reshape(GRID), ids)
    # the other way round: the builder's mode is SOLID, the first object is set back to its surface
    b.SetMeshFill(m.MESH_FILL_SOLID)
    b.SetObjectMeshFill("solid", m.MESH_FILL_SOLID)
    b.SetObjectMeshFill("shell", m.MESH_FILL_SURFACE)
    assert np.array_equal(np.asarray(b.UpdateCollisionMap(m.USE_CACHED)), want)


def test_an_open_mesh_is_refused_by_name(gpu):
    v, t = MC.icosahedron(0.21)
    b = _builder()
    b.UpdatePlanningSceneFromMessage(_scene([("closed", [(v, t, ICO_POSE)], []), ("open one", [(v, t, ICO_POSE), (v, t[:-1], BOX_POSE)], [])]))
    b.UpdateCollisionMap(m.USE_CACHED)                                         # fine as surfaces
    b.SetMeshFill(m.MESH_FILL_SOLID)
    with pytest.raises(ValueError, match="Collision object 'open one' has a mesh that is to be filled as a solid but is not closed"):
        b.UpdateSDF(m.USE_CACHED)
    with pytest.raises(ValueError, match="Invalid mesh fill mode"):
        b.SetMeshFill(3)


def test_more_solid_meshes_than_one_call_takes_are_split(gpu):
    """tiny boxes on a 24^3 grid, more of them than SDFGPU_MAX_SOLID_MESHES, in one collision object: several calls, one result"""
    res, size = 0.04, (0.96, 0.96, 0.96)
    grid = (24, 24, 24)
    rng = np.random.default_rng(9)
    count = capi.MAX_SOLID_MESHES + 44
    meshes = []
    for _ in range(count):
        at = ORIGIN @ np.append(rng.uniform(0.1, 0.86, 3), 1.0)
        meshes.append((*MC.box_triangles(rng.uniform(1.2, 3.4, 3) * res), (tuple(at[:3]), tuple(rng.normal(size=4)))))
    meshes = [(v, t, (p, tuple(np.asarray(q) / np.linalg.norm(q)))) for v, t, (p, q) in meshes]
    b = _builder(size, res)
    b.UpdatePlanningSceneFromMessage(_scene([("many", meshes, [])]))
    b.SetMeshFill(m.MESH_FILL_SOLID)
    got = np.asarray(b.UpdateCollisionMap(m.USE_CACHED))
    records = capi.make_meshes([(1, v, t, _matrix(*p)) for v, t, p in meshes])
    want = S.restated(*records, ORIGIN, res, grid)[0]
    assert got.shape == grid and np.array_equal(got, want), int((got != want).sum())
    assert int(want.sum()) > int(R.restated(*records, ORIGIN, res, grid)[0].sum())
