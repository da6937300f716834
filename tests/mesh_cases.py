"""The scenes of the mesh rasteriser's and the plane's tests (tests/test_mesh_raster_cpu.py judges the restatement on them,
tests/test_gpu_mesh_raster.py runs the device on them), on the grids and origins of scene_cases.
  cases():        name -> (meshes, vertices, triangles, origin, res, grid)   (capi.make_meshes arrays)
  plane_cases():  name -> (shapes, origin, res, grid)                        (capi.SHAPE_DTYPE records of type PLANE)
Meshes are placed in the GRID frame and carried to the world by the origin, as scene_cases does.  Sizes stay at a few voxels where
the exact judge has to look at every candidate."""
import functools

import numpy as np

import resample_restated
import scene_cases
from sdf_tools_amd import capi

RES, GRIDS, GENERIC_Q = scene_cases.RES, scene_cases.GRIDS, scene_cases.GENERIC_Q
IDENT_Q = (1.0, 0.0, 0.0, 0.0)
origins = scene_cases.origins
_local = scene_cases._local


def icosahedron(radius):
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
                  (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)], np.float64)
    t = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], np.uint32)
    return v * (radius / np.linalg.norm(v[0])), t


def box_triangles(dims):
    """the box of full extents dims about the origin as 12 triangles"""
    d = np.asarray(dims, np.float64) * 0.5
    v = np.array([((k & 1) * 2 - 1, ((k >> 1) & 1) * 2 - 1, ((k >> 2) & 1) * 2 - 1) for k in range(8)], np.float64) * d
    t = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)],
                 np.uint32)
    return v, t


def height_field(nu, nv, size_x, size_z, y_of):
    """2 nu nv triangles over [0, size_x] x [0, size_z] at height y = y_of(x, z) (the grid frame's y is up here)"""
    x, z = np.meshgrid(np.linspace(0.0, size_x, nu + 1), np.linspace(0.0, size_z, nv + 1), indexing="ij")
    v = np.stack([x, y_of(x, z), z], -1).reshape(-1, 3)
    i = (np.arange(nu)[:, None] * (nv + 1) + np.arange(nv)[None, :]).reshape(-1)
    t = np.concatenate([np.stack([i, i + nv + 1, i + nv + 2], 1), np.stack([i, i + nv + 2, i + 1], 1)]).astype(np.uint32)
    return v, t


def patch(count, ext, res):
    """`count` triangles of about two voxels each, laid out along a helix through the grid: every count is one mesh"""
    k = np.arange(count, dtype=np.float64)
    s = (k + 0.5) / count
    at = np.stack([(0.5 + 0.4 * np.cos(7.0 * s)) * ext[0], (0.5 + 0.4 * np.sin(7.0 * s)) * ext[1], s * ext[2]], 1)
    v = np.concatenate([at, at + np.array([2.1, 0.3, 0.2]) * res, at + np.array([0.4, 1.9, 1.1]) * res])
    t = np.stack([np.arange(count), np.arange(count) + count, np.arange(count) + 2 * count], 1).astype(np.uint32)
    return v, t


def one_mesh(variety, grid, origin, res=RES):
    origin = np.asarray(origin, np.float64)
    ext = np.asarray(grid, np.float64) * res
    centre = ext * np.array([0.47, 0.553, 0.41])
    radius = float(min(3.15 * res, 0.5 * max(ext)))
    if variety == "icosahedron-generic":
        (v, t), pose = icosahedron(radius), origin @ _local(GENERIC_Q, centre)
    elif variety == "icosahedron-grid-aligned":
        (v, t), pose = icosahedron(radius), origin @ _local(IDENT_Q, centre)
    elif variety == "box-12":
        (v, t), pose = box_triangles(np.minimum(ext, 6.3 * res)), origin @ _local(GENERIC_Q, centre)
    elif variety == "floor":
        # two triangles over a whole z = const layer (between voxel faces)
        zf = (np.floor(grid[2] * 0.4) + 0.37) * res
        v = np.array([(0, 0, zf), (ext[0], 0, zf), (ext[0], ext[1], zf), (0, ext[1], zf)], np.float64)
        t, pose = np.array([(0, 1, 2), (0, 2, 3)], np.uint32), origin @ _local(IDENT_Q, (0.0, 0.0, 0.0))
    elif variety == "sliver":
        v = np.array([(0.0, 0.0, 0.0), ext, ext + np.array([0.3, -0.2, 0.0]) * res], np.float64)
        t, pose = np.array([(0, 1, 2)], np.uint32), origin @ _local(IDENT_Q, (0.0, 0.0, 0.0))
    elif variety == "outside":
        (v, t), pose = icosahedron(radius), origin @ _local(GENERIC_Q, ext + 12.0 * res)
    elif variety == "huge":
        # triangles far larger than the grid, one through it and one past it
        big = 40.0 * float(np.linalg.norm(ext)) + 1.0
        v = np.array([(-big, -big * 0.7, 0.0), (big, -big * 0.6, 0.0), (0.1 * big, big, 0.0), (-big, -big, 3.0 * big), (big, -big, 3.0 * big),
                      (0.0, big, 3.1 * big)], np.float64)
        t, pose = np.array([(0, 1, 2), (3, 4, 5)], np.uint32), origin @ _local(GENERIC_Q, centre)
    elif variety == "segment":
        v = np.array([(-2.3 * res, 0.0, 0.0), (2.6 * res, 0.4 * res, 0.9 * res)], np.float64)
        t, pose = np.array([(0, 1, 1), (1, 0, 0), (0, 1, 0)], np.uint32), origin @ _local(GENERIC_Q, centre)
    elif variety == "point":
        v = np.array([(0.0, 0.0, 0.0)], np.float64)
        t, pose = np.array([(0, 0, 0)], np.uint32), origin @ _local(GENERIC_Q, centre)
    elif variety == "tiny":
        at = (np.floor(np.asarray(grid) * 0.5) + np.array([0.04, -0.03, 0.02])) * res
        v = np.array([(0.0, 0.0, 0.0), (0.1 * res, 0.0, 0.02 * res), (0.0, 0.08 * res, 0.0)], np.float64)
        t, pose = np.array([(0, 1, 2)], np.uint32), origin @ _local(GENERIC_Q, at)
    else:
        raise KeyError(variety)
    return capi.make_meshes([(1, v, t, pose)])


VARIETIES = ["icosahedron-generic", "icosahedron-grid-aligned", "box-12", "floor", "sliver", "outside", "huge", "segment", "point", "tiny"]


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    org = origins()
    for variety in VARIETIES:
        where = [(GRIDS[0], "general"), (GRIDS[0], "identity")]
        if variety in ("icosahedron-generic", "sliver", "tiny"):
            where.append((GRIDS[1], "general"))
        if variety == "floor":
            where = [(GRIDS[2], "identity"), (GRIDS[2], "general"), (GRIDS[0], "translation")]
        for grid, origin in where:
            out["%s-%s-%s" % (variety, "x".join(map(str, grid)), origin)] = one_mesh(variety, grid, org[origin]) + (org[origin], RES, grid)
    # several meshes with distinct ids, overlapping, on every grid under every origin; ids do not ascend with the list
    for grid in GRIDS:
        for origin in org:
            ext = np.asarray(grid, np.float64) * RES
            r = float(min(3.1 * RES, 0.5 * max(ext)))
            items = [(3, *icosahedron(r), org[origin] @ _local(GENERIC_Q, ext * np.array([0.4, 0.5, 0.45]))),
                     (1, *box_triangles(np.minimum(ext, 4.2 * RES)), org[origin] @ _local((0.9, -0.2, 0.3, 0.25), ext * np.array([0.5, 0.45, 0.5]))),
                     (2, *icosahedron(0.7 * r), org[origin] @ _local(IDENT_Q, ext * np.array([0.55, 0.5, 0.5])))]
            out["three-%s-%s" % ("x".join(map(str, grid)), origin)] = capi.make_meshes(items) + (org[origin], RES, grid)
    return out


def box_pair(grid, origin, res=RES):
    """(meshes arrays of the 12-triangle box, shape records of the same box as a primitive)"""
    ext = np.asarray(grid, np.float64) * res
    dims = np.minimum(ext, 6.3 * res)
    pose = np.asarray(origin, np.float64) @ _local(GENERIC_Q, ext * np.array([0.47, 0.553, 0.41]))
    return capi.make_meshes([(1, *box_triangles(dims), pose)]), capi.make_shapes([(capi.SHAPE_BOX, 1, dims, pose)])


@functools.lru_cache(maxsize=None)
def plane_cases():
    out = {}
    org = origins()
    for grid, oname in [(GRIDS[0], "general"), (GRIDS[0], "identity"), (GRIDS[1], "general"), (GRIDS[4], "translation")]:
        o = org[oname]
        ext = np.asarray(grid, np.float64) * RES
        centre = ext * np.array([0.47, 0.553, 0.41])
        name = "%s-%s" % ("x".join(map(str, grid)), oname)
        out["plane-generic-" + name] = (capi.make_shapes([(capi.SHAPE_PLANE, 1, (0.3, -1.1, 0.7), o @ _local(GENERIC_Q, centre))]), o, RES, grid)
        out["plane-axis-" + name] = (capi.make_shapes([(capi.SHAPE_PLANE, 2, (0.0, 0.0, -2.0), o @ _local(IDENT_Q, centre))]), o, RES, grid)
        out["plane-outside-" + name] = (capi.make_shapes([(capi.SHAPE_PLANE, 3, (0.0, 0.0, 1.0), o @ _local(IDENT_Q, ext + 7.3 * RES))]), o, RES, grid)
        out["plane-and-box-" + name] = (capi.make_shapes([(capi.SHAPE_BOX, 4, np.minimum(ext, 3.3 * RES), o @ _local(GENERIC_Q, centre)),
                                                         (capi.SHAPE_PLANE, 2, (0.2, 0.1, 1.0), o @ _local(IDENT_Q, centre))]), o, RES, grid)
    return out


def dyadic_cases():
    """Contact scenes in which every operation is exact: res 2^-3, vertices on multiples of 2^-4, identity rotation; triangles lying
    exactly in voxel faces, edges along voxel edges, a vertex on a voxel corner.  name -> a cases() tuple"""
    res, grid = 0.125, (16, 12, 10)
    shifted = np.eye(4)
    shifted[:3, 3] = (0.5, -1.0, 0.25)
    out = {}
    for oname, origin in (("identity", np.eye(4)), ("translation", shifted)):
        v = np.array([(0.25, 0.25, 0.5), (1.0, 0.25, 0.5), (0.25, 0.875, 0.5),          # in the face z = 0.5
                      (1.5, 0.125, 0.125), (1.5, 1.0, 0.125), (1.5, 0.125, 1.0),        # in the face x = 1.5
                      (0.5, 1.0, 0.0625), (0.5, 1.0, 1.1875), (0.5625, 1.0, 0.5)],      # in the face y = 1.0, off-face vertices in x
                     np.float64)
        t = np.array([(0, 1, 2), (3, 4, 5), (6, 7, 8)], np.uint32)
        out["dyadic-faces-" + oname] = capi.make_meshes([(1, v, t, origin)]) + (origin, res, grid)
    return out


def dyadic_plane_cases():
    res, grid = 0.125, (16, 12, 10)
    shifted = np.eye(4)
    shifted[:3, 3] = (0.5, -1.0, 0.25)
    out = {}
    for oname, origin in (("identity", np.eye(4)), ("translation", shifted)):
        pose = origin.copy()
        pose[:3, 3] = origin[:3, 3] + np.array([0.0, 0.0, 0.5])                       # the plane z = 0.5, a voxel face
        out["dyadic-plane-" + oname] = (capi.make_shapes([(capi.SHAPE_PLANE, 1, (0.0, 0.0, 2.0), pose)]), origin, res, grid)
    return out


def random_scene(seed):
    """a small random scene: a cases() tuple"""
    rng = np.random.default_rng(2000 + seed)
    grid = tuple(int(v) for v in rng.integers(1, 28, 3))
    res = float(rng.choice([0.05, 0.03, 0.125, 0.2]))
    origin = resample_restated.quaternion_origin(rng.normal(size=4), rng.uniform(-2.0, 2.0, 3)) if seed % 3 else np.eye(4)
    ext = np.asarray(grid, np.float64) * res
    items = []
    for i in range(int(rng.integers(1, 5))):
        nv = int(rng.integers(3, 12))
        v = rng.normal(size=(nv, 3)) * rng.uniform(0.3, 5.0) * res
        t = rng.integers(0, nv, (int(rng.integers(1, 14)), 3))
        pose = origin @ _local(rng.normal(size=4), rng.uniform(-0.1, 1.1, 3) * ext)
        items.append((int(rng.integers(1, 9)), v, t, pose))
    return capi.make_meshes(items) + (origin, res, grid)


def random_plane_scene(seed):
    rng = np.random.default_rng(3000 + seed)
    grid = tuple(int(v) for v in rng.integers(1, 28, 3))
    res = float(rng.choice([0.05, 0.03, 0.125, 0.2]))
    origin = resample_restated.quaternion_origin(rng.normal(size=4), rng.uniform(-2.0, 2.0, 3)) if seed % 3 else np.eye(4)
    ext = np.asarray(grid, np.float64) * res
    pose = origin @ _local(rng.normal(size=4), rng.uniform(-0.1, 1.1, 3) * ext)
    return capi.make_shapes([(capi.SHAPE_PLANE, 1 + seed % 5, rng.normal(size=3), pose)]), origin, res, grid
