"""The scenes of the shape rasteriser's tests (tests/test_scene_raster_cpu.py judges the restatement on them, tests/test_gpu_scene_raster.py
runs the device on them): name -> (shapes as capi.SHAPE_DTYPE records, origin 4 x 4, resolution, grid).

Shapes are placed in the GRID frame (fractions of the grid's metric size) and carried to the world by the origin, so the same scene
sits in the same voxels under every origin; "world-aligned" ones take the identity rotation in the WORLD instead.  Sizes stay at a
few voxels: the judge works in fractions.Fraction."""
import functools

import numpy as np

import frame_judge
import resample_restated
from sdf_tools_amd import capi

BOX, SPHERE, CYLINDER = capi.SHAPE_BOX, capi.SHAPE_SPHERE, capi.SHAPE_CYLINDER
RES = 0.05                                             # not a binary fraction
GRIDS = [(24, 20, 17), (33, 9, 40), (64, 8, 64), (1, 1, 9), (20, 40, 1)]
TYPES = {"box": BOX, "sphere": SPHERE, "cylinder": CYLINDER}
GENERIC_Q = (0.71, 0.33, -0.52, 0.27)                  # all nine rotation entries nonzero and distinct


def origins():
    f = frame_judge.frames()
    return {k: f[k] for k in ("identity", "translation", "general")}


def _local(q, at):
    return resample_restated.quaternion_origin(q, at)


def _dims(kind, size):
    """dims of a shape of about `size` (three lengths)"""
    if kind == BOX:
        return (size[0], size[1], size[2])
    if kind == SPHERE:
        return (0.5 * min(size),)
    return (size[2], 0.5 * min(size[0], size[1]))


def one_shape(kind, variety, grid, origin, res=RES):
    """one shape record list for a (type, variety) on a grid under an origin"""
    origin = np.asarray(origin, np.float64)
    ext = np.asarray(grid, np.float64) * res
    few = np.minimum(ext, 6.3 * res)                    # a few voxels, or the grid's own size on a thin axis
    centre = ext * np.array([0.47, 0.553, 0.41])      # (on no voxel face of any grid)
    ident = (1.0, 0.0, 0.0, 0.0)
    if variety == "generic":
        pose, dims = origin @ _local(GENERIC_Q, centre), _dims(kind, few)
    elif variety == "grid-aligned":
        pose, dims = origin @ _local(ident, centre), _dims(kind, few)
    elif variety == "world-aligned":
        pose = np.eye(4)
        pose[:3, 3] = (origin @ np.append(centre, 1.0))[:3]
        dims = _dims(kind, few)
    elif variety == "across-regions":
        # long and thin through the whole grid, along the diagonal: it crosses every coarse and fine region edge on its way
        d = ext / np.linalg.norm(ext)
        z = np.array([0.0, 0.0, 1.0])
        axis, angle = np.cross(z, d), np.arccos(np.clip(d[2], -1.0, 1.0))
        if np.linalg.norm(axis) < 1e-12:
            q = ident
        else:
            axis = axis / np.linalg.norm(axis)
            q = (np.cos(angle / 2),) + tuple(np.sin(angle / 2) * axis)
        length = float(np.linalg.norm(ext)) * 1.1
        pose = origin @ _local(q, ext * 0.5)
        dims = {BOX: (0.7 * res, 0.9 * res, length), SPHERE: (0.45 * float(max(ext)),), CYLINDER: (length, 0.4 * res)}[kind]
        if kind == SPHERE and max(grid) > 40:
            dims = (9.2 * res,)
    elif variety == "outside":
        pose, dims = origin @ _local(GENERIC_Q, ext + 12.0 * res), _dims(kind, few)
    elif variety == "contains-grid":
        big = 4.0 * float(np.linalg.norm(ext)) + 1.0
        pose, dims = origin @ _local(GENERIC_Q, ext * 0.5), _dims(kind, (big, big, big))
        if kind == SPHERE:
            dims = (big,)
    elif variety == "degenerate":
        # radius 0, height 0, a box without thickness: a point, a disc or a segment, a rectangle
        pose = origin @ _local(GENERIC_Q, centre)
        dims = {BOX: (few[0], 0.0, few[2]), SPHERE: (0.0,), CYLINDER: (0.0, 0.5 * float(min(few[:2])))}[kind]
    elif variety == "degenerate-2":
        pose = origin @ _local(GENERIC_Q, centre)
        dims = {BOX: (0.0, 0.0, 0.0), SPHERE: (0.0,), CYLINDER: (float(few[2]), 0.0)}[kind]
    elif variety == "tiny":
        # smaller than a voxel, between centres (at a voxel corner, pushed off it a little)
        at = (np.floor(np.asarray(grid) * 0.5) + np.array([0.04, -0.03, 0.02])) * res
        pose = origin @ _local(GENERIC_Q, at)
        dims = _dims(kind, (0.2 * res, 0.2 * res, 0.2 * res))
    else:
        raise KeyError(variety)
    return capi.make_shapes([(kind, 1, dims, pose)])


VARIETIES = ["generic", "grid-aligned", "world-aligned", "across-regions", "outside", "contains-grid", "degenerate", "degenerate-2", "tiny"]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (shapes, origin, res, grid).  Every variety of every type on the first grid under the general origin and under the
    identity (three of them on the second grid too); all three types in generic poses, with distinct ids, on every grid under
    every origin."""
    out = {}
    org = origins()
    for kind_name, kind in TYPES.items():
        for variety in VARIETIES:
            where = [(GRIDS[0], "general"), (GRIDS[0], "identity")]
            if variety in ("generic", "across-regions", "tiny"):
                where.append((GRIDS[1], "general"))
            for grid, origin in where:
                name = "%s-%s-%s-%s" % (kind_name, variety, "x".join(map(str, grid)), origin)
                out[name] = (one_shape(kind, variety, grid, org[origin]), org[origin], RES, grid)
    for grid in GRIDS:
        for origin in org:
            shapes = []
            ext = np.asarray(grid, np.float64) * RES
            few = np.minimum(ext, 3.1 * RES)
            for i, (kind, q, where) in enumerate([(CYLINDER, GENERIC_Q, (0.3, 0.6, 0.35)), (BOX, (0.9, -0.2, 0.3, 0.25), (0.62, 0.4, 0.6)),
                                                  (SPHERE, (1.0, 0.0, 0.0, 0.0), (0.5, 0.5, 0.5))]):
                shapes.append((kind, i + 1, _dims(kind, few), org[origin] @ _local(q, ext * np.array(where))))
            out["three-%s-%s" % ("x".join(map(str, grid)), origin)] = (capi.make_shapes(shapes), org[origin], RES, grid)
    return out


def dyadic_cases():
    """Contact scenes in which every operation of the kernel is exact: res 2^-3, extents, radii and positions multiples of 2^-4,
    identity rotations, faces exactly on voxel faces.  name -> (shapes, origin, res, grid)"""
    res, grid = 0.125, (16, 12, 10)
    eye = np.eye(4)
    shifted = np.eye(4)
    shifted[:3, 3] = (0.5, -1.0, 0.25)

    def at(origin, x, y, z):
        p = np.eye(4)
        p[:3, 3] = origin[:3, 3] + np.array([x, y, z])
        return p

    out = {}
    for oname, origin in (("identity", eye), ("translation", shifted)):
        out["dyadic-box-" + oname] = (capi.make_shapes([(BOX, 1, (0.5, 0.25, 0.375), at(origin, 1.0, 0.625, 0.5625))]), origin, res, grid)
        out["dyadic-sphere-" + oname] = (capi.make_shapes([(SPHERE, 2, (0.25,), at(origin, 1.0, 0.75, 0.625))]), origin, res, grid)
        out["dyadic-cylinder-" + oname] = (capi.make_shapes([(CYLINDER, 3, (0.5, 0.25), at(origin, 0.75, 0.75, 0.625))]), origin, res, grid)
        out["dyadic-all-" + oname] = (capi.make_shapes([(BOX, 1, (0.5, 0.25, 0.375), at(origin, 1.0, 0.625, 0.5625)),
                                                        (SPHERE, 2, (0.25,), at(origin, 1.0, 0.75, 0.625)),
                                                        (CYLINDER, 3, (0.5, 0.25), at(origin, 0.75, 0.75, 0.625)),
                                                        (BOX, 4, (0.125, 0.125, 0.125), at(origin, 0.0625, 0.0625, 0.0625))]), origin, res, grid)
    return out


def octomap_boxes(count, grid, origin, res=RES, seed=7):
    """`count` small grid-aligned boxes (0.8 .. 1.6 voxels a side) scattered over the grid, ids cycling 1 .. 9"""
    rng = np.random.default_rng(seed)
    ext = np.asarray(grid, np.float64) * res
    items = []
    for i in range(count):
        pose = np.asarray(origin, np.float64) @ _local((1.0, 0.0, 0.0, 0.0), rng.uniform(0.0, 1.0, 3) * ext)
        items.append((BOX, 1 + i % 9, rng.uniform(0.8, 1.6, 3) * res, pose))
    return capi.make_shapes(items)


def random_scene(seed):
    """a small random scene: (shapes, origin, res, grid)"""
    rng = np.random.default_rng(1000 + seed)
    grid = tuple(int(v) for v in rng.integers(1, 28, 3))
    res = float(rng.choice([0.05, 0.03, 0.125, 0.2]))
    origin = resample_restated.quaternion_origin(rng.normal(size=4), rng.uniform(-2.0, 2.0, 3)) if seed % 3 else np.eye(4)
    ext = np.asarray(grid, np.float64) * res
    items = []
    for i in range(int(rng.integers(1, 7))):
        kind = int(rng.integers(1, 4))
        size = rng.uniform(0.3, 7.0, 3) * res
        pose = origin @ _local(rng.normal(size=4), rng.uniform(-0.1, 1.1, 3) * ext)
        items.append((kind, i + 1, _dims(kind, size), pose))
    return capi.make_shapes(items), origin, res, grid
