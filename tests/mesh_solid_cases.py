"""The scenes of the solid fill's tests (tests/test_mesh_solid_cpu.py judges the restatement on them, tests/test_gpu_mesh_solid.py
runs the device on them): closed meshes placed in the GRID frame and carried to the world by the origin, as mesh_cases does.
  cases():         name -> (meshes, vertices, triangles, origin, res, grid)   (capi.make_meshes arrays)
  dyadic_cases():  scenes in which every operation is exact and every tie happens
Sizes stay at a few voxels: the exact judge looks at every voxel."""
import functools

import numpy as np

import mesh_cases as MC
import resample_restated
from sdf_tools_amd import capi

RES, GENERIC_Q, IDENT_Q = MC.RES, MC.GENERIC_Q, MC.IDENT_Q
GRID = (11, 9, 12)
_local = MC._local
icosahedron, box_triangles = MC.icosahedron, MC.box_triangles


def torus(major, minor, nu=9, nv=6):
    """genus 1, about the z axis: 2 nu nv triangles"""
    u, v = np.meshgrid(np.arange(nu) * (2.0 * np.pi / nu), np.arange(nv) * (2.0 * np.pi / nv), indexing="ij")
    p = np.stack([(major + minor * np.cos(v)) * np.cos(u), (major + minor * np.cos(v)) * np.sin(u), minor * np.sin(v)], -1).reshape(-1, 3)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij"))
    a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    return p, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.uint32)


def subdivide(v, t):
    """every triangle into four, the midpoints shared: closed stays closed"""
    v = [tuple(p) for p in np.asarray(v, np.float64)]
    mid, out = {}, []

    def m(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            mid[key] = len(v)
            v.append(tuple(0.5 * (np.asarray(v[a]) + np.asarray(v[b]))))
        return mid[key]

    for a, b, c in np.asarray(t, np.int64):
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return np.asarray(v, np.float64), np.asarray(out, np.uint32)


def flipped(t, which):
    t = np.array(t, np.uint32)
    t[which] = t[which][:, ::-1]
    return t


def soup(v, t):
    """every triangle with three vertices of its own"""
    v, t = np.asarray(v, np.float64), np.asarray(t, np.int64)
    return v[t.reshape(-1)], np.arange(3 * len(t), dtype=np.uint32).reshape(-1, 3)


def joined(parts):
    """several (v, t) as ONE mesh"""
    vs, ts, n = [], [], 0
    for v, t in parts:
        vs.append(np.asarray(v, np.float64))
        ts.append(np.asarray(t, np.int64) + n)
        n += len(v)
    return np.concatenate(vs), np.concatenate(ts).astype(np.uint32)


def tilt(angle):
    """a rotation by `angle` about the axis (1, 1, 0) / sqrt 2, as a quaternion"""
    s = np.sin(0.5 * angle) / np.sqrt(2.0)
    return (np.cos(0.5 * angle), s, s, 0.0)


@functools.lru_cache(maxsize=None)
def cases():
    org = MC.origins()
    ext = np.asarray(GRID, np.float64) * RES
    centre = ext * np.array([0.47, 0.553, 0.46])
    out = {}

    def put(name, items, origin="general", grid=GRID):
        o = org[origin]
        out[name] = capi.make_meshes([(oid, v, t, o @ pose) for oid, v, t, pose in items]) + (o, RES, grid)

    ico = icosahedron(3.3 * RES)
    box = box_triangles((5.3 * RES, 4.1 * RES, 6.2 * RES))
    put("icosahedron-generic", [(1, *ico, _local(GENERIC_Q, centre))])
    put("icosahedron-identity", [(1, *ico, _local(GENERIC_Q, centre))], "identity")
    put("torus", [(1, *torus(3.1 * RES, 1.3 * RES), _local((0.93, 0.21, -0.28, 0.1), centre))], "translation")
    put("torus-upright", [(1, *torus(3.1 * RES, 1.3 * RES), _local((0.71, 0.7, 0.05, 0.02), centre))])
    put("box-12-generic", [(1, *box, _local(GENERIC_Q, centre))])
    put("box-12-tilted-1e-9", [(1, *box, _local(tilt(1.0e-9), centre))], "identity")
    put("box-12-tilted-1e-9-general", [(1, *box, _local(tilt(1.0e-9), centre))])
    hollow_grid = (14, 13, 15)
    outer, inner = box_triangles((10.6 * RES, 10.2 * RES, 11.1 * RES)), box_triangles((4.4 * RES, 4.6 * RES, 4.3 * RES))
    put("cube-in-cube-one-mesh", [(1, *joined([outer, inner]), _local(GENERIC_Q, np.asarray(hollow_grid) * RES * np.array([0.47, 0.553, 0.46])))],
        grid=hollow_grid)
    put("two-overlapping", [(3, *ico, _local(GENERIC_Q, centre - 1.2 * RES)), (2, *box, _local((0.9, -0.2, 0.3, 0.25), centre + 1.1 * RES))])
    put("poking-out-of-all-faces", [(1, *icosahedron(0.75 * float(max(ext))), _local(GENERIC_Q, 0.5 * ext))], grid=(7, 6, 8))
    put("outside", [(1, *ico, _local(GENERIC_Q, ext + 12.0 * RES))])
    put("all-flipped", [(1, ico[0], flipped(ico[1], np.arange(20)), _local(GENERIC_Q, centre))])
    put("half-flipped", [(1, ico[0], flipped(ico[1], np.arange(0, 20, 2)), _local(GENERIC_Q, centre))])
    put("soup", [(1, *soup(*ico), _local(GENERIC_Q, centre))])
    put("subdivided-torus", [(1, *subdivide(*torus(3.3 * RES, 1.9 * RES, 6, 5)), _local((0.93, 0.21, -0.28, 0.1), centre))], "identity")
    return out


def dyadic_cases():
    """res 2^-3, identity rotation, a box whose vertices project exactly onto column centres and whose faces pass exactly through voxel
    centres: every column on its outline and every cell on its faces is a tie"""
    res, grid = 0.125, (10, 9, 8)
    shifted = np.eye(4)
    shifted[:3, 3] = (0.5, -1.0, 0.25)
    lo, hi = np.array([0.1875, 0.3125, 0.1875]), np.array([0.8125, 0.6875, 0.6875])      # (k + 1/2) res each
    v, t = box_triangles(hi - lo)
    out = {}
    for oname, origin in (("identity", np.eye(4)), ("translation", shifted)):
        pose = origin.copy()
        pose[:3, 3] = origin[:3, 3] + 0.5 * (lo + hi)
        out["dyadic-box-" + oname] = capi.make_meshes([(1, v, t, pose)]) + (origin, res, grid)
        out["dyadic-box-flipped-" + oname] = capi.make_meshes([(1, v, flipped(t, np.arange(0, 12, 3)), pose)]) + (origin, res, grid)
    return out


def random_scene(seed):
    """a small random scene of closed meshes: a cases() tuple"""
    rng = np.random.default_rng(5000 + seed)
    grid = tuple(int(v) for v in rng.integers(1, 14, 3))
    res = float(rng.choice([0.05, 0.03, 0.125, 0.2]))
    origin = resample_restated.quaternion_origin(rng.normal(size=4), rng.uniform(-2.0, 2.0, 3)) if seed % 3 else np.eye(4)
    return capi.make_meshes(random_closed_meshes(rng, origin, res, grid)) + (origin, res, grid)


def random_closed_meshes(rng, origin, res, grid, most=4):
    """[(id, v, t, pose)]: randomly posed icosahedra, tori and boxes, randomly subdivided, with random flips"""
    ext = np.asarray(grid, np.float64) * res
    items = []
    for _ in range(int(rng.integers(1, most + 1))):
        kind = int(rng.integers(0, 3))
        if kind == 0:
            v, t = icosahedron(float(rng.uniform(0.4, 5.0)) * res)
        elif kind == 1:
            major = float(rng.uniform(1.5, 4.0)) * res
            v, t = torus(major, float(rng.uniform(0.2, 0.9)) * major, int(rng.integers(3, 8)), int(rng.integers(3, 6)))
        else:
            v, t = box_triangles(rng.uniform(0.3, 7.0, 3) * res)
        if rng.random() < 0.3:
            v, t = subdivide(v, t)
        if rng.random() < 0.2:
            v, t = soup(v, t)
        t = flipped(t, np.flatnonzero(rng.random(len(t)) < rng.random()))
        q = rng.normal(size=4) if rng.random() < 0.8 else IDENT_Q
        items.append((int(rng.integers(1, 12)), v, t, origin @ _local(q, rng.uniform(-0.1, 1.1, 3) * ext)))
    return items
