"""The scenes of the solid fill's tests (tests/test_mesh_solid_cpu.py judges the restatement on them, tests/test_gpu_mesh_solid.py
runs the device on them): closed meshes placed in the GRID frame and carried to the world by the origin, as mesh_cases does.
  cases():         name -> (meshes, vertices, triangles, origin, res, grid)   (capi.make_meshes arrays)
  dyadic_cases():  scenes in which every operation is exact and every tie happens
Sizes stay at a few voxels: the exact judge looks at every voxel.
  GRIDS, grid_scene(grid):   the smallest grid at which each mechanism of the kernels can break
  stack_scene(grid):         12 x 6 x nz (STACK_NZ) against the merge's words, lane groups and chunks
  slot_scene(variant):       1328 triangles against the work distribution (scan blocks, empty meshes, zero-tile slots)
  random_tall_scene(seed):   random closed meshes on narrow grids about 32, 64 and 2048 cells tall
These are judged by the restatement alone (test_mesh_solid_cpu.py says what each must contain)."""
import functools

import numpy as np

import mesh_cases as MC
import mesh_raster_restated as R
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


# Each grid is the smallest at which one mechanism of the kernels can break:
#   1 x 1 x 1     one column, one cell, one word: every index is 0
#   3 x 2 x 1     nz = 1: columns start at bits 0 .. 5 of ONE word of the field, the tail mask keeps a single bit
#   5 x 4 x 33    one bit in a second word: the carry across words, a lane group of 2 (wz = 2, exactly full), a spill word
#   7 x 6 x 67    an odd nz: columns start at every bit offset; wz = 3 in a group of 4 with an idle lane
#   17 x 33 x 40  more than 16 columns each way: the edges of the 16 x 16 column tiles, boxes that end inside a tile
#   16 x 16 x 2100  wz = 66 > 64: the chunk carry and the word before a chunk (one grid-aligned box runs the whole height, so the
#                 carry across word 64 is always 1; stack_scene below has the columns whose carry is 0 there)
# Lane groups of 8, 16 and 32, full groups beyond 2, nz % 32 == 0, a second chunk boundary and a last chunk of one word are
# stack_scene's (STACK_NZ); slots past a scan block, empty meshes and zero-tile slots are slot_scene's.
GRIDS = [(1, 1, 1), (3, 2, 1), (5, 4, 33), (7, 6, 67), (17, 33, 40), (16, 16, 2100)]


def grid_scene(grid, res=RES):
    """three closed meshes sized to the grid: a stretched icosahedron (on the tallest grid a grid-aligned box) along its whole height and
    out of both ends, a box in a generic pose, a torus through the top face"""
    origin = MC.origins()["translation" if grid[2] > 1000 else "general"]
    ext = np.asarray(grid, np.float64) * res
    v, t = icosahedron(1.0)
    long = (2, v * np.array([0.45 * ext[0] + res, 0.4 * ext[1] + res, 0.6 * ext[2]]), t, origin @ _local((0.999, 0.02, -0.03, 0.01), 0.5 * ext))
    if grid[2] > 1000:                                                         # (thin world boxes per triangle keep the restatement quick: no rotation)
        long = (2, *box_triangles((0.5 * ext[0] + 0.37 * res, 0.45 * ext[1] + 0.21 * res, 1.2 * ext[2])),
                origin @ _local(IDENT_Q, 0.5 * ext + np.array([0.13, -0.08, 0.0]) * res))
    box = (1, *box_triangles(np.minimum(0.6 * ext + res, 9.3 * res)), origin @ _local(GENERIC_Q, ext * np.array([0.4, 0.55, 0.3])))
    tor = (3, *torus(3.1 * res, 1.4 * res), origin @ _local((0.9, 0.3, -0.2, 0.1), ext * np.array([0.55, 0.5, 1.0])))
    return capi.make_meshes([long, box, tor]) + (origin, res, grid)


STACK_NZ = (32, 64, 96, 130, 250, 270, 500, 530, 1000, 1030, 2048, 2081, 4100, 4128)
STACK_GRIDS = [(12, 6, nz) for nz in STACK_NZ]


def stack_boundaries(nz):
    """the cells of a column at which the merge changes hands: the middle word of the column, and bits 2048 and 4096 (the first words
    of its second and third chunk of 64) where the grid goes on for ten cells more"""
    wz = (nz + 31) // 32
    return sorted({b for b in (32 * (wz // 2), 2048, 4096) if 0 < b < nz - 10})


def _z_boxes(origin, res, x, y, spans):
    """grid-aligned boxes over x[0] .. x[1] and y[0] .. y[1] (voxels), one per z span, joined to ONE mesh"""
    parts = []
    for z in spans:
        lo, hi = np.array([x[0], y[0], z[0]]) * res, np.array([x[1], y[1], z[1]]) * res
        v, t = box_triangles(hi - lo)
        parts.append((v + 0.5 * (lo + hi), t))
    return (*joined(parts), np.asarray(origin, np.float64))


@functools.lru_cache(maxsize=None)
def stack_scene(grid):
    """12 x 6 x nz under the translation origin (no rotation: the restatement's candidate boxes stay thin).  Three meshes:
      P (id 4) over x in [0.7, 5.6]: boxes stacked along z -- [2.4, 9.7], one [B - 17.6, B + 21.3] across every boundary B, and one
               from about nz - 12 out of the top of the grid (the parity is 1 when the column ends: the tail mask)
      Q (id 2) over x in [6.3, nx - 0.8]: from 1.3 to nz - 1.6 with a gap (B - 5.4, B + 6.7) at every B (the parity is 0 across B
               after earlier toggles)
      a small icosahedron in a generic pose between them
    nz is one of STACK_NZ: wz = 1 .. 129 takes every lane-group size of the merge, full and one word over, nz % 32 zero and not,
    one, two and three chunks, the last of them a single word."""
    nx, ny, nz = grid
    origin = MC.origins()["translation"]
    bounds = stack_boundaries(nz)
    p = [(2.4, 9.7)] + [(b - 17.6, b + 21.3) for b in bounds]
    p.append((max(nz - 11.7, p[-1][1] + 1.5), nz + 3.2))
    edges = [1.3] + [e for b in bounds for e in (b - 5.4, b + 6.7)] + [nz - 1.6]
    q = list(zip(edges[0::2], edges[1::2]))
    items = [(4, *_z_boxes(origin, RES, (0.7, 5.6), (0.7, 5.4), p)),
             (2, *_z_boxes(origin, RES, (6.3, nx - 0.8), (0.6, 5.2), q)),
             (7, *icosahedron(1.7 * RES), origin @ _local(GENERIC_Q, np.array([5.9, 3.1, 20.3]) * RES))]
    return capi.make_meshes(items) + (origin, RES, grid)


SLOT_GRID = (70, 70, 5)
SLOT_VARIANTS = ("trailing", "shared")


@functools.lru_cache(maxsize=None)
def slot_scene(variant="trailing"):
    """70 x 70 x 5, 1328 triangles in one call, laid out against the work distribution of the solid pass:
      1  an icosahedron subdivided three times (1280 triangles: its slots cross a scan block of 1024), flattened to the grid
      2  an empty mesh                                   4  an empty mesh
      3  a box wholly outside the grid in x (every slot has zero column tiles)
      5  a slightly tilted slab over 0.9 x 0.88 of the grid's xy extent (25 column tiles per triangle: chunks of 16 end inside a slot)
      6  a box inside the grid joined with a box far outside it, the triangle rows shuffled (zero-tile slots between the others)
    "trailing": the triangle array carries 40 triangles that no record uses.  "shared": a seventh record re-uses mesh 6's triangle and
    vertex runs with another pose and a lower id (and the array carries the 24 unused triangles that the slot rule then asks for)."""
    origin = MC.origins()["general"]
    ext = np.asarray(SLOT_GRID, np.float64) * RES
    rng = np.random.default_rng(77)
    v, t = icosahedron(1.0)
    for _ in range(3):
        v, t = subdivide(v, t)
    none = (np.zeros((0, 3)), np.zeros((0, 3), np.uint32))
    inner, outer = box_triangles(np.array([9.3, 7.7, 2.9]) * RES), box_triangles(np.array([5.0, 6.0, 3.0]) * RES)
    both_v, both_t = joined([inner, (outer[0] + np.array([400.0, -35.0, 0.0]) * RES, outer[1])])
    both_t = both_t[rng.permutation(len(both_t))]
    items = [(5, v * np.array([0.41 * ext[0], 0.38 * ext[1], 0.62 * ext[2]]), t, origin @ _local((0.9995, 0.004, -0.006, 0.03), ext * np.array([0.46, 0.52, 0.48]))),
             (9, *none, np.eye(4)),
             (3, *box_triangles(np.array([6.0, 8.0, 3.0]) * RES), origin @ _local(GENERIC_Q, ext * np.array([1.0, 0.5, 0.5]) + np.array([15.0, 0.0, 0.0]) * RES)),
             (1, *none, np.eye(4)),
             (8, *box_triangles(np.array([0.9 * ext[0], 0.88 * ext[1], 0.6 * RES])), origin @ _local(tilt(0.004), ext * np.array([0.5, 0.5, 0.9]))),
             (6, both_v, both_t, origin @ _local((0.97, 0.05, -0.04, 0.2), ext * np.array([0.8, 0.17, 0.5])))]
    meshes, vertices, triangles = capi.make_meshes(items)
    spare = 40 if variant == "trailing" else 24
    triangles = np.ascontiguousarray(np.concatenate([triangles, rng.integers(0, 3, (spare, 3)).astype(np.uint32)]))
    if variant == "shared":
        meshes = np.concatenate([meshes, meshes[-1:]])
        meshes[-1]["object_id"] = 2
        meshes[-1]["pose"] = (origin @ _local((0.9, -0.1, 0.1, 0.4), ext * np.array([0.25, 0.8, 0.45]))).reshape(-1)
    elif variant != "trailing":
        raise KeyError(variant)
    return meshes, vertices, triangles, origin, RES, SLOT_GRID


def random_tall_scene(seed):
    """a random scene of closed meshes on a narrow grid whose nz lies about one word, two words and 64 words: random_closed_meshes placed
    on a grid of nz = 12 and stretched along the grid's z (no rotation of the grid where it is tall: the restatement stays quick)"""
    rng = np.random.default_rng(9000 + seed)
    nx, ny = (int(v) for v in rng.integers(1, 9, 2))
    nz = int(rng.integers(31, 71)) if rng.random() < 0.5 else int(rng.integers(2040, 2091))
    res = float(rng.choice([0.05, 0.03, 0.125]))
    origin = np.eye(4)
    origin[:3, 3] = rng.uniform(-2.0, 2.0, 3) if seed % 3 else 0.0
    if nz < 100 and seed % 2:
        origin = resample_restated.quaternion_origin(rng.normal(size=4), origin[:3, 3])
    items = []
    for oid, v, t, pose in random_closed_meshes(rng, np.eye(4), res, (nx, ny, 12)):
        g = R.world(pose, v)
        g[:, 2] *= nz / 12.0
        items.append((oid, g, t, origin))
    return capi.make_meshes(items) + (origin, res, (nx, ny, nz))


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
