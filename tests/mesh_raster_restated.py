"""The mesh rasteriser's decision procedure and the plane's (include/sdfgpu.h "Planes and triangle meshes",
sdf_tools_amd/csrc/sdfgpu_mesh.hpp, sc_plane in sdfgpu_scene.hpp) restated in numpy float64: operation for operation what mr_world,
mr_triangle, mr_hit and sc_plane do, vectorised over the voxels.  numpy never fuses a product with a sum, so the parenthesisation
below is the rounding order.

What is NOT restated is the culling (mr_index_box, mr_may_hit): it only keeps a triangle from voxels whose probes are further from
it than 0.25 h plus a padding many orders above the rounding.  restated() evaluates a triangle at the voxels whose centres lie
inside its world bounding box inflated by the resolution and nowhere else, which is the same statement: a probe that meets the
triangle has its centre within h of that box on every world axis.  (It needs an origin with an inverse; the kernel does not.)

restated() returns the byte mask, the smallest-hit object ids and the packed bit field."""
import numpy as np

import scene_raster_restated as S

PLANE = 5
centres, centres_of, pack_bits = S.centres, S.centres_of, S.pack_bits


def world(pose, v):
    """W = pose * v, rows as ((m0 v0 + m1 v1) + m2 v2) + m3; v [n, 3] -> [n, 3]"""
    p = np.asarray(pose, np.float64).reshape(4, 4)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    return np.stack([((p[r, 0] * v[:, 0] + p[r, 1] * v[:, 1]) + p[r, 2] * v[:, 2]) + p[r, 3] for r in range(3)], 1)


def triangle_constants(W):
    """W [..., 3, 3] (vertex, axis) -> (f [3][3] edges f_j = W_{j+1} - W_j as lists of components, n = f_0 x f_1)"""
    W = np.asarray(W, np.float64)
    f = [[W[..., (j + 1) % 3, k] - W[..., j, k] for k in range(3)] for j in range(3)]
    n = [f[0][1] * f[1][2] - f[0][2] * f[1][1], f[0][2] * f[1][0] - f[0][0] * f[1][2], f[0][0] * f[1][1] - f[0][1] * f[1][0]]
    return f, n


def _separates(p0, p1, p2, r):
    return (np.minimum(np.minimum(p0, p1), p2) > r) | (np.maximum(np.maximum(p0, p1), p2) < -r)


def triangle(W, c, h):
    """mr_hit: world vertices W ([3, 3], or [n, 3, 3]: one triangle per centre) against the probes of half side h about c [n, 3]"""
    W = np.asarray(W, np.float64)
    f, n = triangle_constants(W)
    u = [[W[..., i, k] - c[:, k] for k in range(3)] for i in range(3)]
    ok = np.ones(len(c), bool)
    for a in range(3):
        ok &= ~_separates(u[0][a], u[1][a], u[2][a], h)
    p = [(n[0] * u[i][0] + n[1] * u[i][1]) + n[2] * u[i][2] for i in range(3)]
    ok &= ~_separates(p[0], p[1], p[2], h * ((np.abs(n[0]) + np.abs(n[1])) + np.abs(n[2])))
    for a in range(3):
        a1, a2 = (a + 1) % 3, (a + 2) % 3
        for j in range(3):
            fa1, fa2 = f[j][a1], f[j][a2]
            p = [u[i][a2] * fa1 - u[i][a1] * fa2 for i in range(3)]
            ok &= ~_separates(p[0], p[1], p[2], h * (np.abs(fa2) + np.abs(fa1)))
    return ok


def plane_valid(dims, pose):
    d, p = np.asarray(dims, np.float64).reshape(-1)[:3], np.asarray(pose, np.float64).reshape(-1)
    return bool(np.isfinite(d).all() and np.any(d != 0.0) and np.isfinite(p[:12]).all())


def plane(dims, pose, c, h):
    """sc_plane: N = R n, s = N . (c - T), filled iff |s| <= h (|N_0| + |N_1| + |N_2|)"""
    p = np.asarray(pose, np.float64).reshape(4, 4)
    N = [(p[a, 0] * dims[0] + p[a, 1] * dims[1]) + p[a, 2] * dims[2] for a in range(3)]
    s = (N[0] * (c[:, 0] - p[0, 3]) + N[1] * (c[:, 1] - p[1, 3])) + N[2] * (c[:, 2] - p[2, 3])
    return np.abs(s) <= h * ((abs(N[0]) + abs(N[1])) + abs(N[2]))


def mesh_refusal(meshes, vertices, triangles, ids=True):
    """the lowest refused mesh index (None: none), by the rules of the device and of the host form"""
    vertices = np.asarray(vertices, np.float64).reshape(-1, 3)
    triangles = np.asarray(triangles, np.uint32).reshape(-1, 3)
    slots = 0
    for i, m in enumerate(meshes):
        ft, nt, fv, nv = (int(m[k]) for k in ("first_triangle", "n_triangles", "first_vertex", "n_vertices"))
        ok = 0 <= ft <= len(triangles) and 0 <= nt <= len(triangles) - ft and 0 <= fv <= len(vertices) and 0 <= nv <= len(vertices) - fv
        ok = ok and bool(np.isfinite(np.asarray(m["pose"])[:12]).all())
        ok = ok and not (ids and int(m["object_id"]) in (0, 0xFFFFFFFF))
        if ok:
            slots += nt
            ok = slots <= len(triangles)
        if ok and nt:
            t = triangles[ft:ft + nt].astype(np.int64)
            ok = bool((t < nv).all())
            if ok:
                v = vertices[fv + np.unique(t)]
                with np.errstate(over="ignore", invalid="ignore"):
                    ok = bool(np.isfinite(v).all() and np.isfinite(world(m["pose"], v)).all())
        if not ok:
            return i
    return None


def world_triangles(meshes, vertices, triangles):
    """(object ids uint32 [n], W [n, 3, 3]) of every triangle of every mesh, in mesh and triangle order"""
    vertices = np.asarray(vertices, np.float64).reshape(-1, 3)
    triangles = np.asarray(triangles, np.uint32).reshape(-1, 3)
    oid, Ws = [np.zeros(0, np.uint32)], [np.zeros((0, 3, 3))]
    for m in meshes:
        ft, nt, fv, nv = (int(m[k]) for k in ("first_triangle", "n_triangles", "first_vertex", "n_vertices"))
        W = world(m["pose"], vertices[fv:fv + nv])
        Ws.append(W[triangles[ft:ft + nt].astype(np.int64)].reshape(-1, 3, 3))
        oid.append(np.full(nt, int(m["object_id"]), np.uint32))
    return np.concatenate(oid), np.concatenate(Ws)


def _candidates(W, origin, res, shape):
    """index boxes lo, hi [n, 3] (inclusive, clipped; lo > hi: none) that hold every voxel whose centre lies within `res` of the
    world bounding box of triangle W[i]: the image of that box in the grid frame, rounded outwards (a centre that this
    rounding could lose lies `res` from the box, and no probe within h of a centre reaches further than h).  Bookkeeping of
    this restatement (which voxels it bothers to evaluate); every candidate is still put to the bounding-box test itself."""
    o = np.asarray(origin, np.float64).reshape(4, 4)
    inv = np.linalg.inv(o[:3, :3])
    lo_w, hi_w = W.min(1) - res, W.max(1) + res                          # [n, 3]
    mid, half = 0.5 * (lo_w + hi_w) - o[:3, 3], 0.5 * (hi_w - lo_w)
    g_mid, g_half = mid @ inv.T, half @ np.abs(inv).T
    lo = np.floor((g_mid - g_half) / res - 0.5).astype(np.int64)
    hi = np.ceil((g_mid + g_half) / res - 0.5).astype(np.int64)
    return np.maximum(lo, 0), np.minimum(hi, np.asarray(shape, np.int64) - 1)


def hits_at(meshes, vertices, triangles, origin, res, shape, ids=None, hit_any=None):
    """(filled, smallest-hit object ids (0: none)) per voxel in linear order; `ids` / `hit_any` given: accumulated onto them (OR,
    smallest non-zero).  Pairs of (triangle, voxel) are evaluated in batches; the order plays no part in the result."""
    if mesh_refusal(meshes, vertices, triangles, ids=False) is not None:
        raise ValueError("a mesh is refused")
    nx, ny, nz = shape
    n = nx * ny * nz
    h = res * 0.5
    ids = np.zeros(n, np.uint32) if ids is None else np.array(ids, np.uint32).reshape(-1)
    hit_any = np.zeros(n, bool) if hit_any is None else np.array(hit_any, bool).reshape(-1)
    oid, W = world_triangles(meshes, vertices, triangles)
    if not len(oid):
        return hit_any, ids
    lo, hi = _candidates(W, origin, res, shape)
    ext = np.maximum(hi - lo + 1, 0)
    count = ext.prod(1)
    order = np.flatnonzero(count > 0)
    start = 0
    while start < len(order):
        stop, pairs = start, 0
        while stop < len(order) and (stop == start or pairs + count[order[stop]] <= 1 << 20):
            pairs += count[order[stop]]
            stop += 1
        sel = order[start:stop]
        start = stop
        which = np.repeat(sel, count[sel])                                 # the triangle of each pair
        k = np.arange(len(which), dtype=np.int64) - np.repeat(np.cumsum(count[sel]) - count[sel], count[sel])
        e = ext[which]
        x = lo[which, 0] + k // (e[:, 1] * e[:, 2])
        y = lo[which, 1] + (k // e[:, 2]) % e[:, 1]
        z = lo[which, 2] + k % e[:, 2]
        v = (x * ny + y) * nz + z
        c = centres_of(origin, res, shape, v)
        Wp = W[which]
        near = np.all((c >= Wp.min(1) - res) & (c <= Wp.max(1) + res), axis=1)
        v, c, Wp, which = v[near], c[near], Wp[near], which[near]
        got = triangle(Wp, c, h)
        v, o = v[got], oid[which[got]]
        hit_any[v] = True
        # the smallest id per voxel: descending ids written in order leave the smallest
        by = np.argsort(-o.astype(np.int64), kind="stable")
        best = np.zeros(n, np.uint32)
        best[v[by]] = o[by]
        take = best != 0
        ids[take] = np.where(ids[take] == 0, best[take], np.minimum(ids[take], best[take]))
    return hit_any, ids


def hits_at_linear(meshes, vertices, triangles, origin, res, shape, linear):
    """(filled, smallest-hit ids) at chosen linear indices of a grid that may be too large to enumerate: every triangle against
    every such voxel whose centre lies within `res` of its world bounding box"""
    if mesh_refusal(meshes, vertices, triangles, ids=False) is not None:
        raise ValueError("a mesh is refused")
    c = centres_of(origin, res, shape, linear)
    ids, hit_any = np.zeros(len(c), np.uint32), np.zeros(len(c), bool)
    oid, W = world_triangles(meshes, vertices, triangles)
    for o, Wt in zip(oid, W):
        near = np.flatnonzero(np.all((c >= Wt.min(0) - res) & (c <= Wt.max(0) + res), axis=1))
        if len(near):
            got = near[triangle(Wt, c[near], res * 0.5)]
            hit_any[got] = True
            ids[got] = np.where(ids[got] == 0, o, np.minimum(ids[got], o))
    return hit_any, ids


def restated(meshes, vertices, triangles, origin, res, shape, onto=None):
    """(mask uint8 [nx, ny, nz], object ids uint32 [nx, ny, nz], bits uint32 [ceil(n / 32)]); onto = (mask, ids): accumulate"""
    filled, ids = hits_at(meshes, vertices, triangles, origin, res, shape, *((onto[1], onto[0]) if onto is not None else ()))
    mask = filled.astype(np.uint8).reshape(shape)
    return mask, ids.reshape(shape), pack_bits(mask)


def restated_shapes(shapes, origin, res, shape):
    """scene_raster_restated.restated for a shape list that may hold planes: first hit in list order"""
    c = centres(origin, res, shape)
    h = res * 0.5
    ids = np.zeros(len(c), np.uint32)
    hit_any = np.zeros(len(c), bool)
    for s in shapes:
        if int(s["type"]) == PLANE:
            if not plane_valid(s["dims"], s["pose"]):
                raise ValueError("plane refused")
            got = plane([float(v) for v in s["dims"]], s["pose"], c, h) & ~hit_any
        else:
            one_hit, _ = S.hits_at(np.asarray([s], dtype=shapes.dtype), c, res)
            got = one_hit & ~hit_any
        ids[got] = s["object_id"]
        hit_any |= got
    mask = hit_any.astype(np.uint8).reshape(shape)
    return mask, ids.reshape(shape), pack_bits(mask)
