"""The solid fill of closed meshes (include/sdfgpu.h "Solid meshes", sdf_tools_amd/csrc/sdfgpu_mesh_solid.hpp) restated in numpy
float64, operation for operation what ms_grid, ms_orient, ms_edge, ms_crossing and ms_first_above do, vectorised over the columns.
The surface part (a) is mesh_raster_restated's, unchanged.

The exact sign of the orientation determinant is taken here with the same floating filter and, where that does not decide, with
fractions.Fraction: an exact sign is an exact sign, however it is reached (the kernel's expansion arithmetic is compared with
Fraction directly in test_mesh_solid_cpu.py).

What is NOT restated is the culling (ms_column_box).  A triangle is evaluated at the columns whose centres lie in the closed
bounding rectangle of its grid vertices: a centre strictly outside it is covered under no tie rule.

restated() returns the byte mask, the smallest-id field and the packed bit field, as mesh_raster_restated.restated does.
toggles_of() gives one mesh's crossings per cell for chosen columns, parity_of() and inside_at_columns() their prefix parity: over
the whole grid, and over a window of columns of a grid too large to enumerate."""
from fractions import Fraction

import numpy as np

import mesh_raster_restated as R

pack_bits = R.pack_bits


def inverse(origin):
    """the inverse of the origin's 3 x 3 block by cofactors, as check_mesh_args has it; None when it has none"""
    o = [float(v) for v in np.asarray(origin, np.float64).reshape(-1)]
    c00, c01, c02 = o[5] * o[10] - o[6] * o[9], o[6] * o[8] - o[4] * o[10], o[4] * o[9] - o[5] * o[8]
    with np.errstate(all="ignore"):
        det = np.float64(o[0] * c00 + o[1] * c01 + o[2] * c02)
        inv = np.array([c00 / det, (o[2] * o[9] - o[1] * o[10]) / det, (o[1] * o[6] - o[2] * o[5]) / det,
                        c01 / det, (o[0] * o[10] - o[2] * o[8]) / det, (o[2] * o[4] - o[0] * o[6]) / det,
                        c02 / det, (o[1] * o[8] - o[0] * o[9]) / det, (o[0] * o[5] - o[1] * o[4]) / det], np.float64)
    if not (np.isfinite(det) and det != 0.0 and np.isfinite(inv).all()):
        return None
    return inv


def grid_vertices(inv, origin, W):
    """ms_grid: W [..., 3] world -> grid coordinates, rows as (i0 d0 + i1 d1) + i2 d2"""
    o = np.asarray(origin, np.float64).reshape(4, 4)
    W = np.asarray(W, np.float64)
    d = [W[..., k] - o[k, 3] for k in range(3)]
    return np.stack([(inv[3 * k] * d[0] + inv[3 * k + 1] * d[1]) + inv[3 * k + 2] * d[2] for k in range(3)], -1)


def orient_exact(P, Q, C):
    """the sign of (P_x - C_x)(Q_y - C_y) - (P_y - C_y)(Q_x - C_x) over the doubles, exactly"""
    px, py, qx, qy, cx, cy = (Fraction(float(v)) for v in (P[0], P[1], Q[0], Q[1], C[0], C[1]))
    d = (px - cx) * (qy - cy) - (py - cy) * (qx - cx)
    return (d > 0) - (d < 0)


def orient(P, Q, C):
    """ms_orient: P, Q [2], C [n, 2] -> (exact signs int [n], values float64 [n])"""
    with np.errstate(all="ignore"):
        l = (P[0] - C[:, 0]) * (Q[1] - C[:, 1])
        r = (P[1] - C[:, 1]) * (Q[0] - C[:, 0])
        det = l - r
        total = np.abs(l) + np.abs(r)
        sure = (total >= 2.0 ** -900) & (total <= 2.0 ** 1000) & (np.abs(det) > 2.0 ** -50 * total)
    sign = np.where(det > 0.0, 1, -1)
    for i in np.flatnonzero(~sure):
        sign[i] = orient_exact(P, Q, C[i])
    return sign, det


def edge(P, Q, C):
    """ms_edge: the endpoints in lexicographic order, zeros by the top-left rule, negated when the order swapped them"""
    swap = Q[0] < P[0] or (Q[0] == P[0] and Q[1] < P[1])
    a, b = (Q, P) if swap else (P, Q)
    s, w = orient(a, b, C)
    tie = 1 if a[1] > b[1] else -1 if a[1] < b[1] else 1 if b[0] > a[0] else 0
    s = np.where(s == 0, tie, s)
    return (-s, -w) if swap else (s, w)


def crossing(G, C):
    """ms_crossing: G [3, 3] grid vertices, C [n, 2] column centres -> (covered bool [n], z_c float64 [n])"""
    s0, w0 = edge(G[1], G[2], C)
    s1, w1 = edge(G[2], G[0], C)
    s2, w2 = edge(G[0], G[1], C)
    covered = (s0 != 0) & (s0 == s1) & (s1 == s2)
    zmin, zmax = min(min(G[0][2], G[1][2]), G[2][2]), max(max(G[0][2], G[1][2]), G[2][2])
    with np.errstate(all="ignore"):
        z = ((w0 * G[0][2] + w1 * G[1][2]) + w2 * G[2][2]) / ((w0 + w1) + w2)
    z = np.where(z >= zmin, z, zmin)
    return covered, np.where(z <= zmax, z, zmax)


def toggles_of(W, origin, res, shape, xs=None, ys=None):
    """the crossings of ONE mesh with world triangles W [n, 3, 3], counted at the first cell above each: int64 [len(xs), len(ys), nz + 1]
    for the columns xs x ys (index arrays; default: every column).  Entry nz counts the crossings above the last centre."""
    nx, ny, nz = shape
    inv = inverse(origin)
    if inv is None:
        raise ValueError("the origin has no inverse")
    G = grid_vertices(inv, origin, W)
    if not np.isfinite(G).all():
        raise ValueError("a mesh is refused")
    xs = np.arange(nx, dtype=np.int64) if xs is None else np.asarray(xs, np.int64).reshape(-1)
    ys = np.arange(ny, dtype=np.int64) if ys is None else np.asarray(ys, np.int64).reshape(-1)
    cx, cy = res * (xs.astype(np.float64) + 0.5), res * (ys.astype(np.float64) + 0.5)
    cz = res * (np.arange(nz, dtype=np.float64) + 0.5)
    toggles = np.zeros((len(xs), len(ys), nz + 1), np.int64)
    for g in G:
        ix = np.flatnonzero((cx >= g[:, 0].min()) & (cx <= g[:, 0].max()))
        iy = np.flatnonzero((cy >= g[:, 1].min()) & (cy <= g[:, 1].max()))
        if not len(ix) or not len(iy):
            continue
        X, Y = (a.reshape(-1) for a in np.meshgrid(ix, iy, indexing="ij"))
        covered, zc = crossing([[float(v) for v in row] for row in g], np.stack([cx[X], cy[Y]], 1))
        cell = np.searchsorted(cz, zc[covered], side="right")                # the number of centres <= z_c: the first one above
        np.add.at(toggles, (X[covered], Y[covered], cell), 1)
    return toggles


def inside_at_columns(W, origin, res, shape, xs, ys):
    """parity_of for a window of columns with full z: bool [len(xs), len(ys), nz] (a grid too large to enumerate)"""
    return (np.cumsum(toggles_of(W, origin, res, shape, xs, ys)[:, :, :shape[2]], axis=2) & 1).astype(bool)


def parity_of(W, origin, res, shape):
    """the cells inside ONE mesh with world triangles W [n, 3, 3] by the even-odd rule: bool [nx, ny, nz]"""
    return (np.cumsum(toggles_of(W, origin, res, shape)[:, :, :shape[2]], axis=2) & 1).astype(bool)


def restated(meshes, vertices, triangles, origin, res, shape, onto=None):
    """(mask uint8 [nx, ny, nz], object ids uint32 [nx, ny, nz], bits uint32 [ceil(n / 32)]); onto = (mask, ids): accumulate"""
    filled, ids = R.hits_at(meshes, vertices, triangles, origin, res, shape, *((onto[1], onto[0]) if onto is not None else ()))
    filled, ids = filled.reshape(shape).copy(), ids.reshape(shape).copy()
    vertices = np.asarray(vertices, np.float64).reshape(-1, 3)
    triangles = np.asarray(triangles, np.uint32).reshape(-1, 3)
    for m in meshes:
        _, W = R.world_triangles([m], vertices, triangles)
        if not len(W):
            continue
        inside = parity_of(W, origin, res, shape)
        oid = np.uint32(m["object_id"])
        ids[inside] = np.where(ids[inside] == 0, oid, np.minimum(ids[inside], oid))
        filled |= inside
    mask = filled.astype(np.uint8)
    return mask, ids, pack_bits(mask)
