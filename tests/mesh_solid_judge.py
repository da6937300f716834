"""An exact judge of the solid fill (include/sdfgpu.h "Solid meshes"), in the manner of mesh_judge.py: exact rational arithmetic over
the doubles passed in, polynomials only -- no root, no division.

THE EXACT PREDICATE.  W_i = pose * v_i exactly (the solid is the image of the mesh under the pose as given), C the exact centre
origin * (res (x + 1/2), res (y + 1/2), res (z + 1/2), 1).  A voxel is filled iff mesh_judge's surface verdict holds (its probe meets
a triangle) or C is inside some mesh by the even-odd rule: a ray from C crosses an odd number of that mesh's triangles.

THE RAY.  The judge chooses the direction itself, from the fixed list DIRECTIONS (world frame, small integers in general position);
for a closed mesh the parity does not depend on it.  With e_j = det(D, A_j - C, A_{j+1} - C) over the triangle's edges and
n = (A_1 - A_0) x (A_2 - A_0): the LINE through C along D crosses the triangle's interior iff e_0, e_1, e_2 are all positive or all
negative; it misses the closed triangle iff two of them have strictly opposite signs; anything else is an exact degeneracy (the line
meets an edge or a vertex, or lies in the plane) and the voxel moves on to the next direction.  A proper crossing lies on the ray
iff sign(n . (A_0 - C)) sign(n . D) > 0.  A centre that lies ON a closed triangle (in its plane, on the inner side of every edge) is
found first, whatever the direction: the voxel is reported as on the surface and its parity is not used (the surface verdict
fills it: the probe contains its own centre).  A triangle with n = 0 has no area and takes no part.
Everything is a sign of a determinant of exact numbers: all coordinates are brought to one power-of-two denominator and the
arithmetic is Python's integers, vectorised over the voxels through numpy object arrays.

THE EXCUSE.  check() excuses exactly the cells that mesh_judge calls ambiguous (|ratio| <= 1) and nothing else.  This is a condition
on the scenes, not a measurement: the tests choose scenes for which the count is 0 and assert it."""
from fractions import Fraction

import numpy as np

import mesh_judge as J

F = Fraction
DIRECTIONS = [(97, 13, 41), (-31, 89, 17), (23, -47, 101), (5, 3, -113), (-71, -29, 37), (11, 103, -59), (1, 2, 3), (0, 0, 1)]


def _ints(values, scale):
    return np.array([int(v * scale) for v in values], dtype=object)


def _scale_of(fractions):
    scale = 1
    for v in fractions:
        if v.denominator > scale:
            scale = v.denominator                                            # (denominators are powers of two: the largest is the lcm)
    return scale


def _det3(a, b, c):
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0])


def _sign(a):
    return np.array([(v > 0) - (v < 0) for v in a.reshape(-1)], dtype=np.int64).reshape(a.shape)


def parity(meshes, vertices, triangles, origin, res, grid):
    """(inside bool [n], on_surface bool [n]) per voxel in linear order: inside some mesh by exact even-odd parity; centre exactly
    on a triangle"""
    nx, ny, nz = grid
    n = nx * ny * nz
    vertices = np.asarray(vertices, np.float64).reshape(-1, 3)
    triangles = np.asarray(triangles, np.uint32).reshape(-1, 3)
    O = [[F(float(v)) for v in row] for row in np.asarray(origin, np.float64).reshape(4, 4)[:3]]
    fres = F(float(res))
    # exact world vertices per mesh
    world = []
    for m in meshes:
        ft, nt, fv, nv = (int(m[k]) for k in ("first_triangle", "n_triangles", "first_vertex", "n_vertices"))
        P = [[F(float(v)) for v in row] for row in np.asarray(m["pose"], np.float64).reshape(4, 4)[:3]]
        W = [[P[a][0] * F(float(v[0])) + P[a][1] * F(float(v[1])) + P[a][2] * F(float(v[2])) + P[a][3] for a in range(3)] for v in vertices[fv:fv + nv]]
        world.append((W, triangles[ft:ft + nt].astype(np.int64)))
    # exact centres, separable: C_a = O_a0 gx[x] + O_a1 gy[y] + O_a2 gz[z] + O_a3
    g = [[fres * (F(i) + F(1, 2)) for i in range(k)] for k in (nx, ny, nz)]
    parts = [[[O[a][b] * v for v in g[b]] for b in range(3)] for a in range(3)]
    scale = _scale_of([v for W, _ in world for w in W for v in w] + [v for a in parts for b in a for v in b] + [O[a][3] for a in range(3)])
    C = []
    for a in range(3):
        px, py, pz = (_ints(parts[a][b], scale) for b in range(3))
        C.append(((px[:, None, None] + py[None, :, None]) + pz[None, None, :] + int(O[a][3] * scale)).reshape(-1))
    inside = np.zeros(n, bool)
    on_surface = np.zeros(n, bool)
    for W, tris in world:
        Wi = [[int(v * scale) for v in w] for w in W]
        odd = np.zeros(n, bool)
        # the centres that lie ON a closed triangle, whatever the direction: in its plane and on the inner side of every edge.  A
        # triangle with n = 0 has no area: no ray crosses it properly and it takes no part in the parity.
        normals, touching = [], np.zeros(n, bool)
        for tri in tris:
            f0 = [Wi[int(tri[1])][k] - Wi[int(tri[0])][k] for k in range(3)]
            f1 = [Wi[int(tri[2])][k] - Wi[int(tri[0])][k] for k in range(3)]
            nrm = [f0[1] * f1[2] - f0[2] * f1[1], f0[2] * f1[0] - f0[0] * f1[2], f0[0] * f1[1] - f0[1] * f1[0]]
            normals.append(nrm)
            if not any(nrm):
                continue
            A = [[Wi[int(i)][k] - C[k] for k in range(3)] for i in tri]
            in_plane = _sign((nrm[0] * A[0][0] + nrm[1] * A[0][1]) + nrm[2] * A[0][2]) == 0
            if in_plane.any():
                sel = np.flatnonzero(in_plane)
                As = [[a[sel] for a in row] for row in A]
                Nv = [np.array([v], dtype=object) for v in nrm]
                e = [_sign(_det3(Nv, As[j], As[(j + 1) % 3])) for j in range(3)]
                touching[sel[(np.minimum(np.minimum(e[0], e[1]), e[2]) >= 0)]] = True
        on_surface |= touching
        todo = np.flatnonzero(~touching)
        for D in DIRECTIONS:
            if not len(todo):
                break
            Ct = [c[todo] for c in C]
            count = np.zeros(len(todo), np.int64)
            degenerate = np.zeros(len(todo), bool)
            Dv = [np.array([d], dtype=object) for d in D]
            for tri, nrm in zip(tris, normals):
                if not any(nrm):
                    continue
                A = [[Wi[int(i)][k] - Ct[k] for k in range(3)] for i in tri]       # A_j - C
                e = [_sign(_det3(Dv, A[j], A[(j + 1) % 3])) for j in range(3)]
                least, most = np.minimum(np.minimum(e[0], e[1]), e[2]), np.maximum(np.maximum(e[0], e[1]), e[2])
                proper = (least == most) & (least != 0)
                misses = (least < 0) & (most > 0)
                degenerate |= ~proper & ~misses
                if proper.any():
                    nd = nrm[0] * D[0] + nrm[1] * D[1] + nrm[2] * D[2]
                    side = _sign((nrm[0] * A[0][0] + nrm[1] * A[0][1]) + nrm[2] * A[0][2]) * ((nd > 0) - (nd < 0))
                    count += proper & (side > 0)
            done = ~degenerate
            odd[todo[done]] = (count[done] & 1).astype(bool)
            todo = todo[~done]
        assert not len(todo), "every direction of the list is degenerate for %d voxels" % len(todo)
        inside |= odd & ~on_surface
    return inside, on_surface


def verdict(meshes, vertices, triangles, origin, res, grid):
    """(ratio of the surface judge [n], inside bool [n], on_surface bool [n])"""
    ratio = J.mesh_ratio(meshes, vertices, triangles, origin, res, grid)
    inside, on_surface = parity(meshes, vertices, triangles, origin, res, grid)
    return ratio, inside, on_surface


def check(mask, ratio, inside, on_surface, ties_as_hits=False):
    """asserts mask == (surface verdict OR parity) outside the cells the surface judge calls ambiguous; returns (judged, ambiguous).
    ties_as_hits: no allowance at all -- a surface ratio of exactly 0 is a hit, every other cell is decided by its sign"""
    mask = np.asarray(mask).reshape(-1).astype(bool)
    if ties_as_hits:
        ambiguous = np.zeros(len(mask), bool)
        expected = (ratio >= 0) | inside
    else:
        ambiguous = np.abs(ratio) <= 1.0
        expected = (ratio > 1.0) | inside
    assert not (on_surface & ~ambiguous & ~(ratio >= 0)).any(), "a centre on a triangle whose probe misses it"
    wrong = np.flatnonzero((mask != expected) & ~ambiguous)
    assert not len(wrong), "%d cells differ from the exact judge, the first at linear index %d (mask %d, ratio %r, inside %d)" % (
        len(wrong), wrong[0], mask[wrong[0]], ratio[wrong[0]], inside[wrong[0]])
    return len(mask), int(ambiguous.sum())
