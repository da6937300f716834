"""An exact judge of the triangle's and the plane's predicates (include/sdfgpu.h "Planes and triangle meshes"), in
fractions.Fraction over the doubles passed in, in the manner of scene_judge.py.  Every quantity is a polynomial of the inputs: no
root, no division.

THE EXACT PREDICATE.  W_i = pose * v_i (exact; the solid is the image under the pose as given, whatever its 3 x 3 block is),
C the exact centre origin * (res (x + 1/2), ...), h = res / 2, u_i = W_i - C, f_j = W_{j+1} - W_j, n = f_0 x f_1.
  TRIANGLE  a closed triangle (or segment, or point) and the closed cube are convex: they are disjoint iff one of the thirteen axes
            e_a, n, e_a x f_j separates them (for a segment the axes e_a and e_a x f suffice, for a point the e_a, and those are
            among the thirteen; the others are exactly 0 then).  Per axis L != 0:
            m_L = h sum_a |L_a| - max(min_i L . u_i, -max_i L . u_i); an axis that is exactly 0 is skipped (0 > 0 separates nothing).
            Filled iff every m_L >= 0.
  PLANE     N = R n_shape, s = N . (C - T); m = h sum_a |N_a| - |s|: the cube's extent along N against the centre's distance.

THE ROUNDING BOUND (derived, not tuned; u = 2^-53, gamma_k ~ k u).  Magnitudes: S = sum_a (sum_b |o_ab g_b| + |o_a3|) for the
centre, P = max over the triangle's vertices of sum_a (sum_b |p_ab v_b| + |p_a3|), and M = S + P + 3 h: every coordinate of W, c
and u is at most M in magnitude, every edge component at most 2 M.
  centre: as in scene_judge.py, |c_a - C_a| <= gamma_5 S.  W: three products and three sums, a term passes at most 4 roundings:
    |W - W^| <= gamma_4 P.  u = fl(W^ - c^): within gamma_4 P + gamma_5 S + u M <= 10 u M.  f = fl(W^_{j+1} - W^_j): within
    2 gamma_4 P + 2 u M <= 10 u M.
  e_a: p = u_a, r = h (exact).  bound = 10 u M.
  e_a x f_j: p = fl(fl(u_a2 f_a1) - fl(u_a1 f_a2)).  A product of factors within 10 u M of (<= M) and (<= 2 M) is within
    10 u M * 2 M + M * 10 u M + u * 2 M^2 = 32 u M^2; two of them and the difference's own rounding (u * 4 M^2): 68 u M^2.
    r = fl(h fl(|f_a2| + |f_a1|)): within h (20 u M + 2 u * 4 M) = 28 u h M <= 28 u M^2.  bound = 128 u M^2 >= 96 u M^2.
  n: a component is the difference of two products of edge components: 2 (2 M * 10 u M * 2 + u * 4 M^2) + u * 8 M^2 = 96 u M^2,
    and |n_k| <= 8 M^2.  p = fl(fl(fl(n_0 u_0) + fl(n_1 u_1)) + fl(n_2 u_2)): a term is within 96 u M^2 * M + 8 M^2 * 10 u M plus
    three roundings of at most 8 M^3 = 200 u M^3; three terms: 600 u M^3.  r: h (3 * 96 u M^2 + 3 u * 24 M^2) = 360 u h M^2.
    bound = 1024 u M^3 >= 960 u M^3.
  PLANE: with Q = sum_a sum_k |r_ak n_k| and M = S + sum_a |T_a| + 3 h: N within gamma_3 Q <= 4 u Q; c - T within
    gamma_5 S + u M <= 6 u M; a product N_a (c_a - T_a) within 4 u Q M + Q 6 u M + u Q M, three of them and two sums: 40 u Q M;
    r = fl(h fl(fl(|N_0| + |N_1|) + |N_2|)) within h (12 u Q + 3 u * 3 Q) <= 24 u Q M.  bound = 64 u Q M.
The judge returns min over the axes of m_L / bound_L per (voxel, triangle), the largest over the triangles per voxel;
|ratio| <= 1 is *ambiguous*: either answer passes.  An axis whose exact value is 0 may come out of the kernel's arithmetic as a tiny
non-zero vector; along ANY direction a cube and a triangle that meet are not separated, so such an axis can only move a verdict
within the roundings bounded above.

ECONOMY.  A triangle is judged at the voxels whose float centres lie within `res` of its world bounding box on every axis (a probe
that meets it has its centre within h of that box); elsewhere the ratio is -inf.  There the same margins are first taken in
floats: a float ratio below -10^6 on some axis gives -inf, above 10^6 on every axis +inf (the float margin is within one bound of
the exact one, by the derivation above); everything else is evaluated exactly.

FCL's answers -- that a mesh is its surface, that a plane has no thickness, and that contact counts -- are UNVERIFIED (FCL and
MoveIt are not available to this project)."""
from fractions import Fraction

import numpy as np

import mesh_raster_restated as R

U = Fraction(1, 2 ** 53)
INF = float("inf")
F = Fraction
BIG = 1.0e6


def _fr(a):
    return [F(float(v)) for v in np.asarray(a, np.float64).reshape(-1)]


def _axes_exact(W, C, h):
    """[(margin, kind)] over the non-zero axes; kind 1, 2, 3: the power of M in the bound"""
    u = [[W[i][k] - C[k] for k in range(3)] for i in range(3)]
    f = [[W[(j + 1) % 3][k] - W[j][k] for k in range(3)] for j in range(3)]
    n = [f[0][1] * f[1][2] - f[0][2] * f[1][1], f[0][2] * f[1][0] - f[0][0] * f[1][2], f[0][0] * f[1][1] - f[0][1] * f[1][0]]
    axes = [([F(int(a == k)) for k in range(3)], 1) for a in range(3)] + [(n, 3)]
    for a in range(3):
        a1, a2 = (a + 1) % 3, (a + 2) % 3
        for j in range(3):
            L = [F(0)] * 3
            L[a1], L[a2] = -f[j][a2], f[j][a1]
            axes.append((L, 2))
    out = []
    for L, kind in axes:
        if not any(L):
            continue
        p = [sum(L[k] * u[i][k] for k in range(3)) for i in range(3)]
        out.append((h * sum(abs(v) for v in L) - max(min(p), -max(p)), kind))
    return out


_BOUND = {1: 10, 2: 128, 3: 1024}


def _float_ratios(W, c, h, M):
    """the same margins in floats, over centres c [n, 3]: (least ratio, greatest-lower-bound flag) per centre"""
    f, n = R.triangle_constants(W)
    u = [[W[i, k] - c[:, k] for k in range(3)] for i in range(3)]
    least = np.full(len(c), INF)

    def take(p, r, kind):
        nonlocal least
        m = r - np.maximum(np.minimum(np.minimum(p[0], p[1]), p[2]), -np.maximum(np.maximum(p[0], p[1]), p[2]))
        least = np.minimum(least, m / (_BOUND[kind] * 2.0 ** -53 * M ** kind))

    for a in range(3):
        take([u[i][a] for i in range(3)], h, 1)
    take([(n[0] * u[i][0] + n[1] * u[i][1]) + n[2] * u[i][2] for i in range(3)], h * ((abs(n[0]) + abs(n[1])) + abs(n[2])), 3)
    for a in range(3):
        a1, a2 = (a + 1) % 3, (a + 2) % 3
        for j in range(3):
            take([u[i][a2] * f[j][a1] - u[i][a1] * f[j][a2] for i in range(3)], h * (abs(f[j][a2]) + abs(f[j][a1])), 2)
    return least


def _exact_centre(O, fres, grid, vi):
    nx, ny, nz = grid
    tt, z = divmod(int(vi), nz)
    x, y = divmod(tt, ny)
    g = [fres * (F(x) + F(1, 2)), fres * (F(y) + F(1, 2)), fres * (F(z) + F(1, 2))]
    C = [O[a][0] * g[0] + O[a][1] * g[1] + O[a][2] * g[2] + O[a][3] for a in range(3)]
    S = sum(abs(O[a][0] * g[0]) + abs(O[a][1] * g[1]) + abs(O[a][2] * g[2]) + abs(O[a][3]) for a in range(3))
    return C, S


def mesh_ratio(meshes, vertices, triangles, origin, res, grid):
    """the largest over the triangles of (the least margin / bound over the axes), per voxel of the grid"""
    n = int(np.prod(grid))
    c = R.centres(origin, res, grid)
    best = np.full(n, -INF)
    O = [[F(float(v)) for v in row] for row in np.asarray(origin, np.float64).reshape(4, 4)[:3]]
    fres = F(float(res))
    h = fres / 2
    vertices = np.asarray(vertices, np.float64).reshape(-1, 3)
    triangles = np.asarray(triangles, np.uint32).reshape(-1, 3)
    S_float = float(np.abs(np.asarray(origin, np.float64).reshape(4, 4)[:3, :3]).sum() * res * (max(grid) + 1) + np.abs(np.asarray(origin)[:3, 3]).sum())
    centre_cache = {}
    for m in meshes:
        ft, nt, fv = int(m["first_triangle"]), int(m["n_triangles"]), int(m["first_vertex"])
        pose = np.asarray(m["pose"], np.float64).reshape(4, 4)
        Pf = [[F(float(v)) for v in row] for row in pose[:3]]
        for tri in triangles[ft:ft + nt]:
            v = vertices[fv + tri.astype(np.int64)]
            Wf = R.world(pose, v)
            near = np.flatnonzero(np.all((c >= Wf.min(0) - res) & (c <= Wf.max(0) + res), axis=1))
            if not len(near):
                continue
            vx = [_fr(row) for row in v]
            W = [[Pf[a][0] * vx[i][0] + Pf[a][1] * vx[i][1] + Pf[a][2] * vx[i][2] + Pf[a][3] for a in range(3)] for i in range(3)]
            P = max(sum(abs(Pf[a][0] * vx[i][0]) + abs(Pf[a][1] * vx[i][1]) + abs(Pf[a][2] * vx[i][2]) + abs(Pf[a][3]) for a in range(3))
                    for i in range(3))
            # floats first, with a magnitude at least the exact M of every voxel: the bounds only grow with it, the ratios shrink
            M_float = S_float + float(P) + 3.0 * float(h)
            quick = _float_ratios(Wf, c[near], float(h), M_float * 1.001)
            ratio = np.where(quick < -BIG, -INF, np.where(quick > BIG, INF, np.nan))
            for k in np.flatnonzero(np.isnan(ratio)):
                vi = int(near[k])
                if vi not in centre_cache:
                    centre_cache[vi] = _exact_centre(O, fres, grid, vi)
                C, S = centre_cache[vi]
                M = S + P + 3 * h
                ratio[k] = float(min(mg / (_BOUND[kind] * U * M ** kind) for mg, kind in _axes_exact(W, C, h)))
            best[near] = np.maximum(best[near], ratio)
    return best


def plane_ratio(rec, origin, res, grid):
    """margin / bound of one plane record per voxel, all exact (one inequality)"""
    n = int(np.prod(grid))
    pose = np.asarray(rec["pose"], np.float64).reshape(4, 4)
    Pf = [[F(float(v)) for v in row] for row in pose[:3]]
    nn = _fr(rec["dims"])[:3]
    N = [Pf[a][0] * nn[0] + Pf[a][1] * nn[1] + Pf[a][2] * nn[2] for a in range(3)]
    Q = sum(abs(Pf[a][k] * nn[k]) for a in range(3) for k in range(3))
    T = [Pf[a][3] for a in range(3)]
    O = [[F(float(v)) for v in row] for row in np.asarray(origin, np.float64).reshape(4, 4)[:3]]
    fres = F(float(res))
    h = fres / 2
    # floats first, as for the triangles
    c = R.centres(origin, res, grid)
    Nf = np.array([float(v) for v in N])
    s = (c - pose[:3, 3]) @ Nf
    M_float = float(np.abs(c).max() + np.abs(pose[:3, 3]).sum() + np.abs(np.asarray(origin)[:3, 3]).sum() + 3 * float(h)) * 3.0
    quick = (float(h) * np.abs(Nf).sum() - np.abs(s)) / (64 * 2.0 ** -53 * float(Q) * M_float)
    out = np.where(quick < -BIG, -INF, np.where(quick > BIG, INF, np.nan))
    for vi in np.flatnonzero(np.isnan(out)):
        C, S = _exact_centre(O, fres, grid, vi)
        M = S + sum(abs(v) for v in T) + 3 * h
        margin = h * sum(abs(v) for v in N) - abs(sum(N[a] * (C[a] - T[a]) for a in range(3)))
        out[vi] = float(margin / (64 * U * Q * M))
    assert out.shape == (n,)
    return out


def check(mask, ratio, ties_only=False):
    import scene_judge
    return scene_judge.check(mask, ratio, ties_only)
