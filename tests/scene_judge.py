"""An exact judge of the shape rasteriser's predicate (include/sdfgpu.h "Shape rasteriser"), in fractions.Fraction over the doubles
passed in, in the manner of frame_judge.py: voxel centres are exact, the shape frame comes from the exact inverse of the pose's
3 x 3 block, squared distances are compared and no root is taken.

THE EXACT PREDICATE.  M = the pose's 3 x 3 block, T its translation, N = M^-1 (exact), u_j the columns of M, C the exact centre
origin * (res (x + 1/2), ...), h = res / 2.  The solid is the image of the canonical solid under p -> M p + T, whatever M is.
  SPHERE    margin = r^2 - sum_a max(|C_a - T_a| - h, 0)^2.  (The kernel never reads M here; the judge takes the sphere as the
            world-frame ball, which is the image under any orthonormal M.)
  BOX       the image is a parallelepiped; cube against parallelepiped is decided exactly by 15 axes: e_a, the rows n_j of N, and
            e_a x u_j.  Per axis L: m_L = h sum_a |L_a| + sum_k b_k |u_k . L| - |(T - C) . L|; margin = min over the axes with
            L != 0 (an axis that is exactly 0 is skipped: 0 <= 0 + 0 separates nothing).
  CYLINDER  the corners C + (+-h, +-h, +-h) go to the shape frame by N; each face is clipped to |z| <= H / 2 (Sutherland-Hodgman,
            rational cut points); m_edge = r^2 - the least squared distance from the origin to the xy projection of a clipped edge
            (rational: the foot of the perpendicular is clamped to the segment).  m_axis: the segment T + s (H / 2) u_z, s in
            [-1, 1], against the cube by slabs, hi - lo in the parameter (and h - |C_a - T_a| on an axis the segment does not
            move along).  Filled iff m_edge >= 0 or m_axis >= 0: the cube meets the solid iff the projection of (cube and slab)
            comes within r of the axis, and that projection either contains the axis point (the segment passes through the cube)
            or is nearest to it on the projection of an edge of (cube and slab), every one of which is an edge of a clipped face.

THE ROUNDING BOUND (derived, not tuned; u = 2^-53, gamma_n ~ n u).  Magnitudes: S_a = sum_b |o_ab g_b| + |o_a3| for the centre's
row a, and L = sum_a (S_a + |T_a|) + 3 h + (the shape's extents: sum b_j, r, or r + H / 2).  Every coordinate, difference and
extent the kernel forms is at most L.
  centre: g_b = fl(res fl(x + 1/2)) is one rounding (x + 1/2 is exact), each row three products and three sums: a term passes at
    most 5 roundings, |c_a - C_a| <= gamma_5 S_a.
  orthonormality defect: the kernel uses M^T where the solid is defined through N, and the entries of M where the exact cross
    axes' radii have the cofactors of M.  D = max over rows of sum_j |(N - M^T)_ij| and of sum_j |(cof M - M)_ij|, computed
    exactly.  A shape-frame coordinate or an axis projection of a vector of 1-norm <= L moves by at most D L.
  SPHERE: three differences (2 roundings each on top of the centre's 5), three squares and two sums: each d_a within gamma_8 L,
    the sum of squares within 2 sqrt(3) L gamma_8 L + gamma_5 L^2 < 40 u L^2; r^2 is one rounding.  bound = 48 u L^2.
  BOX: an axis' margin is at most 9 products of magnitudes <= L with at most 8 roundings on any term on top of the centre's 5:
    gamma_13 * 3 L < 48 u L, plus the defect D L on the projections and 1 more D L on the radii.  bound = (48 u + 2 D) L.
  CYLINDER: a corner in the shape frame is within eps = (16 u + D) L (gamma_5 centre, 2 sums, the row's 5).  A cut point
    P = A + t (B - A) on a cube edge along world axis a has t = (plane - z_A) / (z_B - z_A) with |z_B - z_A| = 2 h |N_2a|, so
    it moves by eps + 3 eps / |N_2a| (a second-pass cut works on a part of the same edge: the same ratio).  kappa = the largest
    1 / |N_2a| over the axes with N_2a != 0, at least 1 (an edge with N_2a = 0 has equal z at both ends and is never cut).  A
    polygon vertex is within (1 + 3 kappa) eps; the least squared distance moves by at most 2 L times that, the clamped
    projection adds gamma_8 L^2.  bound_edge = (2 (1 + 3 kappa) (16 u + D) + 16 u) L^2.
    Slabs: s = fl((d -+ h) / g), g = fl((H / 2) M_a2): within gamma_8 L / |g| of the exact quotient; bound_axis = 16 u L / min |g|
    over the axes with g != 0, and 8 u L on the others.
  Shortcuts of the kernel: its rejection (|q_z| - H / 2 > 1.75 h or rho^2 > (r + 1.75 h)^2) leaves (1.75 - sqrt 3) h = 0.018 h
    between it and any cube that touches the solid, its acceptance (the centre is in the solid) is off by eps at the most while
    the cube reaches h around the centre: with eps < 0.001 h (asserted below) neither can contradict a margin beyond the bounds.
The judge returns margin / bound per (voxel, shape); |ratio| <= 1 is *ambiguous*: either answer passes.  For the cylinder the
ratio is max(m_edge / bound_edge, the least of the axis test's ratios).

ECONOMY.  A voxel whose float centre is further than h + extent + res from T on some axis, or further than 1.75 h from the solid
on one shape-frame coordinate (or radially), is empty (ratio -inf: the probe's circum-radius is 1.7321 h); one whose float centre
lies inside the solid by more than 0.01 res in the shape frame is filled (ratio +inf).  The slacks (res, 0.018 h, 0.01 res) are
~10^11 roundings (eps < 0.001 h is asserted).  Everything else is evaluated exactly.

FCL's answer on exact contact is UNVERIFIED (FCL and MoveIt are not available to this project): the predicate counts contact."""
from fractions import Fraction

import numpy as np

BOX, SPHERE, CYLINDER = 1, 2, 3
U = Fraction(1, 2 ** 53)
INF = float("inf")
F = Fraction


def _inverse3(M):
    c = [[M[(i + 1) % 3][(j + 1) % 3] * M[(i + 2) % 3][(j + 2) % 3] - M[(i + 1) % 3][(j + 2) % 3] * M[(i + 2) % 3][(j + 1) % 3]
          for j in range(3)] for i in range(3)]            # cofactors
    det = sum(M[0][j] * c[0][j] for j in range(3))
    if det == 0:
        raise ValueError("singular pose")
    return [[c[j][i] / det for j in range(3)] for i in range(3)], c


def _segment_dsq(a, b):
    ex, ey = b[0] - a[0], b[1] - a[1]
    ee = ex * ex + ey * ey
    t = F(0)
    if ee > 0:
        t = min(max(-(a[0] * ex + a[1] * ey) / ee, F(0)), F(1))
    qx, qy = a[0] + t * ex, a[1] + t * ey
    return qx * qx + qy * qy


def _clip(poly, sign, bound):
    out = []
    for k, cur in enumerate(poly):
        prv = poly[k - 1]
        cin, pin = sign * cur[2] <= bound, sign * prv[2] <= bound
        if cin != pin:
            t = (sign * bound - prv[2]) / (cur[2] - prv[2])
            out.append((prv[0] + t * (cur[0] - prv[0]), prv[1] + t * (cur[1] - prv[1]), sign * bound))
        if cin:
            out.append(cur)
    return out


class Shape:
    """the exact constants of one shape record"""

    def __init__(self, rec):
        self.kind = int(rec["type"])
        self.dims = [F(float(v)) for v in rec["dims"]]
        pose = np.asarray(rec["pose"], np.float64).reshape(4, 4)
        self.pose = pose
        self.M = [[F(float(pose[i, j])) for j in range(3)] for i in range(3)]
        self.T = [F(float(pose[i, 3])) for i in range(3)]
        self.N, cof = _inverse3(self.M)
        self.D = max(max(sum(abs(self.N[i][j] - self.M[j][i]) for j in range(3)) for i in range(3)),
                     max(sum(abs(cof[i][j] - self.M[i][j]) for j in range(3)) for i in range(3)))
        if self.kind == BOX:
            self.b = [d / 2 for d in self.dims]
            self.extent = sum(self.b)
            half = self.b
        elif self.kind == SPHERE:
            self.extent = self.dims[0]
            half = None
        elif self.kind == CYLINDER:
            self.hz, self.r = self.dims[0] / 2, self.dims[1]
            self.extent = self.r + self.hz
            half = [self.r, self.r, self.hz]
        else:
            raise ValueError("shape type %d is refused" % self.kind)
        # world half extents of the image's bounding box (floats, for the economy tests only)
        if half is None:
            self.world = np.array([float(self.dims[0])] * 3)
        else:
            self.world = np.abs(pose[:3, :3]) @ np.array([float(v) for v in half])
        self.Ninv = np.linalg.inv(pose[:3, :3])

    def deep_inside(self, c, slack):
        """float centres [n, 3] that lie inside the solid by more than `slack` (shape-frame distances; the frame is a near-isometry)"""
        q = (c - self.pose[:3, 3]) @ self.Ninv.T
        if self.kind == BOX:
            return np.all(np.abs(q) <= np.array([float(v) for v in self.b]) - slack, axis=1)
        if self.kind == SPHERE:
            return np.sqrt((q * q).sum(1)) <= float(self.dims[0]) - slack
        return (np.abs(q[:, 2]) <= float(self.hz) - slack) & (np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) <= float(self.r) - slack)


def _far_outside(s, c, reach):
    """float centres [n, 3] further than `reach` from the solid on one shape-frame coordinate (or radially)"""
    q = (c - s.pose[:3, 3]) @ s.Ninv.T
    if s.kind == BOX:
        return np.any(np.abs(q) - np.array([float(v) for v in s.b]) > reach, axis=1)
    if s.kind == SPHERE:
        return np.sqrt((q * q).sum(1)) - float(s.dims[0]) > reach
    return (np.abs(q[:, 2]) - float(s.hz) > reach) | (np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) - float(s.r) > reach)


def _ratio(s, C, h, L):
    """margin / bound of shape s at the exact centre C"""
    if s.kind == SPHERE:
        m = s.dims[0] * s.dims[0] - sum(max(abs(C[a] - s.T[a]) - h, F(0)) ** 2 for a in range(3))
        return m / (48 * U * L * L)
    if s.kind == BOX:
        t = [s.T[a] - C[a] for a in range(3)]
        u = [[s.M[a][j] for a in range(3)] for j in range(3)]            # columns
        e = [[F(int(a == k)) for k in range(3)] for a in range(3)]
        axes = e + [list(s.N[j]) for j in range(3)]
        for a in range(3):
            for j in range(3):
                x, y = e[a], u[j]
                axes.append([x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]])
        margins = []
        for Lx in axes:
            if not any(Lx):
                continue
            rc = h * sum(abs(v) for v in Lx)
            rb = sum(s.b[k] * abs(sum(u[k][i] * Lx[i] for i in range(3))) for k in range(3))
            margins.append(rc + rb - abs(sum(t[i] * Lx[i] for i in range(3))))
        return min(margins) / ((48 * U + 2 * s.D) * L)
    # CYLINDER
    eps = (16 * U + s.D) * L
    kappa = max([F(1)] + [1 / abs(s.N[2][a]) for a in range(3) if s.N[2][a] != 0])
    v = []
    for k in range(8):
        w = [C[a] + (h if (k >> a) & 1 else -h) - s.T[a] for a in range(3)]
        v.append(tuple(sum(s.N[j][a] * w[a] for a in range(3)) for j in range(3)))
    best = None
    for f in range(6):
        a = f >> 1
        a1, a2, base = (a + 1) % 3, (a + 2) % 3, (f & 1) << a
        poly = [v[base], v[base | (1 << a1)], v[base | (1 << a1) | (1 << a2)], v[base | (1 << a2)]]
        poly = _clip(_clip(poly, -1, s.hz), 1, s.hz)
        for k in range(len(poly)):
            d = _segment_dsq(poly[k - 1], poly[k])
            best = d if best is None or d < best else best
    bound_edge = (2 * (1 + 3 * kappa) * (16 * U + s.D) + 16 * U) * L * L
    ratio_edge = -INF if best is None else float((s.r * s.r - best) / bound_edge)
    lo, hi, ratio_axis = F(-1), F(1), INF
    gs = [s.hz * s.M[a][2] for a in range(3)]
    moving = [abs(g) for g in gs if g != 0]
    for a in range(3):
        d = C[a] - s.T[a]
        if gs[a] == 0:
            ratio_axis = min(ratio_axis, float((h - abs(d)) / (8 * U * L)))
        else:
            s1, s2 = (d - h) / gs[a], (d + h) / gs[a]
            lo, hi = max(lo, min(s1, s2)), min(hi, max(s1, s2))
    if moving:
        ratio_axis = min(ratio_axis, float((hi - lo) / (16 * U * L / min(moving))))
    assert eps < h / 1000, "the scene's magnitudes leave the kernel's shortcuts no room (eps >= 0.001 h)"
    return max(ratio_edge, ratio_axis)


def ratios(rec, origin, res, grid, linear):
    """margin / bound of one shape record at the voxels `linear` (int array) of grid (nx, ny, nz): float array; >= 0 means the exact
    predicate holds, |ratio| <= 1 is ambiguous, -inf / +inf are the economy's verdicts"""
    import scene_raster_restated as R
    s = Shape(rec)
    nx, ny, nz = grid
    linear = np.asarray(linear, np.int64)
    c = R.centres_of(origin, res, grid, linear)
    out = np.full(len(linear), -INF)
    t = s.pose[:3, 3]
    near = np.all(np.abs(c - t) <= res * 0.5 + s.world + res, axis=1)
    near &= ~_far_outside(s, c, 1.75 * res * 0.5)
    deep = near & s.deep_inside(c, 0.01 * res)
    out[deep] = INF
    O = [[F(float(v)) for v in row] for row in np.asarray(origin, np.float64).reshape(4, 4)[:3]]
    fres = F(float(res))
    h = fres / 2
    for i in np.flatnonzero(near & ~deep):
        vi = int(linear[i])
        tt, z = divmod(vi, nz)
        x, y = divmod(tt, ny)
        g = [fres * (F(x) + F(1, 2)), fres * (F(y) + F(1, 2)), fres * (F(z) + F(1, 2))]
        C = [O[a][0] * g[0] + O[a][1] * g[1] + O[a][2] * g[2] + O[a][3] for a in range(3)]
        S = sum(abs(O[a][0] * g[0]) + abs(O[a][1] * g[1]) + abs(O[a][2] * g[2]) + abs(O[a][3]) for a in range(3))
        L = S + sum(abs(v) for v in s.T) + 3 * h + s.extent
        out[i] = float(_ratio(s, C, h, L))
    return out


def scene_ratio(shapes, origin, res, grid, linear=None):
    """the largest ratio over the shapes, per voxel (all voxels by default)"""
    if linear is None:
        linear = np.arange(int(np.prod(grid)), dtype=np.int64)
    best = np.full(len(linear), -INF)
    for rec in shapes:
        best = np.maximum(best, ratios(rec, origin, res, grid, linear))
    return best


def check(mask, ratio, ties_only=False):
    """mask: the 0 / 1 answers at the judged voxels; ratio: scene_ratio there.  Raises on an answer the judge excludes.  With
    ties_only (exact scenes) the answer must be ratio >= 0 everywhere.  Returns (judged cells, ambiguous cells)."""
    mask = np.asarray(mask).reshape(-1).astype(bool)
    ratio = np.asarray(ratio).reshape(-1)
    assert mask.shape == ratio.shape
    if ties_only:
        wrong = mask != (ratio >= 0)
        ambiguous = np.zeros(len(mask), bool)
    else:
        wrong = (mask & (ratio < -1)) | (~mask & (ratio > 1))
        ambiguous = np.abs(ratio) <= 1
    assert not wrong.any(), "%d of %d cells contradict the exact predicate, first: index %d answer %d ratio %r" % (
        int(wrong.sum()), len(mask), int(np.flatnonzero(wrong)[0]), int(mask[np.flatnonzero(wrong)[0]]), float(ratio[np.flatnonzero(wrong)[0]]))
    return len(mask), int(ambiguous.sum())
