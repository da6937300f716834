"""Frames that exercise every entry of a caller-supplied transform, and an exact judge of sdfgpu_query_points in such frames.

A frame built by test_projection_cpu.rigid() turns about z: w2g[2], w2g[6], w2g[8], w2g[9] and rot[2], rot[5], rot[6], rot[7] are
zero, so a layer that exchanges two of them or drops the z coupling gives the same bits.  frames() names origins that do not have
that blind spot; judge() says what k_query_points must answer in any of them, computed in fractions.Fraction over the doubles and
floats involved (exact), with two derived tolerances and no other.

Notation: u = 2^-53; W = world_to_grid (3 x 4), R = grid_to_world_rotation (3 x 3), p the world point, all as the doubles the
kernel receives; G = W (p, 1) and Q = G / res exactly; S_i = sum_j |w_ij p_j| + |w_i3|, S = max_i S_i.

The cell.  The kernel computes gx = fl(fl(fl(fl(w0 px) + fl(w1 py)) + fl(w2 pz)) + w3): the first product passes four roundings
(its own and three sums), so |gx - G_x| <= gamma_4 S_x, gamma_n = n u / (1 - n u).  Then q = fl(gx fl(1 / res)) adds one rounded
reciprocal and one rounded product: |q - Q_x| <= (gamma_4 + gamma_2 (1 + gamma_4)) S_x / res < 8 u S_x / res = delta_x, since
|G_x| <= S_x.  A point whose Q_i is further than delta_i from every integer has one possible cell, floor(Q); a point within
delta_i of an integer is *ambiguous* on that axis, and the kernel may answer from either neighbour (up to 8 candidates, of which
some may lie outside the grid: flags 0, oob_value, NaN gradient).

The gradient.  The kernel reads the grid-frame gradient of its cell, analysis_scenes.grid_gradient(sdf, res, edge)[cell] (pinned
bit for bit elsewhere, the interior's float32 difference included), and rotates it as fl(fl(fl(r0 g0) + fl(r1 g1)) + fl(r2 g2)):
three products and two sums, at most three roundings on any term, so every component lies within gamma_3 sum_j |R_ij| |g_j| <
4 u sum_j |R_ij| |g_j| of the exact R g.  A non-finite grid gradient leaves no rounding to bound (every component is an infinity
or a NaN whatever the rounding), so there the double evaluation itself is the expectation.

The distance.  EstimateDistance4d (sdf.hpp:773-902, as analysis_scenes.estimate_distance and k_query_points state it): per axis
the neighbour pair on the offset's side of the cell centre (shifted inward at a grid face, collapsed on a singleton axis), the
8 values D_c = f_c -+ res / 2, and the trilinear form sum_c D_c prod_i w_i with w_i in {1 - t_i, t_i}, t_i = (G_i - L_i) / res
and L_i the lower neighbour's centre.  The judge evaluates this exactly at the exact G.  The estimate is continuous across a
cell face (both sides use the same pair) and across a cell centre (both pairs interpolate to the centre's value: a kernel whose
rounded offset has the other sign is off by |offset| / res <= 4 u S / res times a difference of neighbouring values, well inside
the tolerance), so neither kind of ambiguity needs a second candidate; for an ambiguous point on an outer face the judge
evaluates from the candidate cell inside the grid.  Tolerance: each 1-D weight carries an absolute error of about 6 u S / res
(gx's gamma_4 S / res, the rounded lower centre, the difference and the product with the rounded multiplier); three weights of
magnitude at most 1.5 (half a cell of extrapolation) give 3 * 1.5^2 * 6 u S / res ~ 42 u S / res on a trilinear weight; the
about 20 roundings between the corner values and the result, at a weight sum of at most 1.5^3 = 3.4, give 68 u.  Both factors are
rounded to 64: |distance - exact| <= 64 u (1 + S / res) sum_c |D_c| over the 8 corner values.  The bound is derived, not tuned: a
result beyond it is a finding.  A point with a non-finite corner value has no exact estimate and its distance is not judged
(check() counts them as `unjudged`; the fields of the tests have none).

A point with a non-finite coordinate is outside: flags 0, oob_value, NaN gradient."""
import itertools
import math
from fractions import Fraction

import numpy as np

import analysis_scenes as A
import resample_restated
from test_projection_cpu import inverse

U = Fraction(1, 2 ** 53)
N_UNIFORM, N_LATTICE, N_CENTRES, N_BAD = 2000, 64, 64, 2
AMBIGUITY_CAP = 0.005                     # of the uniform points (a condition on the tests' points; 0 is expected)

# the fields of the GPU cases: Bernoulli 0.1 masks, anisotropic so that an axis mix-up changes which points are inside
FIELDS = [((13, 9, 21), 0.05), ((40, 33, 48), 0.05), ((1, 1, 9), 0.3), ((20, 40, 1), 0.1)]


def _with(R, t):
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = t
    return m


def frames():
    """name -> 4 x 4 origin (grid -> world)"""
    c, s = math.cos(0.6), math.sin(0.6)
    cyc = [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    return {
        # controls: the grid coordinates are exact, so the kernel is bit-equal to analysis_scenes.query_points
        "identity": np.eye(4),
        "translation": _with(np.eye(3), (0.1, -0.37, 2.3)),
        # all nine rotation entries nonzero and distinct: any transposition, exchanged pair or dropped term moves the result
        "general": resample_restated.quaternion_origin((0.83, -0.21, 0.4, 0.32), (-1.7, 0.45, 0.9)),
        # the z couplings that a turn about z leaves at zero: entries [1][2], [2][1] ...
        "about-x": _with([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]], (0.3, -1.1, 0.6)),
        # ... and [0][2], [2][0] (w2g[2], w2g[8], rot[2], rot[6])
        "about-y": _with([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], (-0.8, 0.2, 1.4)),
        # x -> y -> z -> x: entries exactly 0 or 1 and R != R^T, so a transposed matrix sends every point to another cell, and
        # 1 x + 0 y + 0 z + t is one rounding, so the double arithmetic is trivial to reason about
        "cyclic": _with(cyc, (0.25, -1.5, 0.75)),
        # its inverse (x -> z -> y -> x): the transposed block, so that neither storage order is the lucky one
        "cyclic-inverse": _with(np.transpose(cyc), (-0.5, 1.25, 2.0)),
    }


def transforms(origin):
    """(world_to_grid 3 x 4, grid_to_world_rotation 3 x 3) of an origin, the inverse in eigen_lite's element order"""
    origin = np.asarray(origin, np.float64)
    return inverse(origin)[:3].copy(), origin[:3, :3].copy()


def to_world(origin, g):
    """origin * (g, 1) in doubles, eigen_lite's order"""
    o = np.asarray(origin, np.float64)
    g = np.asarray(g, np.float64)
    return np.stack([o[i, 0] * g[:, 0] + o[i, 1] * g[:, 1] + o[i, 2] * g[:, 2] + o[i, 3] for i in range(3)], 1)


def case_points(shape, res, origin, seed):
    """World-frame points of one GPU case: N_UNIFORM uniform over the grid and a 10 % margin (drawn in the grid frame), N_LATTICE
    grid-frame multiples of res (cell corners, the grid's own 8 first: ambiguous by construction), N_CENTRES exact cell centres,
    a NaN row and an inf row.  Returns (points, slices by name)."""
    rng = np.random.default_rng(seed)
    size = np.asarray(shape, np.float64) * res
    uniform = rng.uniform(-0.1, 1.1, (N_UNIFORM, 3)) * size
    corners = [[a * shape[0], b * shape[1], c * shape[2]] for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    k = np.asarray(corners + [[int(rng.integers(0, s + 1)) for s in shape] for _ in range(N_LATTICE - 8)], np.float64)
    centres = np.asarray([[int(rng.integers(0, s)) for s in shape] for _ in range(N_CENTRES)], np.float64) + 0.5
    world = to_world(origin, np.concatenate([uniform, k * res, centres * res]))
    bad = np.array([[math.nan, 0.5, 0.5], [0.5, math.inf, 0.5]])
    pts = np.concatenate([world, bad])
    a, b, c = N_UNIFORM, N_UNIFORM + N_LATTICE, N_UNIFORM + N_LATTICE + N_CENTRES
    return pts, {"uniform": slice(0, a), "lattice": slice(a, b), "centres": slice(b, c), "bad": slice(c, c + N_BAD)}


def case_mask(shape):
    """the Bernoulli 0.1 mask of a field: the first seed that leaves both classes (so no distance is infinite)"""
    from sdf_tools_amd import synth
    for seed in range(1, 64):
        m = synth.bernoulli_mask(shape, 0.1, seed)
        if 0 < int(m.sum()) < m.size:
            return m
    raise ValueError("no seed gives both classes")


def case_seed(frame, shape):
    return 1000 * sorted(frames()).index(frame) + [s for s, _ in FIELDS].index(tuple(shape))


def emulate(sdf, res, w2g, rot, points, oob=np.inf, edge=False):
    """A double emulation of k_query_points: the four-term sums, analysis_scenes.query_points at those grid coordinates, and rot
    applied as r0 g0 + r1 g1 + r2 g2 (numpy never fuses a product with a sum)."""
    w, r, p = np.asarray(w2g, np.float64).reshape(3, 4), np.asarray(rot, np.float64).reshape(3, 3), np.asarray(points, np.float64)
    with np.errstate(invalid="ignore"):
        g = np.stack([w[i, 0] * p[:, 0] + w[i, 1] * p[:, 1] + w[i, 2] * p[:, 2] + w[i, 3] for i in range(3)], 1)
        dist, gg, flags = A.query_points(sdf, res, g, oob, edge)
        grad = np.stack([r[i, 0] * gg[:, 0] + r[i, 1] * gg[:, 1] + r[i, 2] * gg[:, 2] for i in range(3)], 1)
    return dist, grad, flags


def _axis_pair(i, n, off):
    """sdf.hpp:798-833 with an exact offset"""
    lo = hi = i
    if off >= 0:
        hi = i + 1
        if hi >= n:
            hi, lo = i, i - 1
            if lo < 0:
                lo = i
    else:
        lo = i - 1
        if lo < 0:
            hi, lo = i + 1, i
            if hi >= n:
                hi = i
    return lo, hi


class _Point:
    __slots__ = ("finite", "axes", "ambiguous", "S", "estimate", "tolerance")


class Exact:
    """What does not depend on `edge` or on oob_value: per point the candidate cells, the exact estimate and its tolerance."""

    def __init__(self, sdf, res, w2g, rot, points):
        self.sdf = np.ascontiguousarray(sdf, np.float32)
        self.res = float(res)
        self.w = np.asarray(w2g, np.float64).reshape(-1)[:12].reshape(3, 4).copy()
        self.r = np.asarray(rot, np.float64).reshape(3, 3).copy()
        self.points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        self._gradients = {}
        shape = self.sdf.shape
        W = [[Fraction(float(v)) for v in row] for row in self.w]
        fres = Fraction(self.res)
        half = fres / 2
        self.per_point = []
        for p in self.points:
            e = _Point()
            self.per_point.append(e)
            e.finite = bool(np.isfinite(p).all())
            if not e.finite:
                continue
            pf = [float(v) for v in p]
            P = [Fraction(v) for v in pf]
            G = [W[i][0] * P[0] + W[i][1] * P[1] + W[i][2] * P[2] + W[i][3] for i in range(3)]
            S = [abs(self.w[i, 0] * pf[0]) + abs(self.w[i, 1] * pf[1]) + abs(self.w[i, 2] * pf[2]) + abs(self.w[i, 3]) for i in range(3)]
            e.S = max(S)
            e.axes, e.ambiguous = [], False
            for i in range(3):
                Q = G[i] / fres
                delta = 8 * U * Fraction(float(S[i])) / fres
                cells = sorted({math.floor(Q - delta), math.floor(Q + delta)})
                e.ambiguous |= len(cells) > 1
                e.axes.append(cells)
            # the estimate, from a candidate cell inside the grid (the exact cell wherever it is one)
            home = []
            for i in range(3):
                exact_cell = math.floor(G[i] / fres)
                inside = [c for c in e.axes[i] if 0 <= c < shape[i]]
                home.append(exact_cell if 0 <= exact_cell < shape[i] else (inside[0] if inside else None))
            e.estimate = e.tolerance = None
            if None in home:
                continue
            pairs = [_axis_pair(home[i], shape[i], G[i] - fres * (Fraction(home[i]) + Fraction(1, 2))) for i in range(3)]
            t = [(G[i] - fres * (Fraction(pairs[i][0]) + Fraction(1, 2))) / fres for i in range(3)]
            total, mag, finite = Fraction(0), Fraction(0), True
            for corner in itertools.product((0, 1), repeat=3):
                v = float(self.sdf[pairs[0][corner[0]], pairs[1][corner[1]], pairs[2][corner[2]]])
                if not math.isfinite(v):
                    finite = False
                    break
                D = Fraction(v) - half if v >= 0.0 else Fraction(v) + half
                wgt = Fraction(1)
                for i in range(3):
                    wgt *= t[i] if corner[i] else 1 - t[i]
                total += D * wgt
                mag += abs(D)
            if finite:
                e.estimate = total
                e.tolerance = 64 * U * (1 + Fraction(float(e.S)) / fres) * mag

    def gradient(self, edge):
        if edge not in self._gradients:
            self._gradients[edge] = A.grid_gradient(self.sdf, self.res, edge)
        return self._gradients[edge]

    def ambiguous(self):
        return np.array([e.finite and e.ambiguous for e in self.per_point])


class Judgement:
    """Expectations for one value of `edge`; check() compares a result with them."""

    def __init__(self, exact, edge):
        self.exact, self.edge = exact, bool(edge)

    def _candidates(self, e):
        """[(flags, grid gradient or None)] of the candidate cells"""
        shape = self.exact.sdf.shape
        gg = self.exact.gradient(self.edge)
        out = []
        for cell in itertools.product(*e.axes):
            if not all(0 <= c < n for c, n in zip(cell, shape)):
                out.append((0, None))
                continue
            have = self.edge or all(0 < c < n - 1 for c, n in zip(cell, shape))
            out.append((1 | (2 if have else 0), gg[cell]))
        return out

    def _gradient_error(self, got, g):
        """None when `got` cannot be the rotation of g, else the worst |error| / tolerance over the components"""
        r = self.exact.r
        if not np.isfinite(g).all():                         # nothing to round: the double evaluation is the expectation
            with np.errstate(invalid="ignore"):
                want = np.array([r[i, 0] * g[0] + r[i, 1] * g[1] + r[i, 2] * g[2] for i in range(3)])
            same = np.isnan(got) == np.isnan(want)
            return 0.0 if same.all() and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]) else None
        if not np.isfinite(got).all():
            return None
        worst = 0.0
        G = [Fraction(float(v)) for v in g]
        for i in range(3):
            R = [Fraction(float(v)) for v in r[i]]
            want = R[0] * G[0] + R[1] * G[1] + R[2] * G[2]
            tol = 4 * U * (abs(R[0] * G[0]) + abs(R[1] * G[1]) + abs(R[2] * G[2]))
            err = abs(Fraction(float(got[i])) - want)
            if err > tol:
                return None
            if err:
                worst = max(worst, float(err / tol))
        return worst

    def evaluate(self, dist, grad, flags, oob=np.inf):
        """(the points that no candidate explains, as a list of descriptions; the figures check() returns)"""
        pts = self.exact.points
        dist, grad, flags = np.asarray(dist, np.float64), np.asarray(grad, np.float64).reshape(-1, 3), np.asarray(flags)
        assert len(dist) == len(grad) == len(flags) == len(pts), "result length"
        oob = float(np.float32(oob))
        bad, inside, worst_d, worst_g, unjudged = [], 0, 0.0, 0.0, 0
        for k, e in enumerate(self.exact.per_point):
            f, d, g = int(flags[k]), float(dist[k]), grad[k]
            outside_ok = f == 0 and (d == oob or (math.isnan(d) and math.isnan(oob))) and bool(np.isnan(g).all())
            if not e.finite:
                if not outside_ok:
                    bad.append((k, "non-finite point", f, d, tuple(g)))
                continue
            verdict = None
            for cf, cg in self._candidates(e):
                if cf != f:
                    continue
                if cf == 0:
                    verdict = (0.0, 0.0) if outside_ok else None
                else:
                    ge = self._gradient_error(g, cg)
                    if ge is None:
                        continue
                    if e.estimate is None:
                        verdict = (None, ge)
                    elif math.isfinite(d):
                        err = abs(Fraction(d) - e.estimate)
                        if err <= e.tolerance:
                            verdict = (float(err / e.tolerance) if err else 0.0, ge)
                if verdict is not None:
                    break
            if verdict is None:
                bad.append((k, "ambiguous" if e.ambiguous else "one cell", f, d, tuple(g), "exact estimate",
                            None if e.estimate is None else float(e.estimate), "tolerance",
                            None if e.tolerance is None else float(e.tolerance), "candidates", self._candidates(e)))
                continue
            if f:
                inside += 1
                if verdict[0] is None:
                    unjudged += 1
                else:
                    worst_d = max(worst_d, verdict[0])
                worst_g = max(worst_g, verdict[1])
        return bad, {"inside": inside, "ambiguous": int(self.exact.ambiguous().sum()), "unjudged": unjudged,
                     "distance": worst_d, "gradient": worst_g}

    def check(self, dist, grad, flags, oob=np.inf):
        """Raises AssertionError naming the first points that no candidate explains.  Returns a dict: inside (points answered
        from a cell), ambiguous, unjudged (distances with a non-finite corner), and the worst |error| / tolerance of the
        distances and of the gradients."""
        bad, figures = self.evaluate(dist, grad, flags, oob)
        assert not bad, "%d of %d points outside the judge's bounds, the first: %r" % (len(bad), len(self.exact.points), bad[:3])
        return figures

    def failures(self, dist, grad, flags, oob=np.inf):
        """the number of points check() would reject"""
        return len(self.evaluate(dist, grad, flags, oob)[0])


def judge(sdf, res, w2g, rot, points, edge, exact=None):
    """The expectations of sdfgpu_query_points(sdf, res, w2g, rot, points, edge) as a Judgement.  `exact` (an Exact of the same
    field, transforms and points) is reused when given: it does not depend on `edge` or on oob_value."""
    return Judgement(exact if exact is not None else Exact(sdf, res, w2g, rot, points), edge)
