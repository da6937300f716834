"""Smooth and autodiff gradients and DistanceToBoundary without a GPU: SignedDistanceField's host members (include/sdf_tools/sdf.hpp,
reference include/sdf_tools/sdf.hpp:528-653, 963-988) pinned to hand-derived answers, to an independent Python restatement of the
dual-number arithmetic, and to finite differences.  The host core is the yardstick of the GPU kernel
(tests/test_gpu_query_gradients.py compares the two bit for bit)."""
import math

import numpy as np
import pytest

from sdf_tools_amd import capi
from sdf_tools_amd._bindings import load_pysdf_tools
from test_projection_cpu import inverse, rigid, slab

m = load_pysdf_tools()
SMOOTH, AUTODIFF, BOUNDARY = capi.QUERY_SMOOTH_GRADIENT, capi.QUERY_AUTODIFF_GRADIENT, capi.QUERY_DISTANCE_TO_BOUNDARY
OK, OUTSIDE, TOO_LARGE, NON_FINITE = capi.QUERY_OK, capi.QUERY_OUTSIDE, capi.QUERY_WINDOW_TOO_LARGE, capi.QUERY_NON_FINITE
TOO_LARGE_MSG = "Window size for GetSmoothGradient is too large for SDF"


def field(data, res, origin=None, oob=math.inf):
    data = np.ascontiguousarray(data, np.float32)
    s = m.SignedDistanceField(m.Isometry3d(np.eye(4) if origin is None else origin), "world", float(res), *data.shape, oob)
    s.SetRawDataNumpy(data)
    return s


def world(origin, g):
    """grid-frame point -> world frame, eigen_lite's order"""
    o = np.eye(4) if origin is None else origin
    return tuple(float(o[i, 0]) * g[0] + float(o[i, 1]) * g[1] + float(o[i, 2]) * g[2] + float(o[i, 3]) for i in range(3))


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


# ---- an independent restatement of the autodiff estimate: Eigen::AutoDiffScalar's rules on (value, d0, d1, d2) tuples ------------
# Python floats are IEEE doubles and never fuse a product with a sum.
def ad(v, d=(0.0, 0.0, 0.0)):
    return (float(v), float(d[0]), float(d[1]), float(d[2]))


def mul(a, b):                     # AD * AD: value a b, derivatives (a.d b) + (b.d a)
    return (a[0] * b[0], a[1] * b[0] + b[1] * a[0], a[2] * b[0] + b[2] * a[0], a[3] * b[0] + b[3] * a[0])


def smul(s, b):                    # double * AD: b.d s
    return (s * b[0], b[1] * s, b[2] * s, b[3] * s)


def add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def rsub(s, b):                    # double - AD: -b.d
    return (s - b[0], -b[1], -b[2], -b[3])


def dsub(a, s):                    # AD - double: a.d
    return (a[0] - s, a[1], a[2], a[3])


def axis_pair(i, n, off):
    lo = hi = i
    if off >= 0.0:
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


def restated(data, res, origin, p):
    """GetAutoDiffGradient(x, y, z) and its value, from the reference text; None outside the grid"""
    w = inverse(np.eye(4) if origin is None else origin)
    seeds = [ad(p[k], [1.0 if j == k else 0.0 for j in range(3)]) for k in range(3)]
    one = ad(1.0)
    q = []
    for i in range(3):           # inverse_origin_transform_ * Alocation, ((m0 p0 + m1 p1) + m2 p2) + m3 p3
        q.append(add(add(add(smul(float(w[i, 0]), seeds[0]), smul(float(w[i, 1]), seeds[1])), smul(float(w[i, 2]), seeds[2])),
                     smul(float(w[i, 3]), one)))
    inv = 1.0 / res
    cell = [math.floor(q[k][0] * inv) for k in range(3)]
    if not all(0 <= cell[k] < data.shape[k] for k in range(3)):
        return None
    idx = [axis_pair(cell[k], data.shape[k], q[k][0] - res * (cell[k] + 0.5)) for k in range(3)]
    lo = [res * (idx[k][0] + 0.5) for k in range(3)]
    half = res * 0.5

    def D(a, b, c):
        v = float(data[a, b, c])
        return v - half if v >= 0.0 else v + half

    def bilinear(l1, h1, l2, h2, q1, q2, ll, lh, hl, hh):
        mult = ad(1.0 / ((h1 - l1) * (h2 - l2)))
        a0, a1 = mul(mult, rsub(h1, q1)), mul(mult, dsub(q1, l1))
        r0 = add(mul(a0, ad(ll)), mul(a1, ad(hl)))
        r1 = add(mul(a0, ad(lh)), mul(a1, ad(hh)))
        return add(mul(r0, rsub(h2, q2)), mul(r1, dsub(q2, l2)))

    (x0, x1), (y0, y1), (z0, z1) = idx
    mz = bilinear(lo[0], lo[0] + res, lo[1], lo[1] + res, q[0], q[1], D(x0, y0, z0), D(x0, y1, z0), D(x1, y0, z0), D(x1, y1, z0))
    pz = bilinear(lo[0], lo[0] + res, lo[1], lo[1] + res, q[0], q[1], D(x0, y0, z1), D(x0, y1, z1), D(x1, y0, z1), D(x1, y1, z1))
    slope = smul(1.0 / res, sub(pz, mz))
    r = add(mz, mul(sub(q[2], ad(lo[2])), slope))
    return r[0], r[1:]


def host(s, pts, kind, window=0.0):
    return s.QueryGradientsNumpyHost(np.asarray(pts, np.float64).reshape(-1, 3), kind, window)


# ---- known answers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", ["identity", "rotated"])
def test_slab_known_answers(frame):
    """near x = 10 (grid frame, cells) the estimate of the slab is exactly (10 - x) res: the autodiff gradient is the grid x axis
    negated, rotated into the world; the smooth gradient with window res / 8 agrees to 1e-12 (res = 1/8: the float32 cells hold
    the slab's multiples of res exactly)"""
    res = 0.125
    origin = None if frame == "identity" else rigid(0.7, (0.3, -1.2, 0.5))
    s = field(slab(res), res, origin)
    want = np.array([-1.0, 0.0, 0.0]) if origin is None else -origin[:3, 0]
    for gx in (9.3, 9.71, 10.2, 10.45):
        p = world(origin, (gx * res, 2.3 * res, 2.2 * res))
        g = np.array(s.GetAutoDiffGradient(*p))
        assert np.allclose(g, want, atol=1e-12, rtol=0), (gx, g)
        sm = np.array(s.GetSmoothGradient(*p, res / 8))
        assert np.allclose(sm, g, atol=1e-12, rtol=0), (gx, sm)
        v, grad, st = host(s, [p], AUTODIFF)
        assert st[0] == OK and abs(v[0] - (10 - gx) * res) < 1e-12


def test_autodiff_matches_restatement_bit_for_bit():
    rng = np.random.default_rng(5)
    import frame_judge                                           # (imports this directory's modules: not at module level)
    fr = frame_judge.frames()                                    # frames with z couplings, which rigid() leaves at zero
    cases = [((7, 9, 6), 0.05, None), ((11, 5, 8), 0.02, rigid(0.4, (0.2, -0.1, 0.3))), ((20, 40, 1), 0.1, None),
             ((20, 40, 1), 0.1, rigid(-1.1, (1.0, 2.0, -0.5))), ((1, 1, 9), 0.3, rigid(2.0, (0.0, 0.5, 0.25))),
             ((7, 9, 6), 0.05, fr["general"]), ((11, 5, 8), 0.02, fr["about-x"]), ((9, 4, 7), 0.05, fr["cyclic"]),
             ((20, 40, 1), 0.1, fr["general"])]
    checked = 0
    for shape, res, origin in cases:
        data = rng.uniform(-3 * res, 5 * res, shape).astype(np.float32)
        s = field(data, res, origin)
        size = np.array(shape) * res
        g = list(rng.uniform(-0.05, 1.05, (300, 3)) * size)
        g += [np.array([(i + 0.5) * res for i in c]) for c in [(0, 0, 0), tuple(n - 1 for n in shape), tuple(n // 2 for n in shape)]]
        g += [np.array([a, b, c]) for a in (0.0, size[0] - 1e-9) for b in (0.0, size[1] - 1e-9) for c in (0.0, size[2] - 1e-9)]
        g += [np.array([res * k, size[1] * 0.5, size[2] * 0.3]) for k in range(shape[0] + 1)]            # cell faces
        pts = np.array([world(origin, tuple(float(v) for v in x)) for x in g])
        v, grad, st = host(s, pts, AUTODIFF)
        for i, p in enumerate(pts):
            r = restated(data, res, origin, p)
            if r is None:
                assert st[i] == OUTSIDE and v[i] == math.inf and np.isnan(grad[i]).all()
                assert s.GetAutoDiffGradient(*p) == []
                continue
            assert st[i] == OK
            assert bits(v[i]) == bits(r[0]), (shape, p)
            assert np.array_equal(bits(grad[i]), bits(r[1])), (shape, p, grad[i], r[1])
            assert np.array_equal(bits(s.GetAutoDiffGradient(*p)), bits(r[1]))
            checked += 1
    assert checked > 2000


def test_autodiff_value_is_estimate_distance():
    rng = np.random.default_rng(8)
    res = 0.04
    data = rng.uniform(-0.2, 0.3, (9, 10, 11)).astype(np.float32)
    origin = rigid(0.25, (-0.3, 0.1, 0.2))
    s = field(data, res, origin)
    pts = [world(origin, tuple(rng.uniform(-0.02, 1.02, 3) * np.array(data.shape) * res)) for _ in range(500)]
    v, _, st = host(s, pts, AUTODIFF)
    vs, _, sts = host(s, pts, SMOOTH, res)
    for i, p in enumerate(pts):
        d, inside = s.EstimateDistance(*p)
        assert bits(v[i]) == bits(d) and (st[i] == OK) == inside
        if inside:
            assert bits(vs[i]) == bits(d)


def test_autodiff_agrees_with_finite_differences():
    rng = np.random.default_rng(13)
    res = 0.05
    data = rng.uniform(-0.2, 0.3, (8, 9, 7)).astype(np.float32)
    origin = rigid(0.5, (0.4, -0.2, 0.1))
    s = field(data, res, origin)
    h = 1e-6 * res
    checked = 0
    for _ in range(400):
        g = rng.uniform(0.02, 0.98, 3) * np.array(data.shape) * res
        off = g / res - 0.5
        # keep away from the cell-centre planes (where the corners switch) and from the cell faces (where the cell does)
        if np.any(np.abs(off - np.round(off)) < 1e-3) or np.any(np.abs(g / res - np.round(g / res)) < 1e-3):
            continue
        p = np.array(world(origin, tuple(g)))
        ga = np.array(s.GetAutoDiffGradient(*p))
        fd = np.array([(s.EstimateDistance(*(p + h * e))[0] - s.EstimateDistance(*(p - h * e))[0]) / (2 * h) for e in np.eye(3)])
        assert np.allclose(ga, fd, rtol=1e-6, atol=1e-6 * max(1.0, np.abs(ga).max())), (g, ga, fd)
        checked += 1
    assert checked > 200


# ---- smooth gradient edge cases ------------------------------------------------------------------------------------------------
def test_smooth_edges_and_refusals():
    res = 0.1
    data = slab(res)
    s = field(data, res)
    nx, ny, nz = data.shape
    c = (20.3 * res, 2.5 * res, 2.5 * res)
    w = res / 8
    # one-sided at the low x face: the minus end leaves the grid
    p = (0.01 * res, 2.5 * res, 2.5 * res)
    d0 = s.EstimateDistance(*p)[0]
    dp = s.EstimateDistance(p[0] + w, p[1], p[2])[0]
    g = s.GetSmoothGradient(*p, w)
    assert bits(g[0]) == bits((dp - d0) / ((p[0] + w) - p[0]))
    # ... and at the high face the plus end does
    p = ((nx - 0.01) * res, 2.5 * res, 2.5 * res)
    d0 = s.EstimateDistance(*p)[0]
    dm = s.EstimateDistance(p[0] - w, p[1], p[2])[0]
    assert bits(s.GetSmoothGradient(*p, w)[0]) == bits((d0 - dm) / (p[0] - (p[0] - w)))
    # a window past both ends of an axis (z has 5 cells)
    with pytest.raises(RuntimeError, match=TOO_LARGE_MSG):
        s.GetSmoothGradient(*c, 3.0 * res)
    v, grad, st = host(s, [c], SMOOTH, 3.0 * res)
    assert st[0] == TOO_LARGE and np.isnan(grad).all() and bits(v[0]) == bits(s.EstimateDistance(*c)[0])
    # outside: an empty list; a negative window is its absolute value; zero gives 0 / 0
    assert s.GetSmoothGradient(-0.01, 0.2, 0.2, w) == []
    assert np.array_equal(bits(s.GetSmoothGradient(*c, -w)), bits(s.GetSmoothGradient(*c, w)))
    assert np.isnan(s.GetSmoothGradient(*c, 0.0)).all()
    v, grad, st = host(s, [c], SMOOTH, 0.0)
    assert st[0] == OK and np.isnan(grad).all()
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError):
            s.GetSmoothGradient(*c, bad)
        with pytest.raises(ValueError):
            host(s, [c], SMOOTH, bad)
        with pytest.raises(ValueError):
            s.GetSmoothGradient(bad, 0.2, 0.2, w)
        with pytest.raises(ValueError):
            s.GetAutoDiffGradient(0.2, bad, 0.2)
    v, grad, st = host(s, [(math.nan, 0.2, 0.2), (0.2, 0.2, math.inf)], AUTODIFF)
    assert (st == NON_FINITE).all() and np.isnan(v).all() and np.isnan(grad).all()
    with pytest.raises(ValueError):
        host(s, [c], 7)


def test_smooth_restated_on_random_field():
    _smooth_restated(rigid(-0.6, (0.1, 0.2, -0.3)))


@pytest.mark.parametrize("frame", ["general", "about-x", "cyclic"])
def test_smooth_restated_in_frames_with_z_couplings(frame):
    import frame_judge
    _smooth_restated(frame_judge.frames()[frame])


def _smooth_restated(origin):
    rng = np.random.default_rng(21)
    res = 0.05
    data = rng.uniform(-0.2, 0.3, (9, 8, 10)).astype(np.float32)
    s = field(data, res, origin)
    for w in (res / 8, res, 3 * res):
        pts = [world(origin, tuple(rng.uniform(-0.05, 1.05, 3) * np.array(data.shape) * res)) for _ in range(200)]
        v, grad, st = host(s, pts, SMOOTH, w)
        for i, p in enumerate(pts):
            d = s.EstimateDistance(*p)
            if not d[1]:
                assert st[i] == OUTSIDE and s.GetSmoothGradient(*p, w) == []
                continue
            want = []
            for k in range(3):
                lo, hi = list(p), list(p)
                lo[k] -= w
                hi[k] += w
                dm, dp = s.EstimateDistance(*lo), s.EstimateDistance(*hi)
                if dm[1] and dp[1]:
                    want.append((dp[0] - dm[0]) / (hi[k] - lo[k]))
                elif dm[1]:
                    want.append((d[0] - dm[0]) / (p[k] - lo[k]))
                elif dp[1]:
                    want.append((dp[0] - d[0]) / (hi[k] - p[k]))
                else:
                    want = None
                    break
            if want is None:
                assert st[i] == TOO_LARGE
                with pytest.raises(RuntimeError, match=TOO_LARGE_MSG):
                    s.GetSmoothGradient(*p, w)
            else:
                assert st[i] == OK and np.array_equal(bits(grad[i]), bits(want))
                assert np.array_equal(bits(s.GetSmoothGradient(*p, w)), bits(want))


# ---- DistanceToBoundary ----------------------------------------------------------------------------------------------------------
def test_distance_to_boundary_hand_cases():
    res = 0.5
    s = field(np.zeros((4, 6, 8), np.float32), res)          # size 2 x 3 x 4
    assert s.DistanceToBoundary(1.0, 1.5, 2.0) == (1.0, True)                 # centre: x is nearest (1.0 < 1.5 < 2.0)
    assert s.DistanceToBoundary(0.25, 1.5, 2.0) == (0.25, True)
    assert s.DistanceToBoundary(1.0, 2.9, 2.0) == pytest.approx((0.1, True))
    assert s.DistanceToBoundary(1.0, 1.5, 3.75) == (0.25, True)
    assert s.DistanceToBoundary(-0.5, 1.5, 2.0) == (-0.5, False)              # beyond the low x face
    assert s.DistanceToBoundary(2.25, 1.5, 2.0) == (-0.25, False)
    assert s.DistanceToBoundary(1.0, 1.5, 4.5) == (-0.5, False)
    assert s.DistanceToBoundary(1.0, -0.125, 2.0) == (-0.125, False)
    assert s.DistanceToBoundary(0.5, 0.5, 2.0) == (0.5, True)                 # a tie: the first axis wins
    assert s.DistanceToBoundary(1.5, 0.5, 2.0) == (0.5, True)
    assert s.DistanceToBoundary(0.0, 1.5, 2.0) == (0.0, True)                 # on a face
    assert s.DistanceToBoundary(-0.25, 0.25, 2.0) == (-0.25, False)           # |-0.25| == |0.25|: the first
    v, g, st = host(s, [(1.0, 1.5, 2.0), (-0.5, 1.5, 2.0)], BOUNDARY)
    assert list(v) == [1.0, -0.5] and list(st) == [OK, OUTSIDE] and np.isnan(g).all()
    origin = rigid(0.9, (1.0, -2.0, 0.5))
    r = field(np.zeros((4, 6, 8), np.float32), res, origin)
    for gp, want in (((1.0, 1.5, 2.0), (1.0, True)), ((0.5, 0.3, 2.0), (0.3, True)), ((1.0, 3.2, 2.0), (-0.2, False))):
        got = r.DistanceToBoundary(*world(origin, gp))
        assert got[1] == want[1] and abs(got[0] - want[0]) < 1e-12
        q = np.array(world(inverse(origin), world(origin, gp)))
        d = [min(q[k], sz - q[k]) for k, sz in enumerate((2.0, 3.0, 4.0))]
        assert bits(got[0]) == bits(d[int(np.argmin(np.abs(d)))])


# ---- fields with infinite values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [math.inf, -math.inf])
def test_infinite_fields(fill):
    """an all-empty (+inf) or all-filled (-inf) field: the estimate is NaN (inf - inf in the bilinear sums), and the autodiff
    derivatives are NaN through the kept zero terms (0 * inf)"""
    res = 0.1
    data = np.full((6, 5, 4), fill, np.float32)
    s = field(data, res)
    p = (0.23, 0.31, 0.17)
    v, grad, st = host(s, [p], AUTODIFF)
    r = restated(data, res, None, p)
    assert st[0] == OK and bits(v[0]) == bits(r[0]) and np.array_equal(bits(grad[0]), bits(r[1]))
    assert math.isnan(v[0]) and np.isnan(grad[0]).all()
    v, grad, st = host(s, [p], SMOOTH, res)
    assert st[0] == OK and math.isnan(v[0]) and np.isnan(grad[0]).all()
