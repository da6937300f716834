"""tests/frame_judge.py pinned before it judges the GPU: the controls (where the judge must accept analysis_scenes.query_points' own
output), hand cases on a slab whose estimate is linear, a double emulation of k_query_points that passes in every frame, mutants
of that emulation that fail, the blind spot of rigid() written down, and the cap on ambiguous points of every GPU case."""
import math
from fractions import Fraction

import numpy as np
import pytest

import analysis_scenes as A
import frame_judge as J
from oracle import oracle as O
from test_projection_cpu import inverse, rigid, slab

FRAMES = sorted(J.frames())
_CASES = {}


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def _field(shape, res):
    key = (tuple(shape), res)
    if key not in _CASES:
        _CASES[key] = O.reference_sdf(J.case_mask(shape), res)[0]
        assert np.isfinite(_CASES[key]).all()
    return _CASES[key]


def _case(frame, shape, res):
    """(field, w2g, rot, points, slices, Exact), computed once per (frame, shape) and left unchanged"""
    key = (frame, tuple(shape))
    if key not in _CASES:
        sdf = _field(shape, res)
        origin = J.frames()[frame]
        w2g, rot = J.transforms(origin)
        pts, parts = J.case_points(shape, res, origin, J.case_seed(frame, shape))
        _CASES[key] = (sdf, w2g, rot, pts, parts, J.Exact(sdf, res, w2g, rot, pts))
    return _CASES[key]


# ---- controls ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("shape, res", [f for f in J.FIELDS if f[0] != (40, 33, 48)])
@pytest.mark.parametrize("frame", ["identity", "translation"])
def test_controls_accept_the_restatement(frame, shape, res, edge):
    """w2g = (I, -t): 1 x + 0 y + 0 z - t is x - t, one rounding, so the kernel is analysis_scenes.query_points at pts - t"""
    sdf, w2g, rot, pts, parts, exact = _case(frame, shape, res)
    with np.errstate(invalid="ignore"):
        g = pts - J.frames()[frame][:3, 3]
    dist, grad, flags = A.query_points(sdf, res, g, 7.5, edge)
    got = J.judge(sdf, res, w2g, rot, pts, edge, exact).check(dist, grad, flags, 7.5)
    assert 0 < got["inside"] < len(pts) and got["unjudged"] == 0
    assert got["gradient"] == 0.0                                 # (the rotation by exact 0 / 1 entries is exact)


# ---- hand cases -------------------------------------------------------------------------------------------------------------------
def test_hand_cases_on_the_slab():
    """slab(): cells 10 .. 30 of 41 filled along x; near x = 10 the estimate is (10 - x) res, beyond x = 31 it is (x - 31) res, in
    grid cells.  res = 1/8, so every value is exact in float32 and in the judge."""
    res = 0.125
    sdf = slab(res)
    w2g, rot = J.transforms(np.eye(4))
    y, z = 2.3 * res, 2.2 * res
    pts = np.array([[12.5 * res, 2.5 * res, 2.5 * res],           # a cell centre: D = f - res / 2 toward the surface
                    [0.0, y, z],                                   # half a cell before the first centre: 1 * 0 + 0 y + 0 z + 0 is exact
                    [41.0 * res, y, z],                            # half a cell beyond the last centre: the exact cell is outside
                    [11.0 * res, y, z]])                           # on the face between cells 10 and 11
    exact = J.Exact(sdf, res, w2g, rot, pts)
    e = exact.per_point
    assert [p.ambiguous for p in e] == [False, False, True, True]     # (S_x = 0 at x = 0: nothing was rounded)
    assert e[0].estimate == Fraction(-2.5 * res) and e[0].axes == [[12], [2], [2]]
    assert e[1].estimate == Fraction(10 * res) and e[1].axes[0] == [0]         # 9.5 res at the centre, extrapolated
    assert e[2].estimate == Fraction(10 * res) and e[2].axes[0] == [40, 41]
    assert e[3].estimate == Fraction(-1.0 * res) and e[3].axes[0] == [10, 11]
    nan3 = [math.nan] * 3
    judged = J.judge(sdf, res, w2g, rot, pts, False, exact)

    def accepted(k, d, g, f):
        dist, grad, flags = np.array([-2.5 * res, 10 * res, math.inf, -res]), np.array([[-1.0, 0, 0], nan3, nan3, [-1.0, 0, 0]]), \
            np.array([3, 1, 0, 3], np.uint8)                       # (answers the judge accepts, but for point k)
        dist[k], grad[k], flags[k] = d, g, f
        bad, _ = judged.evaluate(dist, grad, flags)
        assert [b[0] for b in bad] in ([], [k])
        return not bad

    assert accepted(0, -2.5 * res, [-1.0, 0, 0], 3)
    assert not accepted(0, -2.5 * res + 1e-12, [-1.0, 0, 0], 3)   # (the tolerance there is 64 u (1 + 12.5) 8 * 2.5 res ~ 4e-13)
    assert not accepted(0, -2.5 * res, [-1.0, 0, 0], 1) and not accepted(0, -2.5 * res, [0, -1.0, 0], 3)
    for k in (1, 2):                                               # the outer faces: the extrapolated estimate
        assert accepted(k, 10 * res, nan3, 1)                      # cells 0 and 40 are boundary cells: no gradient without `edge`
        assert accepted(k, math.inf, nan3, 0) == (k == 2)          # ... or outside, where rounding may have put the point there
        assert not accepted(k, 9.5 * res, nan3, 1) and not accepted(k, 10 * res, nan3, 0) and not accepted(k, math.inf, nan3, 1)
    assert accepted(3, -res, [-1.5, 0, 0], 3)                      # cell 10: (f(11) - f(9)) / 2 res
    assert accepted(3, -res, [-1.0, 0, 0], 3)                      # cell 11: (f(12) - f(10)) / 2 res
    assert not accepted(3, -res, [-1.25, 0, 0], 3) and not accepted(3, -res, nan3, 0) and not accepted(3, -1.5 * res, [-1.0, 0, 0], 3)
    edge = J.judge(sdf, res, w2g, rot, pts[1:3], True)            # with edge gradients: one-sided differences, -1 and +1
    assert edge.failures([10 * res, 10 * res], [[-1.0, 0, 0], [1.0, 0, 0]], [3, 3]) == 0
    assert edge.failures([10 * res, 10 * res], [[1.0, 0, 0], [-1.0, 0, 0]], [3, 3]) == 2


# ---- the emulation passes, its mutants fail -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, res", J.FIELDS)
@pytest.mark.parametrize("frame", FRAMES)
def test_emulation_passes_and_few_points_are_ambiguous(frame, shape, res):
    """The ambiguity cap is a condition on the points of every GPU case (tests/test_gpu_query_frames.py draws the same ones): at
    most 0.5 % of the uniform points may be ambiguous, so that no case can pass on points the judge lets choose; the lattice
    points are ambiguous by construction, so the accept-either arm runs."""
    sdf, w2g, rot, pts, parts, exact = _case(frame, shape, res)
    amb = exact.ambiguous()
    assert amb[parts["uniform"]].mean() <= J.AMBIGUITY_CAP
    assert amb[parts["uniform"]].sum() == 0                       # (what to expect: delta is some 1e-14 of a cell)
    assert amb[parts["lattice"]].sum() >= 32
    for edge in (False, True):
        dist, grad, flags = J.emulate(sdf, res, w2g, rot, pts, 7.5, edge)
        got = J.judge(sdf, res, w2g, rot, pts, edge, exact).check(dist, grad, flags, 7.5)
        assert 0 < got["inside"] < len(pts) and got["unjudged"] == 0
        print("emulation %s %s edge %d: worst |error| / tolerance: distance %.4f gradient %.4f" % (
            frame, shape, edge, got["distance"], got["gradient"]))


def _transposed_block(w):
    m = w.copy()
    m[:, :3] = w[:, :3].T
    return m


def _exchanged(m, a, b):
    out = m.copy().reshape(-1)
    out[a], out[b] = out[b], out[a]
    return out.reshape(m.shape)


def _dropped(w):
    m = w.copy()
    m[0, 3] = 0.0
    return m


MUTANTS = {
    "w2g block transposed": lambda w, r: (_transposed_block(w), r),
    "rot transposed": lambda w, r: (w, r.T.copy()),
    "w2g[2] <-> w2g[8]": lambda w, r: (_exchanged(w, 2, 8), r),
    "rot[2] <-> rot[6]": lambda w, r: (w, _exchanged(r, 2, 6)),
    "w2g[3] dropped": lambda w, r: (_dropped(w), r),
}
# where a mutation leaves the matrices as they are: a symmetric block; zero entries exchanged (about-x keeps x: [0][2] = [2][0] = 0);
# no translation to drop
NO_OPS = {("identity", k) for k in MUTANTS} | {("translation", k) for k in MUTANTS if k != "w2g[3] dropped"} | \
    {("about-x", "w2g[2] <-> w2g[8]"), ("about-x", "rot[2] <-> rot[6]")}


@pytest.mark.parametrize("frame", FRAMES)
def test_mutants_fail(frame):
    shape, res = J.FIELDS[0]
    sdf, w2g, rot, pts, parts, exact = _case(frame, shape, res)
    judged = J.judge(sdf, res, w2g, rot, pts, True, exact)        # edge gradients: every inside point has a gradient to rotate
    inside = np.flatnonzero(J.emulate(sdf, res, w2g, rot, pts, np.inf, True)[2] & 1)
    assert len(inside) > 500
    for name, mutate in MUTANTS.items():
        w, r = mutate(w2g, rot)
        if (frame, name) in NO_OPS:
            assert np.array_equal(w, w2g) and np.array_equal(r, rot), (frame, name)
            continue
        assert not (np.array_equal(w, w2g) and np.array_equal(r, rot)), (frame, name)
        bad, _ = judged.evaluate(*J.emulate(sdf, res, w, r, pts, np.inf, True))
        failed = np.intersect1d([b[0] for b in bad], inside)
        assert len(failed) >= 0.1 * len(inside), (frame, name, len(failed), len(inside))


def test_the_blind_spot_of_a_turn_about_z():
    """The hole this module closes: under rigid(0.6, t) the exchanged entries are all zero, so a layer that reads w2g[8] for w2g[2]
    or rot[6] for rot[2] computes the same bits and passes; the same mutants fail in `general` (test_mutants_fail)."""
    shape, res = J.FIELDS[0]
    sdf = _field(shape, res)
    origin = rigid(0.6, (-0.4, 1.25, 0.3))
    w2g, rot = J.transforms(origin)
    assert np.array_equal(w2g, inverse(origin)[:3])
    pts, _ = J.case_points(shape, res, origin, 5)
    want = J.emulate(sdf, res, w2g, rot, pts, np.inf, True)
    judged = J.judge(sdf, res, w2g, rot, pts, True)
    assert judged.check(*want)["inside"] > 500
    for name in ("w2g[2] <-> w2g[8]", "rot[2] <-> rot[6]"):
        w, r = MUTANTS[name](w2g, rot)
        got = J.emulate(sdf, res, w, r, pts, np.inf, True)
        assert all(_same(a, b) for a, b in zip(got, want)), name
        assert judged.failures(*got) == 0
    for name in ("w2g block transposed", "rot transposed", "w2g[3] dropped"):    # (what z turns do catch)
        w, r = MUTANTS[name](w2g, rot)
        assert judged.failures(*J.emulate(sdf, res, w, r, pts, np.inf, True)) > 100, name
