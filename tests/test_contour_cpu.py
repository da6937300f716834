"""The contour rule without a GPU (tests/contour_restated.py): the reference's recipe -- one exact distance
field per object, finished as this project finishes it, and the literal float comparisons -- equals the 26-neighbour rule at
reach(resolution); the reach table; the monotonicity that the derivation rests on; the C helper; and the closed form of the
large GPU cases on a small replica."""
import numpy as np
import pytest
import torch

import contour_restated as CR
import display_cases as C
import resolution_domain as RD
from sdf_tools_amd import capi

OCC_VALUES = C.OCC_VALUES
TABLE_RES = [r for r, _ in CR.REACH_TABLE]
CLASS_RES = list(RD.CLASS_A) + list(RD.CLASS_B) + [RD.SUBNORMAL, RD.STRADDLE, RD.STRADDLE_DENSE, RD.STRADDLE_NOISE, RD.UNDERFLOW, 2.0 ** 125, 2.0 ** 126,
                                                  2.0 ** 127, 1.5 * 2.0 ** 127, RD.TOTAL_OVERFLOW]


def _random_grid(rng):
    shape = tuple(int(v) for v in rng.integers(1, 10, size=3))
    shape = (min(shape[0], 9), min(shape[1], 8), min(shape[2], 7))
    occ = rng.choice(OCC_VALUES, size=shape, p=rng.dirichlet(np.ones(len(OCC_VALUES))))
    if rng.random() < 0.5:                                      # mostly filled: interiors with D >= 4 exist
        occ = np.where(rng.random(shape) < 0.9, np.float32(1.0), occ).astype(np.float32)
    pool = np.array([[7], [0, 3], [1, 2, 3], [0, 1, 2 ** 32 - 1, 9], [0, 5, 6, 70000, 2 ** 31]][int(rng.integers(5))], np.uint32)
    keys = rng.choice(pool, size=shape)
    if rng.random() < 0.5:                                      # slabs of one id
        keys = np.broadcast_to(pool[(np.arange(shape[0]) * len(pool) // shape[0])][:, None, None], shape).copy()
    return occ, keys, pool


@pytest.mark.parametrize("res", TABLE_RES + CLASS_RES)
def test_literal_equals_neighbour_rule(res):
    rng = np.random.default_rng(int(abs(np.log2(res)) * 1000) % 100003)
    reach = CR.reach(res)
    for case in range(12):
        occ, keys, pool = _random_grid(rng)
        for uif in (True, False):
            draw = None if case % 3 == 0 else np.unique(rng.choice(pool, size=2))
            draw_zero = bool(case % 2)
            want = CR.literal(occ, keys, res, uif, draw, draw_zero)
            got = CR.by_neighbours(occ, keys, reach, uif, draw, draw_zero)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (res, reach, occ.shape, uif, draw, draw_zero)


def test_solid_grid_with_an_interior_beyond_the_reach():
    """a 9 x 8 x 7 box with one free corner cell: cells with D = 4 .. exist and none of them is drawn at any resolution of the table"""
    occ = np.ones((9, 8, 7), np.float32)
    occ[0, 0, 0] = 0.0
    keys = np.full(occ.shape, 4, np.uint32)
    D = -CR.object_dsq(CR.filled_cells(occ))
    assert (D >= 4).sum() > 400
    for res in TABLE_RES:
        idx, _ = CR.literal(occ, keys, res)
        assert np.array_equal(idx, CR.by_neighbours(occ, keys, CR.reach(res))[0])
        assert (D.reshape(-1)[idx] <= 3).all() and len(idx) == int(((D >= 1) & (D <= CR.reach(res))).sum())


def test_reach_table():
    for res, want in CR.REACH_TABLE:
        assert CR.reach(res) == want, (res, CR.reach(res), want)


def _probe_resolutions():
    out = list(np.exp2(np.linspace(-170.0, 130.0, 10000)))
    for res in TABLE_RES + CLASS_RES:
        out += [float(np.nextafter(res, 0.0)), float(res), float(np.nextafter(res, np.inf))]
        with np.errstate(over="ignore", under="ignore"):
            r32 = np.float32(res)
        if np.isfinite(r32) and r32 > 0:
            out += [float(np.nextafter(r32, np.float32(0.0))), float(r32), float(np.nextafter(r32, np.float32(np.inf)))]
    return [r for r in out if r > 0.0 and np.isfinite(r)]


def test_f_is_monotone_and_d4_is_never_drawn():
    res = np.array(_probe_resolutions(), np.float64)
    f = [CR.f(D, res) for D in range(1, 30)]
    for a, b in zip(f[:-1], f[1:]):
        assert (a <= b).all()
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        bdy = (np.float64(-1.9) * res).astype(np.float32)
        assert (CR.f(4, res) >= -bdy).all()                     # float(2 res) >= float(1.9 res): rounding is monotone
    for r in res:
        drawn = [CR.admits(D, r) for D in (1, 2, 3, 4, 5, 9)]
        assert not any(drawn[3:]), r
        assert drawn[:3] == [D <= CR.reach(r) for D in (1, 2, 3)], (r, drawn)      # the drawn set is a prefix: {D <= reach}


def test_c_helper_equals_reach():
    for r in _probe_resolutions():
        assert capi.display_contour_reach(r) == CR.reach(r), r
    for r in (0.0, -0.0, -1.0, float("nan"), float("-inf"), -1e-320):
        assert capi.display_contour_reach(r) == 0, r
    assert capi.display_contour_reach(float("inf")) == 0
    assert capi.load_library().sdfgpu_display_contour_reach(0.1, None) == -1


def test_lattice_closed_form_on_a_small_replica():
    """the scene of the large GPU cases (boxes on a lattice, clipped by the far faces) at small sizes: the closed-form count and the
    per-cell closed form against by_neighbours at every reach >= 1"""
    for shape, period, size in (((12, 11, 10), 5, 3), ((13, 9, 16), 6, 5), ((7, 8, 9), 4, 1), ((10, 10, 11), 5, 4), ((5, 5, 5), 9, 4),
                                ((6, 7, 8), 3, 2)):
        occ, keys = CR.lattice_scene(shape, period, size)
        assert len(np.unique(keys)) > 1
        for reach in (1, 2, 3):
            idx, k = CR.by_neighbours(occ, keys, reach)
            assert len(idx) == CR.lattice_contour_count(shape, period, size), (shape, period, size, reach)
            every = np.arange(int(np.prod(shape)))
            assert np.array_equal(np.flatnonzero(CR.lattice_drawn(shape, period, size, every)), idx)
            assert np.array_equal(k, keys.reshape(-1)[idx]) and np.array_equal(CR.lattice_key(shape, period, idx.astype(np.int64)), k)
            t = torch.from_numpy(every)
            assert np.array_equal(CR.lattice_drawn(shape, period, size, t).numpy(), CR.lattice_drawn(shape, period, size, every))
            assert np.array_equal(CR.lattice_key(shape, period, t).numpy(), CR.lattice_key(shape, period, every))
