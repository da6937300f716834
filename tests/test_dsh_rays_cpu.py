"""A frame of sensor rays without a GPU (include/sdfgpu.h "Sensor rays"): the restatement
(tests/dsh_rays_restated.py) against hand-worked walks, the properties every walk has, an exact judge in fractions.Fraction, the
header's names, and the host-side sizing arithmetic in a stand-alone program under -fsanitize=address,undefined
(tests/dsh_rays_plan_harness.cpp)."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dsh_restated as R
import dsh_rays_restated as RR
from sdf_tools_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREE, HIT = R.record(0.0, 1), R.record(1.0, 2)


def cells_of(gs, ge):
    return [c for c, _ in RR.walk(list(map(float, gs)), list(map(float, ge)))]


# ---- hand-worked walks ----------------------------------------------------------------------------------------------------------------
def test_a_tie_at_every_step_goes_x_then_y_then_z():
    got = RR.walk([0.5, 0.5, 0.5], [8.5, 8.5, 8.5])
    want = [(0, 0, 0)]
    for k in range(1, 9):
        want += [(k, k - 1, k - 1), (k, k, k - 1), (k, k, k)]
    assert [c for c, _ in got] == want
    # the three steps into diagonal cell k share the parameter (k - 0.5) / 8, which is exact
    assert [t for _, t in got] == [0.0] + [(k - 0.5) / 8 for k in range(1, 9) for _ in range(3)]


def test_a_ray_along_a_cell_face_stays_on_the_upper_side_of_it():
    assert cells_of((0.5, 1.0, 0.5), (4.5, 1.0, 0.5)) == [(x, 1, 0) for x in range(5)]
    assert cells_of((0.5, 2.0, 0.5), (2.5, 2.0, 2.5)) == [(0, 2, 0), (1, 2, 0), (1, 2, 1), (2, 2, 1), (2, 2, 2)]
    assert cells_of((0.5, -3.0, 0.5), (0.5, -3.0, -1.5)) == [(0, -3, 0), (0, -3, -1), (0, -3, -2)]


def test_negative_directions_from_an_integer_corner():
    got = RR.walk([2.0, 2.0, 2.0], [-0.5, -0.5, -0.5])
    # the corner belongs to cell (2, 2, 2); the first three crossings are at the start itself (-0.0 / 2.5), then 0.4, then 0.8
    assert [c for c, _ in got] == [(2, 2, 2), (1, 2, 2), (1, 1, 2), (1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 0, 0), (-1, 0, 0), (-1, -1, 0), (-1, -1, -1)]
    assert [t for _, t in got] == [0.0, 0.0, 0.0, 0.0, 0.4, 0.4, 0.4, 0.8, 0.8, 0.8]


def test_a_ray_inside_one_cell_carves_nothing_and_hits_it():
    assert RR.walk([0.25, 0.25, 0.25], [0.75, 0.5, 0.25]) == [((0, 0, 0), 0.0)]
    assert RR.ray([0.25, 0.25, 0.25], [0.75, 0.5, 0.25], 4.0) == (RR.RAY_HIT, [], (0, 0, 0))
    assert RR.ray([0.25, 0.25, 0.25], [0.25, 0.25, 0.25], 0.001) == (RR.RAY_HIT, [], (0, 0, 0))       # length 0 is not long
    # the same cell, but longer than the range: the sensor's cell is carved (t_0 = 0 is always in range) and nothing is hit
    assert RR.ray([0.25, 0.25, 0.25], [0.75, 0.5, 0.25], 0.125) == (RR.RAY_TRUNCATED, [(0, 0, 0)], None)


def test_a_long_ray_whose_prefix_ends_mid_way():
    # cell x is entered at distance x - 0.5: 2.5 is in range 3, 3.5 is not
    assert RR.ray([0.5, 0.5, 0.5], [10.5, 0.5, 0.5], 3.0) == (RR.RAY_TRUNCATED, [(x, 0, 0) for x in range(4)], None)
    assert RR.ray([0.5, 0.5, 0.5], [10.5, 0.5, 0.5], 2.5) == (RR.RAY_TRUNCATED, [(x, 0, 0) for x in range(4)], None)   # (0.25^2 * 100 <= 6.25)
    assert RR.ray([0.5, 0.5, 0.5], [10.5, 0.5, 0.5], 0.25) == (RR.RAY_TRUNCATED, [(0, 0, 0)], None)
    assert RR.ray([0.5, 0.5, 0.5], [-9.5, 0.5, 0.5], 3.0) == (RR.RAY_TRUNCATED, [(-x, 0, 0) for x in range(4)], None)


def test_a_long_ray_whose_end_cell_is_still_in_range():
    # length 3.4 > 3, but the end's cell is entered at distance 2.5: the whole walk is carved, end cell included, and nothing is hit
    assert RR.ray([0.5, 0.5, 0.5], [3.9, 0.5, 0.5], 3.0) == (RR.RAY_TRUNCATED, [(x, 0, 0) for x in range(4)], None)
    assert RR.ray([0.5, 0.5, 0.5], [3.9, 0.5, 0.5], 3.5) == (RR.RAY_HIT, [(x, 0, 0) for x in range(3)], (3, 0, 0))


def test_the_frame_on_a_map_hits_win_and_refusals_write_nothing():
    m = R.Map(cell_size=0.5, chunk_dims=(2, 2, 2), default=R.record(0.5, 9))
    m.set_chunk((-0.75, 0.25, 0.25), R.record(1.0, 4))                       # chunk (-1, 0, 0): chunk-filled
    pts = np.array([(2.25, 0.25, 0.25), (1.25, 0.25, 0.25), (np.nan, 0, 0), (-0.75, 0.25, 0.25), (50.0, 0.25, 0.25)], np.float32)
    st, counts = RR.insert_rays(m, (0.25, 0.25, 0.25), pts, 2.0, FREE, HIT)
    assert st.tolist() == [1, 1, 0, 1, 2]
    # cells x = 0 .. 4 at 0.5 a cell: ray 0 carves 0 .. 3 and hits 4, ray 1 carves 0, 1 and hits 2 (which ray 0 carved: the hit wins),
    # ray 3 carves 0, -1 and hits -2, ray 4 is long and carves x = 0 .. 4 (cell 4 is entered at 3.5 of the 4 cells of range), hits nothing
    assert counts == {"rays_hit": 3, "rays_truncated": 1, "rays_skipped": 1, "cells_carved": 4 + 2 + 2 + 5, "new_chunks": 3}
    assert [m.get_cell((x, 0, 0))[0] for x in range(-2, 6)] == [HIT, FREE, FREE, FREE, HIT, FREE, HIT, R.record(0.5, 9)]
    assert m.get_cell((-2, 1, 0)) == (R.record(1.0, 4), R.FOUND_IN_CELL)       # the chunk-filled chunk keeps its record elsewhere
    assert m.get_cell((5, 1, 1)) == (R.record(0.5, 9), R.FOUND_IN_CELL) and m.get_cell((6, 0, 0))[1] == R.NOT_FOUND
    before = {c: (k, np.copy(w)) for c, (k, w) in m.chunks.items()}
    for sensor, max_range in [((np.nan, 0, 0), 1.0), ((0, np.inf, 0), 1.0), ((2.0 ** 21, 0, 0), 1.0), ((0, 0, 0), 0.0), ((0, 0, 0), -1.0),
                              ((0, 0, 0), np.nan), ((0, 0, 0), 32768.0 + 0.01), ((0, 0, 0), np.inf)]:
        with pytest.raises(RR.Refused):
            RR.insert_rays(m, sensor, pts, max_range, FREE, HIT)
    assert before.keys() == m.chunks.keys() and all(np.array_equal(before[c][1], m.chunks[c][1]) for c in before)
    RR.insert_rays(m, (0.25, 0.25, 0.25), pts[:0], 32768.0, FREE, HIT)                                   # 65536 cells: the largest range


# ---- properties and the exact judge -------------------------------------------------------------------------------------------------
def ray_lists():
    rng = np.random.default_rng(30)
    rays = []
    for _ in range(150):                                                      # anywhere, a few cells long
        s = rng.uniform(-20, 20, 3)
        rays.append((s, s + rng.uniform(-12, 12, 3)))
    for _ in range(80):                                                       # ends on the half-integer lattice: ties and boundary hits
        s = rng.integers(-8, 8, 3) / 2.0
        rays.append((s, s + rng.integers(-14, 14, 3) / 2.0))
    for _ in range(40):                                                       # axis-parallel and face-diagonal
        s = rng.integers(-8, 8, 3) / 2.0
        d = rng.integers(-9, 9, 3).astype(np.float64)
        d[rng.integers(0, 3)] = 0.0
        rays.append((s, s + d))
    long_rays = []
    for k in range(12):                                                       # up to 1000 cells along one axis, a few across
        s = rng.uniform(-3, 3, 3)
        d = rng.uniform(-3, 3, 3)
        d[k % 3] = rng.choice([-1, 1]) * rng.uniform(300, 1000)
        long_rays.append((s, s + d))
    return [(list(map(float, s)), list(map(float, e))) for s, e in rays], [(list(map(float, s)), list(map(float, e))) for s, e in long_rays]


RAYS, LONG_RAYS = ray_lists()


def test_properties_of_every_walk():
    for gs, ge in RAYS + LONG_RAYS:
        got = RR.walk(gs, ge)
        i0, i1 = [math.floor(v) for v in gs], [math.floor(v) for v in ge]
        assert len(got) == sum(abs(b - a) for a, b in zip(i0, i1)) + 1
        assert got[0] == (tuple(i0), 0.0) and got[-1][0] == tuple(i1)
        for (a, ta), (b, tb) in zip(got, got[1:]):
            assert sorted(abs(x - y) for x, y in zip(a, b)) == [0, 0, 1]
            assert ta <= tb <= 1.0
        # the range prefix: what ray() carves of a long ray is a prefix, and the ray that is not long has every cell in range
        len2 = RR.length2(gs, ge)
        for r in (0.4, 3.0, math.sqrt(len2) * 0.5, math.sqrt(len2) * 2 + 1):
            status, carved, hit = RR.ray(gs, ge, r)
            cells = [c for c, _ in got]
            assert carved == cells[:len(carved)]
            in_range = [(t * t) * len2 <= r * r for _, t in got]
            assert in_range == sorted(in_range, reverse=True)
            if status == RR.RAY_HIT:
                assert all(in_range) and carved == cells[:-1] and hit == cells[-1]
            else:
                assert hit is None and len(carved) == sum(in_range) >= 1


EPS = Fraction(1, 1 << 30)


def meets(gs, d, lo, hi):
    """does the exact segment gs + t d, t in [0, 1], meet the box [lo, hi] (Fractions)"""
    t0, t1 = Fraction(0), Fraction(1)
    for a in range(3):
        if d[a] == 0:
            if not lo[a] <= gs[a] <= hi[a]:
                return False
            continue
        ta, tb = (lo[a] - gs[a]) / d[a], (hi[a] - gs[a]) / d[a]
        if ta > tb:
            ta, tb = tb, ta
        t0, t1 = max(t0, ta), min(t1, tb)
        if t0 > t1:
            return False
    return True


def judge(gs, ge):
    """every visited cell's cube grown by EPS meets the exact segment; every cell of the bounding box whose cube shrunk by EPS meets it
    is visited (where the box has at most 20 000 cells)"""
    fs, fe = [Fraction(v) for v in gs], [Fraction(v) for v in ge]            # the exact rationals the doubles are
    d = [e - s for s, e in zip(fs, fe)]
    visited = [c for c, _ in RR.walk(gs, ge)]
    for c in visited:
        assert meets(fs, d, [Fraction(v) - EPS for v in c], [Fraction(v) + 1 + EPS for v in c]), (gs, ge, c)
    lo = [min(math.floor(a), math.floor(b)) for a, b in zip(gs, ge)]
    hi = [max(math.floor(a), math.floor(b)) for a, b in zip(gs, ge)]
    if np.prod([h - l + 1 for l, h in zip(lo, hi)]) > 20000:
        return False
    seen = set(visited)
    for x in range(lo[0], hi[0] + 1):
        for y in range(lo[1], hi[1] + 1):
            for z in range(lo[2], hi[2] + 1):
                if (x, y, z) not in seen:
                    c = (x, y, z)
                    assert not meets(fs, d, [Fraction(v) + EPS for v in c], [Fraction(v) + 1 - EPS for v in c]), (gs, ge, c)
    return True


def test_the_exact_judge_on_random_lattice_and_tie_rays():
    ties = [([0.5, 0.5, 0.5], [8.5, 8.5, 8.5]), ([2.0, 2.0, 2.0], [-0.5, -0.5, -0.5]), ([0.5, 1.0, 0.5], [4.5, 1.0, 0.5]), ([0.0, 0.0, 0.0], [-3.0, 5.0, -7.0]),
            ([0.25, 0.25, 0.25], [0.75, 0.5, 0.25])]
    assert all(judge(gs, ge) for gs, ge in RAYS + ties)


def test_the_exact_judge_on_rays_of_up_to_a_thousand_cells():
    assert sum(judge(gs, ge) for gs, ge in LONG_RAYS) >= 8                    # (the visited half is judged for every one of them)


# ---- the header and the library ----------------------------------------------------------------------------------------------------------
def test_header_names_struct_layout_and_exports():
    hdr = open(os.path.join(ROOT, "include", "sdfgpu.h")).read()
    assert "SDFGPU_DSH_RAY_SKIPPED = 0, SDFGPU_DSH_RAY_HIT = 1, SDFGPU_DSH_RAY_TRUNCATED = 2" in hdr
    assert (capi.DSH_RAY_SKIPPED, capi.DSH_RAY_HIT, capi.DSH_RAY_TRUNCATED) == (RR.RAY_SKIPPED, RR.RAY_HIT, RR.RAY_TRUNCATED) == (0, 1, 2)
    src, exe = os.path.join(ROOT, "tests", "dsh_rays_layout_probe.c"), os.path.join(ROOT, "tests", "dsh_rays_layout_probe")
    names = capi.DSH_RAY_COUNTS_DTYPE.names
    assert names == ("rays_hit", "rays_truncated", "rays_skipped", "cells_carved", "new_chunks")
    body = 'printf("size %zu\\n", sizeof(sdfgpu_dsh_ray_counts));\n' + "".join('printf("%s %%zu\\n", offsetof(sdfgpu_dsh_ray_counts, %s));\n' % (f, f) for f in names)
    body += 'printf("status %d %d %d\\n", SDFGPU_DSH_RAY_SKIPPED, SDFGPU_DSH_RAY_HIT, SDFGPU_DSH_RAY_TRUNCATED);\n'
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "sdfgpu.h"\nint main(void) {\n%sreturn 0;\n}\n' % body)
    try:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split(None, 1) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    finally:
        for p in (src, exe):
            if os.path.exists(p):
                os.remove(p)
    assert int(got["size"]) == capi.DSH_RAY_COUNTS_DTYPE.itemsize == 40 and got["status"] == "0 1 2"
    for f in names:
        assert int(got[f]) == capi.DSH_RAY_COUNTS_DTYPE.fields[f][1]
    for name in ("sdfgpu_dsh_insert_rays_device", "sdfgpu_dsh_insert_rays"):
        assert name in capi.EXPORTS and hasattr(capi.load_library(), name)


# ---- the host arithmetic under the sanitizers --------------------------------------------------------------------------------------------
def test_the_frame_sizing_arithmetic_under_asan_and_ubsan():
    tests = os.path.join(ROOT, "tests")
    exe = os.path.join(tests, "dsh_rays_plan_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(tests, "dsh_rays_plan_harness.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "dsh rays plan OK" in r.stdout, r.stdout + r.stderr
