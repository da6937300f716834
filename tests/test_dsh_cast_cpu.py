"""Ray casts without a GPU (include/sdfgpu.h "Ray casts"): the restatement (tests/dsh_cast_restated.py) against
hand-worked rays, against an independent route (the first walk cell whose bit is set in the predicate of Map.window over the rays'
bounding box), and the header's layout and names."""
import math
import os
import subprocess

import numpy as np

import dsh_cast_restated as C
import dsh_restated as R
import dsh_rays_restated as RR
from sdf_tools_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREE, FILLED, UNKNOWN = R.record(0.0, 1), R.record(1.0, 2), R.record(0.5, 3)
BOTH = C.SKIP_FIRST | C.SKIP_LAST


def cast(m, gs, ge, r=100.0, flags=0):
    """one ray in grid coordinates on a map of unit cells at the identity: (status, cell, record, t, step, found)"""
    status, (cell, record, t, step, found) = C.cast(m, list(map(float, gs)), list(map(float, ge)), float(r), flags)
    return status, cell, record, t, step, found


def free_map(**kw):
    return R.Map(default=FREE, **kw)


# ---- the hand-worked walks of tests/test_dsh_rays_cpu.py, cast ----------------------------------------------------------------------------
def test_the_tie_diagonal_clear_and_blocked_at_each_of_a_steps_three_cells():
    gs, ge = (0.5, 0.5, 0.5), (8.5, 8.5, 8.5)
    m = free_map(chunk_dims=(3, 2, 5))
    assert cast(m, gs, ge) == (C.CAST_CLEAR, (8, 8, 8), FREE, 7.5 / 8, 24, R.NOT_FOUND)
    # the walk enters (3, 2, 2), (3, 3, 2), (3, 3, 3) at the same parameter 2.5 / 8, in that order: x before y before z
    for k, c in enumerate([(3, 2, 2), (3, 3, 2), (3, 3, 3)]):
        b = free_map(chunk_dims=(3, 2, 5))
        RR.set_cell_index(b, c, FILLED)
        assert cast(b, gs, ge) == (C.CAST_BLOCKED, c, FILLED, 2.5 / 8, 7 + k, R.FOUND_IN_CELL)
    b = free_map(chunk_dims=(3, 2, 5))
    for c in [(3, 3, 2), (3, 2, 2), (5, 5, 5)]:
        RR.set_cell_index(b, c, FILLED)
    assert cast(b, gs, ge)[1:5:3] == ((3, 2, 2), 7), "the first blocker in walk order"
    RR.set_cell_index(b, (2, 3, 2), FILLED)                                  # beside the walk: never visited
    assert cast(b, gs, ge)[1] == (3, 2, 2)


def test_face_rays_see_the_upper_side_of_the_face():
    m = free_map()
    RR.set_cell_index(m, (2, 0, 0), FILLED)                                   # below the face y = 1: not on the walk
    assert cast(m, (0.5, 1.0, 0.5), (4.5, 1.0, 0.5)) == (C.CAST_CLEAR, (4, 1, 0), FREE, 3.5 / 4, 4, R.FOUND_IN_CELL)
    RR.set_cell_index(m, (2, 1, 0), FILLED)
    assert cast(m, (0.5, 1.0, 0.5), (4.5, 1.0, 0.5)) == (C.CAST_BLOCKED, (2, 1, 0), FILLED, 1.5 / 4, 2, R.FOUND_IN_CELL)
    d = free_map()
    RR.set_cell_index(d, (1, 2, 1), FILLED)                                   # (0,2,0) (1,2,0) (1,2,1) (2,2,1) (2,2,2): x before z at the ties
    assert cast(d, (0.5, 2.0, 0.5), (2.5, 2.0, 2.5)) == (C.CAST_BLOCKED, (1, 2, 1), FILLED, 0.25, 2, R.FOUND_IN_CELL)


def test_negative_directions_from_an_integer_corner():
    m = free_map(chunk_dims=(2, 2, 2))
    gs, ge = (2.0, 2.0, 2.0), (-0.5, -0.5, -0.5)
    assert cast(m, gs, ge) == (C.CAST_CLEAR, (-1, -1, -1), FREE, 0.8, 9, R.NOT_FOUND)
    RR.set_cell_index(m, (1, 1, 2), FILLED)                                   # entered at the start itself: t = 0, step 2
    assert cast(m, gs, ge) == (C.CAST_BLOCKED, (1, 1, 2), FILLED, 0.0, 2, R.FOUND_IN_CELL)
    assert cast(m, gs, ge, flags=C.SKIP_FIRST)[1] == (1, 1, 2), "SKIP_FIRST leaves out c_0 only, not the cells entered at t = 0"
    RR.set_cell_index(m, (1, 1, 2), FREE)
    RR.set_cell_index(m, (-1, 0, 0), FILLED)
    assert cast(m, gs, ge) == (C.CAST_BLOCKED, (-1, 0, 0), FILLED, 0.8, 7, R.FOUND_IN_CELL)


def test_a_ray_inside_one_cell_has_n_zero():
    gs, ge = (0.25, 0.25, 0.25), (0.75, 0.5, 0.25)
    m = free_map()
    RR.set_cell_index(m, (0, 0, 0), FILLED)
    assert cast(m, gs, ge) == (C.CAST_BLOCKED, (0, 0, 0), FILLED, 0.0, 0, R.FOUND_IN_CELL)
    # c_0 is c_N: either skip leaves the one cell out, and the record still describes it
    for flags in (C.SKIP_FIRST, C.SKIP_LAST, BOTH):
        assert cast(m, gs, ge, flags=flags) == (C.CAST_CLEAR, (0, 0, 0), FILLED, 0.0, 0, R.FOUND_IN_CELL)
    # longer than the range: W is c_0 alone, which is also c_N
    assert cast(m, gs, ge, r=0.125) == (C.CAST_BLOCKED, (0, 0, 0), FILLED, 0.0, 0, R.FOUND_IN_CELL)
    assert cast(m, gs, ge, r=0.125, flags=BOTH) == (C.CAST_CLEAR_IN_RANGE, (0, 0, 0), FILLED, 0.0, 0, R.FOUND_IN_CELL)


# ---- blockers, skips and ranges along one line ----------------------------------------------------------------------------------------------
LINE = ((0.5, 0.5, 0.5), (10.5, 0.5, 0.5))                                     # cells x = 0 .. 10, cell x entered at (x - 0.5) / 10


def line_map(filled, **kw):
    m = free_map(**kw)
    for x in filled:
        RR.set_cell_index(m, (x, 0, 0), FILLED)
    return m


def test_blockers_at_the_start_the_end_and_between_under_the_skips():
    m = line_map([0, 4, 10])
    assert cast(m, *LINE) == (C.CAST_BLOCKED, (0, 0, 0), FILLED, 0.0, 0, R.FOUND_IN_CELL)
    assert cast(m, *LINE, flags=C.SKIP_LAST)[1] == (0, 0, 0)
    assert cast(m, *LINE, flags=C.SKIP_FIRST) == (C.CAST_BLOCKED, (4, 0, 0), FILLED, 0.35, 4, R.FOUND_IN_CELL)
    ends = line_map([0, 10])
    assert cast(ends, *LINE, flags=C.SKIP_FIRST) == (C.CAST_BLOCKED, (10, 0, 0), FILLED, 0.95, 10, R.FOUND_IN_CELL)
    assert cast(ends, *LINE, flags=BOTH) == (C.CAST_CLEAR, (10, 0, 0), FILLED, 0.95, 10, R.FOUND_IN_CELL), "clear between the ends; the record is c_N's"
    assert cast(line_map([9]), *LINE, flags=BOTH)[:2] == (C.CAST_BLOCKED, (9, 0, 0))
    assert cast(line_map([1]), *LINE, flags=BOTH)[:2] == (C.CAST_BLOCKED, (1, 0, 0))


def test_long_rays_stop_at_the_range_and_skip_last_needs_the_end_cell():
    m = line_map([4, 10])
    # range 3: cell 3 is entered at 2.5, cell 4 at 3.5 -> W = cells 0 .. 3, clear in range, described by cell 3
    assert cast(m, *LINE, r=3.0) == (C.CAST_CLEAR_IN_RANGE, (3, 0, 0), FREE, 0.25, 3, R.FOUND_IN_CELL)
    assert cast(m, *LINE, r=3.5) == (C.CAST_BLOCKED, (4, 0, 0), FILLED, 0.35, 4, R.FOUND_IN_CELL)
    assert cast(m, *LINE, r=0.25) == (C.CAST_CLEAR_IN_RANGE, (0, 0, 0), FREE, 0.0, 0, R.FOUND_IN_CELL)
    # SKIP_LAST on a long ray that never reaches c_N leaves nothing out: the last cell of W is tested
    cut = line_map([3, 10])
    assert cast(cut, *LINE, r=3.0, flags=C.SKIP_LAST)[:2] == (C.CAST_BLOCKED, (3, 0, 0))
    # a long ray whose in-range prefix reaches c_N: length 9.7 > 9.6, but cell 10 is entered at 9.5
    gs, ge = (0.5, 0.5, 0.5), (10.2, 0.5, 0.5)
    reach = line_map([10])
    t10 = 9.5 / (10.2 - 0.5)
    assert cast(reach, gs, ge, r=9.6) == (C.CAST_BLOCKED, (10, 0, 0), FILLED, t10, 10, R.FOUND_IN_CELL)
    assert cast(reach, gs, ge, r=9.6, flags=C.SKIP_LAST) == (C.CAST_CLEAR_IN_RANGE, (10, 0, 0), FILLED, t10, 10, R.FOUND_IN_CELL)
    assert cast(reach, gs, ge, r=9.7)[0] == C.CAST_BLOCKED and cast(reach, gs, ge, r=9.7, flags=C.SKIP_LAST)[0] == C.CAST_CLEAR


# ---- the predicate ---------------------------------------------------------------------------------------------------------------------------
def test_the_occupancy_values_that_block():
    def hit_with(record, flags=0):
        m = free_map()
        RR.set_cell_index(m, (4, 0, 0), record)
        return cast(m, *LINE, flags=flags)
    assert hit_with(UNKNOWN)[0] == C.CAST_CLEAR
    assert hit_with(UNKNOWN, C.UNKNOWN_IS_FILLED) == (C.CAST_BLOCKED, (4, 0, 0), UNKNOWN, 0.35, 4, R.FOUND_IN_CELL)
    above, below = R.record_bits(0x3F000001, 7), R.record_bits(0x3EFFFFFF, 7)   # the floats next to 0.5
    assert hit_with(above)[0] == C.CAST_BLOCKED and hit_with(below, C.UNKNOWN_IS_FILLED)[0] == C.CAST_CLEAR
    for bits in (0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001):             # NaNs, quiet and signalling, never block
        for flags in (0, C.UNKNOWN_IS_FILLED):
            assert hit_with(R.record_bits(bits, 9), flags)[0] == C.CAST_CLEAR
    for bits in (0x00000000, 0x80000000, 0xFF800000, 0xBF800000):             # +0, -0, -inf, -1
        assert hit_with(R.record_bits(bits, 9), C.UNKNOWN_IS_FILLED)[0] == C.CAST_CLEAR
    assert hit_with(R.record_bits(0x7F800000, 0xFFFFFFFF)) == (C.CAST_BLOCKED, (4, 0, 0), R.record_bits(0x7F800000, 0xFFFFFFFF), 0.35, 4, R.FOUND_IN_CELL)
    assert hit_with(R.record_bits(0x3F000000, 0xFFFFFFFF))[0] == C.CAST_CLEAR, "the component word takes no part"


def test_defaults_and_chunk_filled_chunks():
    # a blocking default: absent space blocks at once, NOT_FOUND, and SKIP_FIRST moves the hit to c_1 of the same absent chunk
    m = R.Map(default=FILLED, chunk_dims=(4, 4, 4))
    assert cast(m, *LINE) == (C.CAST_BLOCKED, (0, 0, 0), FILLED, 0.0, 0, R.NOT_FOUND)
    assert cast(m, *LINE, flags=C.SKIP_FIRST) == (C.CAST_BLOCKED, (1, 0, 0), FILLED, 0.05, 1, R.NOT_FOUND)
    u = R.Map(default=UNKNOWN, chunk_dims=(4, 4, 4))
    assert cast(u, *LINE) == (C.CAST_CLEAR, (10, 0, 0), UNKNOWN, 0.95, 10, R.NOT_FOUND)
    assert cast(u, *LINE, flags=C.UNKNOWN_IS_FILLED | C.SKIP_FIRST) == (C.CAST_BLOCKED, (1, 0, 0), UNKNOWN, 0.05, 1, R.NOT_FOUND)
    # a blocking chunk-filled chunk entered mid-walk: chunk 1 holds x = 4 .. 7
    f = free_map(chunk_dims=(4, 4, 4))
    f.set_chunk((5.5, 0.5, 0.5), R.record(0.75, 11))
    assert cast(f, *LINE) == (C.CAST_BLOCKED, (4, 0, 0), R.record(0.75, 11), 0.35, 4, R.FOUND_IN_CHUNK)
    # started inside it: SKIP_FIRST moves the hit to c_1, still in the chunk; started in its last cell, the free chunk behind is clear
    assert cast(f, (5.5, 0.5, 0.5), (10.5, 0.5, 0.5), flags=C.SKIP_FIRST) == (C.CAST_BLOCKED, (6, 0, 0), R.record(0.75, 11), 0.1, 1, R.FOUND_IN_CHUNK)
    assert cast(f, (7.5, 0.5, 0.5), (10.5, 0.5, 0.5), flags=C.SKIP_FIRST)[:2] == (C.CAST_CLEAR, (10, 0, 0))
    # a free chunk-filled chunk is walked through; a cell-filled chunk behind it blocks
    g = R.Map(default=FILLED, chunk_dims=(4, 4, 4))
    g.set_chunk((1.5, 0.5, 0.5), FREE)
    g.set_chunk((5.5, 0.5, 0.5), R.record(0.25, 5))
    g.set_cell((8.5, 1.5, 0.5), FREE)                                          # chunk 2 becomes cell-filled with the blocking default
    assert cast(g, *LINE) == (C.CAST_BLOCKED, (8, 0, 0), FILLED, 0.75, 8, R.FOUND_IN_CELL)
    assert cast(g, (0.5, 0.5, 0.5), (7.5, 0.5, 0.5)) == (C.CAST_CLEAR, (7, 0, 0), R.record(0.25, 5), 6.5 / 7, 7, R.FOUND_IN_CHUNK)


def test_the_frame_forms_skips_refusals_and_distance():
    m = R.Map(cell_size=0.5, chunk_dims=(2, 2, 2), default=UNKNOWN)
    RR.insert_rays(m, (0.25, 0.25, 0.25), np.array([(2.25, 0.25, 0.25)], np.float32), 10.0, FREE, FILLED)
    pts = np.array([(3.25, 0.25, 0.25), (1.25, 0.25, 0.25), (np.nan, 0, 0), (2.0 ** 21, 0, 0), (50.0, 0.25, 0.25)], np.float32)
    st, hits = C.cast_rays(m, (0.25, 0.25, 0.25), pts, 2.5, 0)
    assert st.tolist() == [C.CAST_BLOCKED, C.CAST_CLEAR, C.CAST_SKIPPED, C.CAST_SKIPPED, C.CAST_BLOCKED]
    assert hits["cell"].tolist() == [[4, 0, 0], [2, 0, 0], [0, 0, 0], [0, 0, 0], [4, 0, 0]] and hits["step"].tolist() == [4, 2, 0, 0, 4]
    assert hits[2].tobytes() == bytes(48) and hits.dtype.itemsize == 48
    assert hits["t"][0] == 3.5 / 6 and C.distance((0.25, 0.25, 0.25), pts[0], hits["t"][0]) == (3.5 / 6) * 3.0
    st2, hits2 = C.cast_segments(m, [(0.25, 0.25, 0.25)] * 5, pts.astype(np.float64), 2.5, 0)
    assert np.array_equal(st, st2) and hits.tobytes() == hits2.tobytes(), "a segment from the sensor is the frame's ray"
    st3, _ = C.cast_segments(m, [(np.inf, 0, 0), (0.25, 0.25, 0.25), (-2.0 ** 21, 0, 0)], [(0.25, 0.25, 0.25), (0.25, np.nan, 0.25), (0.25, 0.25, 0.25)], 2.5, 0)
    assert st3.tolist() == [0, 0, 0]
    for sensor, max_range, flags in [((np.nan, 0, 0), 1.0, 0), ((2.0 ** 21, 0, 0), 1.0, 0), ((0, 0, 0), 0.0, 0), ((0, 0, 0), -1.0, 0), ((0, 0, 0), np.nan, 0),
                                     ((0, 0, 0), 32768.01, 0), ((0, 0, 0), 1.0, 8), ((0, 0, 0), 1.0, 1 << 31)]:
        try:
            C.cast_rays(m, sensor, pts, max_range, flags)
        except C.Refused:
            continue
        raise AssertionError("not refused: %r" % ((sensor, max_range, flags),))
    C.cast_rays(m, (0, 0, 0), pts[:0], 32768.0, 7)                             # 65536 cells and all three flags: the largest call


# ---- an independent route: the window's predicate ---------------------------------------------------------------------------------------------
def test_random_maps_and_rays_against_the_first_set_bit_of_the_window():
    rng = np.random.default_rng(330)
    totals = {C.CAST_BLOCKED: 0, C.CAST_CLEAR: 0, C.CAST_CLEAR_IN_RANGE: 0}
    for case in range(6):
        dims = [(1, 1, 1), (3, 2, 5), (4, 4, 4)][case % 3]
        m = R.Map(chunk_dims=dims, default=[FREE, UNKNOWN][case % 2])
        m.set_chunks(rng.uniform(-9, 9, (12, 3)), np.array([[FREE, FILLED, UNKNOWN][k % 3] for k in range(12)], np.uint64))
        m.set_cells(rng.uniform(-9, 9, (150, 3)), np.array([[FILLED, FREE, UNKNOWN, R.record_bits(0x7FC00000)][k % 4] for k in range(150)], np.uint64))
        s = rng.uniform(-6, 6, (60, 3))
        e = s + rng.uniform(-7, 7, (60, 3))
        e[::7] = np.floor(e[::7])                                              # some ends on the lattice
        lower = np.floor(np.minimum(s, e).min(0)).astype(int)
        shape = tuple(int(v) for v in np.floor(np.maximum(s, e).max(0)).astype(int) - lower + 1)
        window = m.window(lower, shape)
        for flags in range(8):
            bits = R.classify(window, flags & C.UNKNOWN_IS_FILLED)
            r = [2.5, 5.0, 100.0][flags % 3]
            st, hits = C.cast_segments(m, s, e, r, flags)
            for k in range(len(s)):
                cells = RR.walk(list(map(float, s[k])), list(map(float, e[k])))
                n_steps = len(cells) - 1
                is_long = RR.length2(list(map(float, s[k])), list(map(float, e[k]))) > r * r
                want = None
                for j, (c, t) in enumerate(cells):
                    if is_long and not (t * t) * RR.length2(list(map(float, s[k])), list(map(float, e[k]))) <= r * r:
                        break
                    if (j == 0 and flags & C.SKIP_FIRST) or (j == n_steps and flags & C.SKIP_LAST):
                        continue
                    if bits[tuple(np.subtract(c, lower))]:
                        want = (c, j)
                        break
                totals[int(st[k])] += 1
                if want is None:
                    assert st[k] == (C.CAST_CLEAR_IN_RANGE if is_long else C.CAST_CLEAR)
                else:
                    assert st[k] == C.CAST_BLOCKED and tuple(hits["cell"][k]) == want[0] and hits["step"][k] == want[1]
                    assert int(hits["record"][k]) == int(window[tuple(np.subtract(want[0], lower))])
    assert min(totals.values()) > 200, totals


# ---- the header and the library -------------------------------------------------------------------------------------------------------------
def test_header_layout_enum_values_and_exports():
    hdr = open(os.path.join(ROOT, "include", "sdfgpu.h")).read()
    assert "SDFGPU_DSH_CAST_SKIPPED = 0, SDFGPU_DSH_CAST_CLEAR = 1, SDFGPU_DSH_CAST_CLEAR_IN_RANGE = 2, SDFGPU_DSH_CAST_BLOCKED = 3" in hdr
    assert "SDFGPU_DSH_CAST_SKIP_FIRST = 1, SDFGPU_DSH_CAST_SKIP_LAST = 2, SDFGPU_DSH_CAST_UNKNOWN_IS_FILLED = 4" in hdr
    assert "#define SDFGPU_DSH_CAST" not in hdr
    assert (capi.DSH_CAST_SKIPPED, capi.DSH_CAST_CLEAR, capi.DSH_CAST_CLEAR_IN_RANGE, capi.DSH_CAST_BLOCKED) == (
        C.CAST_SKIPPED, C.CAST_CLEAR, C.CAST_CLEAR_IN_RANGE, C.CAST_BLOCKED) == (0, 1, 2, 3)
    assert (capi.DSH_CAST_SKIP_FIRST, capi.DSH_CAST_SKIP_LAST, capi.DSH_CAST_UNKNOWN_IS_FILLED) == (C.SKIP_FIRST, C.SKIP_LAST, C.UNKNOWN_IS_FILLED) == (1, 2, 4)
    assert capi.DSH_CAST_HIT_DTYPE == C.HIT_DTYPE
    src, exe = os.path.join(ROOT, "tests", "dsh_cast_layout_probe.c"), os.path.join(ROOT, "tests", "dsh_cast_layout_probe")
    names = capi.DSH_CAST_HIT_DTYPE.names
    assert names == ("cell", "record", "t", "step", "found")
    body = 'printf("size %zu\\n", sizeof(sdfgpu_dsh_cast_hit));\n' + "".join('printf("%s %%zu\\n", offsetof(sdfgpu_dsh_cast_hit, %s));\n' % (f, f) for f in names)
    body += 'printf("status %d %d %d %d\\n", SDFGPU_DSH_CAST_SKIPPED, SDFGPU_DSH_CAST_CLEAR, SDFGPU_DSH_CAST_CLEAR_IN_RANGE, SDFGPU_DSH_CAST_BLOCKED);\n'
    body += 'printf("flags %d %d %d\\n", SDFGPU_DSH_CAST_SKIP_FIRST, SDFGPU_DSH_CAST_SKIP_LAST, SDFGPU_DSH_CAST_UNKNOWN_IS_FILLED);\n'
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "sdfgpu.h"\nint main(void) {\n%sreturn 0;\n}\n' % body)
    try:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split(None, 1) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    finally:
        for p in (src, exe):
            if os.path.exists(p):
                os.remove(p)
    assert int(got["size"]) == capi.DSH_CAST_HIT_DTYPE.itemsize == 48 and got["status"] == "0 1 2 3" and got["flags"] == "1 2 4"
    assert [int(got[f]) for f in names] == [capi.DSH_CAST_HIT_DTYPE.fields[f][1] for f in names] == [0, 24, 32, 40, 44]
    for name in ("sdfgpu_dsh_cast_rays_device", "sdfgpu_dsh_cast_rays", "sdfgpu_dsh_cast_segments_device", "sdfgpu_dsh_cast_segments"):
        assert name in capi.EXPORTS and hasattr(capi.load_library(), name) and ("int %s(" % name) in hdr
    assert math.isclose(C.distance((0, 0, 0), (3, 4, 12), 0.5), 6.5)
