"""Frontier cells without a GPU (include/sdfgpu.h "Frontier cells" and "Component statistics"): the restatement
(tests/dsh_frontier_restated.py) against hand-worked cases, against an independent route (a numpy shifted-array stencil over
Map.window of the box grown by one cell), the pinned numbers of one carved frame, the list order, the statistics against
numpy.bincount, the header's layout and names, and what the class's frontier methods answer on an uninitialised map
(tests/dsh_frontier_class_check.cpp), and the host-side box and stencil arithmetic of sdf_tools_amd/csrc/sdfgpu_dsh.hpp in a stand-alone
program under -fsanitize=address,undefined (tests/dsh_frontier_plan_harness.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import dsh_frontier_restated as F
import dsh_rays_restated as RR
import dsh_restated as R
from sdf_tools_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREE, FILLED, UNKNOWN = R.record(0.0, 1), R.record(1.0, 2), R.record(0.5, 3)
BELOW, ABOVE = R.record_bits(0x3EFFFFFF, 4), R.record_bits(0x3F000001, 5)     # the two float neighbours of 0.5f
NAN_CELL = R.record_bits(0x7FC00001, 6)
BOTH_RULES = (0, F.FRONTIER_26)


def cells_of(a):
    return [tuple(int(v) for v in row) for row in a]


# ---- hand-worked cases ---------------------------------------------------------------------------------------------------------------------
def test_a_single_free_cell_under_each_default():
    for default, want in ((R.record(0.5, 9), [(5, 6, 7)]), (R.record(0.0, 9), []), (R.record(1.0, 9), [])):
        m = R.Map(chunk_dims=(4, 4, 4), default=default)
        RR.set_cell_index(m, (5, 6, 7), FREE)
        for flags in BOTH_RULES:
            got = cells_of(F.frontier_cells(m, None, flags))
            if default == R.record(0.0, 9):
                # every cell of the chunk is free now, and nothing anywhere is unknown
                assert got == []
            elif default == R.record(1.0, 9):
                assert got == [], "a filled default is not unknown"
            else:
                assert got == want, "its 63 chunk mates are unknown, and so are not free"
    # default 0.5: the cell's six neighbours are all unknown cells of its own chunk
    m = R.Map(chunk_dims=(4, 4, 4), default=R.record(0.5))
    RR.set_cell_index(m, (5, 6, 6), FREE)
    assert F.deciding_kinds(m, (5, 6, 6)) == {"same"}


def test_exactly_half_and_its_two_float_neighbours():
    assert F.is_unknown(UNKNOWN) and not F.is_free(UNKNOWN)
    assert F.is_free(BELOW) and not F.is_unknown(BELOW)
    assert not F.is_free(ABOVE) and not F.is_unknown(ABOVE)
    for centre, beside, want in ((BELOW, UNKNOWN, True), (UNKNOWN, UNKNOWN, False), (ABOVE, UNKNOWN, False), (FREE, BELOW, False), (FREE, ABOVE, False),
                                 (FREE, UNKNOWN, True)):
        m = R.Map(chunk_dims=(3, 2, 5), default=FILLED)
        RR.set_cell_index(m, (1, 1, 1), centre)
        RR.set_cell_index(m, (1, 1, 2), beside)
        assert F.is_frontier(m, (1, 1, 1)) == want, (hex(centre), hex(beside))


def test_nan_zeros_and_infinities():
    values = {"nan": NAN_CELL, "nan-": R.record_bits(0xFFC12345), "+0": R.record(0.0), "-0": R.record(-0.0), "+inf": R.record(np.inf), "-inf": R.record(-np.inf)}
    free = {"+0", "-0", "-inf"}
    for name, v in values.items():
        assert F.is_free(v) == (name in free) and not F.is_unknown(v), name
        m = R.Map(chunk_dims=(2, 2, 2), default=FILLED)
        RR.set_cell_index(m, (0, 0, 0), v)
        RR.set_cell_index(m, (0, 0, 1), UNKNOWN)
        assert F.is_frontier(m, (0, 0, 0)) == (name in free), name
        m = R.Map(chunk_dims=(2, 2, 2), default=FILLED)                        # ... and as the neighbour: none of them is unknown
        RR.set_cell_index(m, (0, 0, 0), FREE)
        RR.set_cell_index(m, (0, 0, 1), v)
        assert not F.is_frontier(m, (0, 0, 0)), name


def test_a_free_chunk_filled_chunk_beside_an_absent_chunk():
    m = R.Map(chunk_dims=(3, 2, 5), default=UNKNOWN)
    m.set_chunk((0.5, 0.5, 0.5), FREE)                                          # chunk (0, 0, 0), chunk-filled
    for c in [(-1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]:        # free chunks on every side but +x
        m.set_chunk(tuple((np.array(c) + 0.5) * np.array(m.n)), FREE)
    got = cells_of(F.frontier_cells(m, ((0, 0, 0), m.n), 0))
    assert got == [(2, y, z) for y in range(2) for z in range(5)], "the whole +x face, in cell slot order"
    assert all(F.deciding_kinds(m, i) == {"absent"} for i in got)
    # under 26 the twelve chunks across its edges and the eight across its corners are absent too: a cell sees one of them wherever it
    # can cross two faces at once, and every cell can cross a y face (n_y = 2)
    want_26 = [(x, y, z) for x in range(3) for y in range(2) for z in range(5) if x in (0, 2) or z in (0, 4)]
    assert cells_of(F.frontier_cells(m, ((0, 0, 0), m.n), F.FRONTIER_26)) == want_26 and len(want_26) == 24


def test_a_free_cell_of_an_absent_chunk_is_never_a_frontier_cell():
    m = R.Map(chunk_dims=(4, 4, 4), default=FREE)
    RR.set_cell_index(m, (4, 0, 0), UNKNOWN)                                    # chunk (1, 0, 0) is live, chunk (0, 0, 0) absent
    assert m.get_cell((3, 0, 0)) == (FREE, R.NOT_FOUND)
    assert not F.is_frontier(m, (3, 0, 0)), "free by the default, beside an unknown live cell, but its chunk is absent"
    assert F.is_frontier(m, (5, 0, 0)) and F.is_frontier(m, (4, 1, 0))
    assert sorted(cells_of(F.frontier_cells(m, None, 0))) == [(4, 0, 1), (4, 1, 0), (5, 0, 0)]
    want_26 = sorted((x, y, z) for x in (4, 5) for y in (0, 1) for z in (0, 1) if (x, y, z) != (4, 0, 0))
    assert sorted(cells_of(F.frontier_cells(m, None, F.FRONTIER_26))) == want_26


def test_a_cell_whose_only_unknown_neighbour_is_diagonal():
    m = R.Map(chunk_dims=(4, 4, 4), default=FILLED)
    RR.set_cell_index(m, (3, 3, 3), FREE)
    RR.set_cell_index(m, (4, 4, 4), UNKNOWN)                                    # across a chunk corner
    RR.set_cell_index(m, (1, 1, 1), FREE)
    RR.set_cell_index(m, (2, 2, 1), UNKNOWN)                                    # across an edge, inside the chunk
    assert cells_of(F.frontier_cells(m, None, 0)) == []
    assert cells_of(F.frontier_cells(m, None, F.FRONTIER_26)) == [(1, 1, 1), (3, 3, 3)]
    assert F.deciding_kinds(m, (3, 3, 3), F.FRONTIER_26) == {"live"} and F.deciding_kinds(m, (1, 1, 1), F.FRONTIER_26) == {"same"}


def test_chunks_at_the_ends_of_the_key_range_read_the_default_beyond_them():
    n = (3, 2, 5)
    for c, step in ((-R.CHUNK_BIAS, -1), (R.CHUNK_BIAS - 1, 1)):
        m = R.Map(chunk_dims=n, default=UNKNOWN)
        m.chunks[(c, c, c)] = ("chunk", FREE)
        corner = tuple(c * n[a] + (0 if step < 0 else n[a] - 1) for a in range(3))
        assert m.get_cell(tuple(v + step for v in corner)) == (UNKNOWN, R.NOT_FOUND)
        assert F.deciding_kinds(m, corner) == {"absent"}
        assert len(F.frontier_cells(m, None, 0)) == 30, "n_y = 2: every cell of the chunk lies on one of its faces"


# ---- an independent route: a shifted-array stencil over the window grown by one cell ------------------------------------------------------------
def random_map(rng, dims, default, half):
    m = R.Map(chunk_dims=dims, default=default)
    n = np.array(dims)
    lo, hi = np.floor(-half / n).astype(int), np.floor(half / n).astype(int)
    kinds = [FREE, FREE, FREE, UNKNOWN, FILLED]
    for c in np.stack(np.meshgrid(*[np.arange(l, h + 1) for l, h in zip(lo, hi)], indexing="ij"), -1).reshape(-1, 3):
        k = rng.random()
        if k < 0.45:
            m.chunks[tuple(int(v) for v in c)] = ("chunk", kinds[int(rng.integers(len(kinds)))])
    values = [FREE, FREE, UNKNOWN, FILLED, NAN_CELL, BELOW, ABOVE, FREE]
    for i in rng.integers(-half, half, (int(np.prod(hi - lo + 1)) * 3 + 10, 3)):
        RR.set_cell_index(m, tuple(int(v) for v in i), values[int(rng.integers(len(values)))])
    return m


def stencil(m, lower, shape, flags):
    """bool [shape]: the frontier cells of the window by whole-array operations"""
    grown = m.window([v - 1 for v in lower], [s + 2 for s in shape])
    occ = R.occupancy(grown.reshape(-1)).reshape(grown.shape)
    unknown = occ == np.float32(0.5)
    free = occ < np.float32(0.5)
    live = np.zeros(shape, bool)
    for x in range(shape[0]):
        for y in range(shape[1]):
            for z in range(shape[2]):
                c = m.split((lower[0] + x, lower[1] + y, lower[2] + z))[0]
                live[x, y, z] = all(R.chunk_in_range(v) for v in c) and c in m.chunks
    near = np.zeros(shape, bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                steps = (dx != 0) + (dy != 0) + (dz != 0)
                if steps == 0 or (not flags and steps != 1):
                    continue
                near |= unknown[1 + dx:1 + dx + shape[0], 1 + dy:1 + dy + shape[1], 1 + dz:1 + dz + shape[2]]
    return live & free[1:-1, 1:-1, 1:-1] & near


@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 2, 5), (4, 4, 4)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("default", [UNKNOWN, FREE, FILLED], ids=["unknown", "free", "filled"])
def test_the_restatement_against_a_shifted_array_stencil(dims, default):
    rng = np.random.default_rng(340 + sum(dims))
    half = 4 if dims == (1, 1, 1) else 8
    m = random_map(rng, dims, default, half)
    lower, shape = (-half - 1, -half, -half + 1), (2 * half + 2, 2 * half, 2 * half - 1)
    total = 0
    for flags in BOTH_RULES:
        want = stencil(m, lower, shape, flags)
        got = F.frontier_window(m, lower, shape, flags)
        assert np.array_equal(got, want)
        assert np.array_equal(F.frontier_window_bits(m, lower, shape, flags), R.pack_bits(want))
        listed = F.frontier_cells(m, (lower, shape), flags)
        assert sorted(cells_of(listed)) == sorted(cells_of(np.argwhere(want) + np.array(lower))), "the list holds the window's set bits"
        total += len(listed)
    if default != FILLED or dims != (1, 1, 1):
        assert total > 0


# ---- one carved frame: the pinned numbers ---------------------------------------------------------------------------------------------------
def carved_frame():
    m = R.Map(chunk_dims=(4, 4, 4), default=R.record(0.5))
    wall = np.array([(CARVED_SENSOR[0] + 12.0, y + 0.5, z + 0.5) for y in range(CARVED_LOW, CARVED_LOW + 11) for z in range(CARVED_LOW, CARVED_LOW + 11)], np.float32)
    assert len(wall) == 121
    RR.insert_rays(m, np.array(CARVED_SENSOR), wall, 100.0, R.record(0.0), R.record(1.0))
    return m


def pieces(cells):
    """face-connected pieces of a set of cells"""
    left, count = set(cells), 0
    while left:
        stack = [left.pop()]
        count += 1
        while stack:
            i = stack.pop()
            for d in F.OFFSETS_6:
                j = (i[0] + d[0], i[1] + d[1], i[2] + d[2])
                if j in left:
                    left.remove(j)
                    stack.append(j)
    return count


CARVED_LOW, CARVED_SENSOR = 2, (2.5, 7.5, 7.5)


def test_one_carved_frame_gives_the_pinned_numbers():
    m = carved_frame()
    six, all_26 = cells_of(F.frontier_cells(m, None, 0)), cells_of(F.frontier_cells(m, None, F.FRONTIER_26))
    assert (len(six), len(all_26)) == (241, 322) and set(six) <= set(all_26)
    only_absent = [i for i in six if F.deciding_kinds(m, i) == {"absent"}]
    assert len(only_absent) == CARVED_ONLY_ABSENT
    assert (pieces(six), pieces(all_26)) == CARVED_PIECES


CARVED_ONLY_ABSENT, CARVED_PIECES = 15, (6, 1)


# ---- list order -----------------------------------------------------------------------------------------------------------------------------
def test_the_list_is_in_chunk_then_cell_slot_order():
    rng = np.random.default_rng(341)
    m = random_map(rng, (3, 2, 5), UNKNOWN, 9)
    for flags in BOTH_RULES:
        listed = cells_of(F.frontier_cells(m, None, flags))
        assert len(listed) > 100

        def key(i):
            c, l = m.split(i)
            return (c, (l[0] * m.n[1] + l[1]) * m.n[2] + l[2])
        assert listed == sorted(listed, key=key) and len(set(listed)) == len(listed)
        assert listed != sorted(listed), "the order is by chunk first: it is not the order of the global cell"
        # a box lists the same cells, in the same order, minus those outside
        box = ((-4, -3, -2), (9, 7, 8))
        inside = [i for i in listed if all(box[0][a] <= i[a] < box[0][a] + box[1][a] for a in range(3))]
        assert cells_of(F.frontier_cells(m, box, flags)) == inside and 0 < len(inside) < len(listed)
    assert len(F.frontier_cells(m, ((100, 100, 100), (5, 5, 5)), 0)) == 0, "a box without a live chunk"


# ---- statistics -------------------------------------------------------------------------------------------------------------------------------
def test_component_stats_against_bincount():
    rng = np.random.default_rng(342)
    shape = (5, 3, 33)
    bits = rng.random(shape) < 0.4
    labels = rng.integers(1, 20, shape).astype(np.uint32)                      # (any labelling: the statistics do not ask where it came from)
    got = F.component_stats(bits, labels, shape, 19)
    x, y, z = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    lab = labels[bits]
    count = np.bincount(lab, minlength=20)
    assert [s["label"] for s in got] == [k for k in range(1, 20) if count[k]]
    for s in got:
        k = s["label"]
        assert s["count"] == count[k]
        for a, coord in enumerate((x, y, z)):
            assert s["sum"][a] == np.bincount(lab, weights=coord[bits], minlength=20)[k]
            assert s["lo"][a] == coord[bits][lab == k].min() and s["hi"][a] == coord[bits][lab == k].max()
    assert [s["label"] for s in F.component_stats(bits, labels, shape, 7)] == [k for k in range(1, 8) if count[k]], "labels above label_count are left out"
    rec = F.component_stats_records(got, capi.COMPONENT_STATS_DTYPE)
    assert rec.dtype.itemsize == 64 and not rec["reserved"].any() and np.array_equal(rec["count"], count[1:][count[1:] > 0])
    assert F.component_stats(np.zeros(shape, bool), labels, shape) == []


# ---- the header and the library -------------------------------------------------------------------------------------------------------------
def test_header_layout_enum_values_and_exports(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sdfgpu.h")).read()
    assert "SDFGPU_DSH_FRONTIER_26 = 1" in hdr and "Frontier cells" in hdr
    assert capi.DSH_FRONTIER_26 == F.FRONTIER_26 == 1
    names = capi.COMPONENT_STATS_DTYPE.names
    assert names == ("label", "reserved", "count", "sum", "lo", "hi")
    body = 'printf("size %zu\\n", sizeof(sdfgpu_component_stats));\n' + "".join('printf("%s %%zu\\n", offsetof(sdfgpu_component_stats, %s));\n' % (f, f) for f in names)
    body += 'printf("flag %d\\n", SDFGPU_DSH_FRONTIER_26);\n'
    src, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "sdfgpu.h"\nint main(void) {\n%sreturn 0;\n}\n' % body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = dict(line.split(None, 1) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == capi.COMPONENT_STATS_DTYPE.itemsize == 64 and got["flag"] == "1"
    assert [int(got[f]) for f in names] == [capi.COMPONENT_STATS_DTYPE.fields[f][1] for f in names] == [0, 4, 8, 16, 40, 52]
    for name in ("sdfgpu_dsh_frontier_window_device", "sdfgpu_dsh_frontier_window", "sdfgpu_dsh_frontier_cells_device", "sdfgpu_dsh_frontier_cells",
                 "sdfgpu_component_stats_device"):
        assert name in capi.EXPORTS and hasattr(capi.load_library(), name) and ("int %s(" % name) in hdr


# ---- the C++ class without a GPU ---------------------------------------------------------------------------------------------------------
def test_the_frontier_methods_of_the_class_on_an_uninitialised_map(tmp_path):
    """tests/dsh_frontier_class_check.cpp: the additions' signatures are static_asserts, and a default-constructed map answers without a GPU"""
    tests = os.path.join(ROOT, "tests")
    exe = str(tmp_path / "dsh_frontier_class_check")
    pkg = os.path.join(ROOT, "sdf_tools_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", "-DSDF_TOOLS_VECTOR_ADOPT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(tests, "dsh_frontier_class_check.cpp"), "-o", exe, "-L", pkg, "-lsdfgpu", "-Wl,-rpath," + pkg, "-lz"])
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dsh frontier class OK" in r.stdout, r.stdout + r.stderr


# ---- the host arithmetic under the sanitizers --------------------------------------------------------------------------------------------
def test_boxes_and_stencil_steps_under_asan_and_ubsan(tmp_path):
    tests = os.path.join(ROOT, "tests")
    exe = str(tmp_path / "dsh_frontier_plan_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(tests, "dsh_frontier_plan_harness.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "dsh frontier plan OK" in r.stdout, r.stdout + r.stderr
