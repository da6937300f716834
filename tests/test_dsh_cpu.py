"""The dynamic spatial hashed map without a GPU: the restatement (tests/dsh_restated.py) against hand-worked cases, the key packing at
the +-2^20 edges, the layout of the header's structs and constants, and the host-side arithmetic of sdf_tools_amd/csrc/sdfgpu_dsh.hpp
in a stand-alone program under -fsanitize=address,undefined (tests/dsh_plan_harness.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import dsh_restated as R
from sdf_tools_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, C = R.record(1.0, 7), R.record(0.0, 9), R.record(0.5, 0xDEADBEEF)


# ---- the restatement against hand-worked cases --------------------------------------------------------------------------------------
def test_floor_not_truncation_at_negative_coordinates():
    m = R.Map(cell_size=0.25, chunk_dims=(4, 4, 4))
    assert m.global_cell((0.0, 0.0, 0.0)) == (0, 0, 0)
    assert m.global_cell((-0.0, 0.24, 0.25)) == (0, 0, 1)
    assert m.global_cell((-0.01, -0.25, -0.26)) == (-1, -1, -2)          # truncation would give (0, -1, -1)
    assert m.global_cell((-1.0, -1.01, 0.99)) == (-4, -5, 3)
    assert m.split((-1, -4, -5)) == ((-1, -1, -2), (3, 0, 3))
    assert m.split((0, 3, 4)) == ((0, 0, 1), (0, 3, 0))


def test_floor_div_at_minus_one_and_at_multiples():
    for n in (1, 3, 16):
        assert R.floor_div(-1, n) == -1
        assert R.floor_div(-n, n) == -1 and R.floor_div(-n - 1, n) == -2 and R.floor_div(n - 1, n) == 0 and R.floor_div(n, n) == 1
        for i in range(-3 * n, 3 * n + 1):
            assert R.floor_div(i, n) == i // n


def test_the_origin_is_applied_as_its_inverse_with_the_stated_order():
    inv = np.eye(4)
    inv[:3, 3] = (-1.0, 2.0, 0.5)                                         # origin translated by (1, -2, -0.5): whole cells of 0.5
    m = R.Map(inverse_origin=inv, cell_size=0.5, chunk_dims=(3, 2, 5))
    assert m.global_cell((1.0, -2.0, -0.5)) == (0, 0, 0)
    assert m.global_cell((0.75, -2.0, 2.0)) == (-1, 0, 5)
    assert m.split((-1, 0, 5)) == ((-1, 0, 1), (2, 0, 0))


def test_the_three_state_changes():
    m = R.Map(chunk_dims=(2, 2, 2), default=B)
    p, q = (0.5, 0.5, 0.5), (1.5, 0.5, 0.5)                               # two cells of chunk (0, 0, 0)
    assert m.get(p) == (B, R.NOT_FOUND) and m.counts() == (0, 0)
    # absent -> cell-filled: every other cell is the default
    assert m.set_cell(p, A) == R.SET_CELL and m.get(p) == (A, R.FOUND_IN_CELL) and m.get(q) == (B, R.FOUND_IN_CELL)
    assert m.counts() == (0, 1) and not m.components_valid
    # cell-filled -> chunk-filled: the cells are dropped
    assert m.set_chunk(q, C) == R.SET_CHUNK and m.get(p) == (C, R.FOUND_IN_CHUNK) and m.counts() == (1, 0)
    # chunk-filled -> cell-filled: the other cells keep the chunk's record
    assert m.set_cell(p, A) == R.SET_CELL and m.get(p) == (A, R.FOUND_IN_CELL) and m.get(q) == (C, R.FOUND_IN_CELL)
    assert m.get((2.5, 0.5, 0.5)) == (B, R.NOT_FOUND)
    chunks, cells = m.export()
    assert chunks == [((0, 0, 0), R.FOUND_IN_CELL, 0, 0)] and cells.shape == (1, 2, 2, 2)
    assert int(cells[0, 0, 0, 0]) == A and int((cells == np.uint64(C)).sum()) == 7


def test_invalid_locations_change_nothing_and_batches_go_in_list_order():
    m = R.Map(chunk_dims=(1, 1, 1), default=B)
    far = float(1 << 20)
    loc = [(0.5, 0.5, 0.5), (np.nan, 0, 0), (0.5, 0.5, 0.5), (0, np.inf, 0), (far, 0, 0), (-far - 0.5, 0, 0), (-far, 0, 0), (0.5, 0.5, 0.5)]
    st = m.set_cells(loc, [1, 2, 3, 4, 5, 6, 7, 8])
    assert st.tolist() == [2, 0, 2, 0, 0, 0, 2, 2]
    assert m.get((0.5, 0.5, 0.5)) == (8, R.FOUND_IN_CELL) and m.get((-far, 0, 0)) == (7, R.FOUND_IN_CELL)
    assert m.get((far, 0, 0)) == (B, R.NOT_FOUND) and len(m.chunks) == 2
    assert m.set_chunks([(0.5, 0.5, 0.5), (0.5, 0.5, 0.5)], [11, 12]).tolist() == [1, 1] and m.get((0.5, 0.5, 0.5)) == (12, R.FOUND_IN_CHUNK)


def test_window_and_bits_of_the_restatement():
    m = R.Map(chunk_dims=(2, 2, 2), default=B)
    m.set_chunk((-1.0, -1.0, -1.0), A)
    m.set_cell((0.5, 0.5, 0.5), C)
    w = m.window((-1, -1, -1), (3, 2, 2))
    assert int(w[0, 0, 0]) == A and int(w[1, 1, 1]) == C and int(w[2, 1, 1]) == B and int(w[1, 0, 1]) == B
    assert R.classify(w, False).sum() == 1 and R.classify(w, True).sum() == 2
    assert R.pack_bits(R.classify(w, True)).tolist() == [1 | 1 << 7]


# ---- keys -----------------------------------------------------------------------------------------------------------------------------------
def test_key_packing_round_trips_at_the_edges():
    lo, hi = -R.CHUNK_BIAS, R.CHUNK_BIAS - 1
    edge = [lo, lo + 1, -1, 0, 1, hi - 1, hi]
    keys = []
    for x in edge:
        for y in edge:
            for z in edge:
                k = R.pack_key((x, y, z))
                assert 0 <= k < (1 << 63) and k != R.EMPTY_KEY and R.unpack_key(k) == (x, y, z)
                keys.append(k)
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert R.pack_key((hi, hi, hi)) == (1 << 63) - 1 and R.pack_key((lo, lo, lo)) == 0
    assert not R.chunk_in_range(lo - 1) and not R.chunk_in_range(hi + 1)
    with pytest.raises(AssertionError):
        R.pack_key((hi + 1, 0, 0))


# ---- the header ------------------------------------------------------------------------------------------------------------------------
def test_header_constants_and_struct_layouts():
    hdr = open(os.path.join(ROOT, "include", "sdfgpu.h")).read()
    consts = dict(re.findall(r"#define (SDFGPU_DSH_\w+) (\d+)", hdr))
    assert {k: int(v) for k, v in consts.items()} == {
        "SDFGPU_DSH_NOT_FOUND": 0, "SDFGPU_DSH_FOUND_IN_CHUNK": 1, "SDFGPU_DSH_FOUND_IN_CELL": 2, "SDFGPU_DSH_NOT_SET": 0,
        "SDFGPU_DSH_SET_CHUNK": 1, "SDFGPU_DSH_SET_CELL": 2, "SDFGPU_DSH_MAX_CHUNK_CELLS": 32768}
    assert (capi.DSH_NOT_FOUND, capi.DSH_FOUND_IN_CHUNK, capi.DSH_FOUND_IN_CELL) == (R.NOT_FOUND, R.FOUND_IN_CHUNK, R.FOUND_IN_CELL) == (0, 1, 2)
    assert (capi.DSH_NOT_SET, capi.DSH_SET_CHUNK, capi.DSH_SET_CELL) == (R.NOT_SET, R.SET_CHUNK, R.SET_CELL) == (0, 1, 2)
    assert capi.DSH_MAX_CHUNK_CELLS == R.MAX_CHUNK_CELLS == 32768
    # the two structs, compiled: sizes and offsets as the numpy records of capi state them
    src = os.path.join(ROOT, "tests", "dsh_layout_probe.c")
    exe = os.path.join(ROOT, "tests", "dsh_layout_probe")
    fields = {"sdfgpu_dsh_counts": capi.DSH_COUNTS_DTYPE, "sdfgpu_dsh_chunk": capi.DSH_CHUNK_DTYPE}
    body = "".join('printf("%s %%zu\\n", sizeof(%s));\n' % (s, s) + "".join('printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (s, f, s, f) for f in d.names)
                   for s, d in fields.items())
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "sdfgpu.h"\nint main(void) {\n%sreturn 0;\n}\n' % body)
    try:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    finally:
        for p in (src, exe):
            if os.path.exists(p):
                os.remove(p)
    assert int(got["sdfgpu_dsh_counts"]) == capi.DSH_COUNTS_DTYPE.itemsize == 56 and int(got["sdfgpu_dsh_chunk"]) == capi.DSH_CHUNK_DTYPE.itemsize == 48
    for s, d in fields.items():
        for f in d.names:
            assert int(got["%s.%s" % (s, f)]) == d.fields[f][1], (s, f)
    assert capi.dsh_record(1.0, 7) == A == 0x3F800000 | 7 << 32
    for name in ("sdfgpu_dsh_create", "sdfgpu_dsh_destroy", "sdfgpu_dsh_info", "sdfgpu_dsh_set_cells_device", "sdfgpu_dsh_set_cells",
                 "sdfgpu_dsh_set_chunks_device", "sdfgpu_dsh_set_chunks", "sdfgpu_dsh_insert_points_device", "sdfgpu_dsh_get_device", "sdfgpu_dsh_get",
                 "sdfgpu_dsh_extract_window_device", "sdfgpu_dsh_extract_window", "sdfgpu_dsh_export_device", "sdfgpu_dsh_export"):
        assert name in capi.EXPORTS and hasattr(capi.load_library(), name)


# ---- the host arithmetic under the sanitizers --------------------------------------------------------------------------------------------
def test_key_packing_capacity_planning_and_growth_arithmetic_under_asan_and_ubsan():
    tests = os.path.join(ROOT, "tests")
    exe = os.path.join(tests, "dsh_plan_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(tests, "dsh_plan_harness.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "dsh plan OK" in r.stdout, r.stdout + r.stderr


# ---- the C++ class without a GPU ---------------------------------------------------------------------------------------------------------
def test_the_class_signatures_and_an_uninitialised_map():
    """tests/dsh_class_check.cpp: the reference's signatures are static_asserts, and a default-constructed map answers without a GPU"""
    tests = os.path.join(ROOT, "tests")
    exe = os.path.join(tests, "dsh_class_check")
    pkg = os.path.join(ROOT, "sdf_tools_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", "-DSDF_TOOLS_VECTOR_ADOPT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(tests, "dsh_class_check.cpp"), "-o", exe, "-L", pkg, "-lsdfgpu", "-Wl,-rpath," + pkg, "-lz"])
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dsh class OK" in r.stdout, r.stdout + r.stderr
