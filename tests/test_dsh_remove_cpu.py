"""Removal from the dynamic spatial hashed map without a GPU (include/sdfgpu.h "Removal"): the restatement
(tests/dsh_remove_restated.py) against hand-worked cases, the header's enum and the new entry points, the host-side arithmetic of
sdf_tools_amd/csrc/sdfgpu_dsh.hpp in a stand-alone program under -fsanitize=address,undefined (tests/dsh_remove_plan_harness.cpp),
and what the class's removal methods answer on an uninitialised map (tests/dsh_remove_class_check.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import dsh_remove_restated as X
import dsh_restated as R
from sdf_tools_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, C = R.record(1.0, 7), R.record(0.0, 9), R.record(0.5, 0xDEADBEEF)
NEW = ("sdfgpu_dsh_remove_chunks_device", "sdfgpu_dsh_remove_chunks", "sdfgpu_dsh_retain_box", "sdfgpu_dsh_shrink")


def line_map(dims=(4, 4, 4), chunks=range(-3, 4)):
    """chunks (k, 0, 0): even k cell-filled (one cell set), odd k chunk-filled"""
    m = R.Map(chunk_dims=dims, default=B)
    for k in chunks:
        p = (dims[0] * k + 0.5, 0.5, 0.5)
        m.set_cell(p, A) if k % 2 == 0 else m.set_chunk(p, C)
    return m


# ---- the restatement against hand-worked cases --------------------------------------------------------------------------------------
def test_removals_go_in_list_order_and_only_the_first_of_duplicates_removes():
    m = line_map()
    m.components_valid = True                                             # (nothing sets it; a removal must clear it)
    far = float(1 << 20) * 4
    loc = [(0.5, 0.5, 0.5), (3.5, 3.5, 3.5), (np.nan, 0, 0), (100.5, 0.5, 0.5), (far, 0, 0), (-0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (-3.5, 1, 1), (0, np.inf, 0)]
    st = X.remove_chunks(m, loc)
    # chunk 0 | the same chunk by another cell | invalid | absent | out of range | chunk -1 | chunk 0 again | chunk -1 again | invalid
    assert st.tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0]
    assert sorted(c[0] for c in m.chunks) == [-3, -2, 1, 2, 3] and not m.components_valid
    assert m.get((0.5, 0.5, 0.5)) == (B, R.NOT_FOUND) and m.get((-0.5, 0.5, 0.5)) == (B, R.NOT_FOUND)
    assert m.get((4.5, 0.5, 0.5)) == (C, R.FOUND_IN_CHUNK) and m.get((8.5, 0.5, 0.5)) == (A, R.FOUND_IN_CELL)
    # a later SetCell makes a fresh cell-filled chunk: the other cells are the default, not what the chunk held
    assert m.set_cell((1.5, 0.5, 0.5), C) == R.SET_CELL
    assert m.get((1.5, 0.5, 0.5)) == (C, R.FOUND_IN_CELL) and m.get((0.5, 0.5, 0.5)) == (B, R.FOUND_IN_CELL)
    m.components_valid = True
    assert X.remove_chunks(m, [(100.5, 0.5, 0.5), (np.nan, 0, 0)]).tolist() == [0, 0] and m.components_valid    # nothing removed: nothing changes
    assert X.remove_chunks(m, np.zeros((0, 3))).tolist() == []


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_box_that_cuts_a_chunk_by_one_cell_on_each_side_of_each_face(axis):
    n = (3, 2, 5)

    def scene():
        m = R.Map(chunk_dims=n, default=B)
        for k in (-2, -1, 0, 1, 2):
            c = [0, 0, 0]
            c[axis] = k
            m.set_chunk(tuple((c[a] + 0.5) * n[a] for a in range(3)), A)
        return m

    def kept(lower_a, extent_a, invert=False):
        m = scene()
        lower, extent = [0, 0, 0], list(n)
        lower[axis], extent[axis] = lower_a, extent_a
        removed = X.retain_box(m, lower, extent, invert)
        assert removed == 5 - len(m.chunks)
        return sorted(c[axis] for c in m.chunks)
    s = n[axis]
    assert kept(0, s) == [0]                                              # exactly chunk 0's cells
    assert kept(-1, s + 1) == [-1, 0] and kept(0, s + 1) == [0, 1] and kept(-1, s + 2) == [-1, 0, 1]     # one cell past each face
    assert kept(1, s - 1) == [0] if s > 1 else True                       # one cell inside the lower face: the chunk stays whole
    assert kept(s - 1, 1) == [0] and kept(s, 1) == [1] and kept(-1, 1) == [-1]                           # single cells beside the faces
    assert kept(-s, s) == [-1] and kept(-s - 1, 2) == [-2, -1]            # negative coordinates: floor, not truncation
    assert kept(-2 * s, 5 * s) == [-2, -1, 0, 1, 2] and kept(3 * s, s) == []
    assert kept(0, s, invert=True) == [-2, -1, 1, 2] and kept(-1, 2, invert=True) == [-2, 1, 2]


def test_a_box_must_hold_a_cell_on_every_axis():
    m = line_map(chunks=[0])
    assert X.retain_box(m, (0, 4, 0), (4, 4, 4), invert=True) == 0 and X.retain_box(m, (0, 0, -4), (4, 4, 4), invert=True) == 0
    assert X.retain_box(m, (3, 3, 3), (1, 1, 1), invert=True) == 1 and not m.chunks


def test_the_empty_box_both_ways():
    for extent in [(0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)]:
        m = line_map()
        assert X.retain_box(m, (0, 0, 0), extent, invert=True) == 0 and len(m.chunks) == 7     # removes nothing
        assert X.retain_box(m, (0, 0, 0), extent) == 7 and not m.chunks                       # clears the map
        assert X.retain_box(m, (0, 0, 0), extent) == 0


def test_the_refusal_bounds_at_two_to_the_forty():
    big = 1 << 40
    m = line_map()
    for a in range(3):
        for lower_a, extent_a, ok in [(big, 1, True), (-big, 1, True), (big + 1, 1, False), (-big - 1, 1, False), (0, big, True), (0, big + 1, False),
                                      (0, -1, False), (-big, big, True)]:
            lower, extent = [0, 0, 0], [4, 4, 4]
            lower[a], extent[a] = lower_a, extent_a
            assert X.box_ok(lower, extent) == ok
            if not ok:
                with pytest.raises(X.Refused):
                    X.retain_box(m, lower, extent, invert=True)
                assert len(m.chunks) == 7                                 # refused: nothing written
    # a box far beyond the key range holds no chunk of the map
    assert X.retain_box(m, (big - 8, 0, 0), (8, 4, 4), invert=True) == 0
    assert X.retain_box(m, (-big, -big, -big), (big, big, big), invert=True) == 0    # (every chunk of the map has y and z cells 0 .. 3)
    assert X.retain_box(m, (-big, 0, 0), (big, 1, 1), invert=True) == 3 and sorted(c[0] for c in m.chunks) == [0, 1, 2, 3]


def test_the_shrink_plan():
    assert X.shrink_plan(100, 0, 8192, 16384, 30) == (100, 256, 256 * 12 + 100 * (24 + 240))
    assert X.shrink_plan(100, 10, 8192, 16384, 30)[:2] == (110, 256) and X.shrink_plan(100, 29, 8192, 16384, 30)[:2] == (129, 512)
    assert X.shrink_plan(0, 0, 64, 128, 1)[:2] == (1, 16)
    assert X.shrink_plan(100, 1000, 200, 256, 1)[:2] == (200, 256)         # an allocation is replaced only where the new size is smaller


# ---- the header and the library ------------------------------------------------------------------------------------------------------
def test_the_enum_and_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "sdfgpu.h")).read()
    found = re.search(r"enum \{ SDFGPU_DSH_CHUNK_NOT_REMOVED = (\d+), SDFGPU_DSH_CHUNK_REMOVED = (\d+) \};", hdr)
    assert found and (int(found.group(1)), int(found.group(2))) == (0, 1)
    assert not re.search(r"#define SDFGPU_DSH_CHUNK", hdr)
    assert (capi.DSH_CHUNK_NOT_REMOVED, capi.DSH_CHUNK_REMOVED) == (X.CHUNK_NOT_REMOVED, X.CHUNK_REMOVED) == (0, 1)
    lib = capi.load_library()
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(lib, name) and re.search(r"\b%s\(" % name, hdr), name
    for method in ("remove_chunks", "remove_chunks_device", "retain_box", "remove_box", "clear", "shrink"):
        assert callable(getattr(capi.DshMap, method))
    assert capi.DSH_COUNTS_DTYPE.itemsize == 56                           # removal added no field to sdfgpu_dsh_counts


# ---- the host arithmetic under the sanitizers --------------------------------------------------------------------------------------------
def test_box_ranges_pairing_and_shrink_sizes_under_asan_and_ubsan():
    tests = os.path.join(ROOT, "tests")
    exe = os.path.join(tests, "dsh_remove_plan_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(tests, "dsh_remove_plan_harness.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "dsh remove plan OK" in r.stdout, r.stdout + r.stderr


# ---- the C++ class without a GPU ---------------------------------------------------------------------------------------------------------
def test_the_removal_methods_of_the_class_on_an_uninitialised_map():
    """tests/dsh_remove_class_check.cpp: the additions' signatures are static_asserts, and a default-constructed map answers without a GPU"""
    tests = os.path.join(ROOT, "tests")
    exe = os.path.join(tests, "dsh_remove_class_check")
    pkg = os.path.join(ROOT, "sdf_tools_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", "-DSDF_TOOLS_VECTOR_ADOPT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(tests, "dsh_remove_class_check.cpp"), "-o", exe, "-L", pkg, "-lsdfgpu", "-Wl,-rpath," + pkg, "-lz"])
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dsh remove class OK" in r.stdout, r.stdout + r.stderr
