"""The connected components of the sparse map without a GPU: the restatement
(tests/dsh_components_restated.py) against hand-worked cases, the header's declarations, and the host arithmetic of
sdf_tools_amd/csrc/sdfgpu_dsh.hpp as a stand-alone program under -fsanitize=address,undefined
(tests/dsh_components_plan_harness.cpp)."""
import os
import subprocess

import numpy as np

import dsh_components_restated as C
import dsh_restated as R
from sdf_tools_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLED, FREE, UNKNOWN = R.record(1.0), R.record(0.0), R.record(0.5)
NAN = R.record_bits(0x7FC00000)


def centre(i):
    return [v + 0.5 for v in i]


def block(m, c, fill, others=()):
    """chunk c of m as cells: `fill` everywhere but the (local cell, record) pairs of `others`"""
    base = [c[a] * m.n[a] for a in range(3)]
    for x in range(m.n[0]):
        for y in range(m.n[1]):
            for z in range(m.n[2]):
                m.set_cell(centre((base[0] + x, base[1] + y, base[2] + z)), fill)
    for l, rec in others:
        m.set_cell(centre((base[0] + l[0], base[1] + l[1], base[2] + l[2])), rec)


def labels_of(m, flags=0):
    """(K, {chunk: labels as a nested list, or the one label of a chunk-filled chunk})"""
    count, labels, (order, bases, total) = C.components(m, flags)
    assert len(labels) == total
    cpc = int(np.prod(m.n))
    out = {}
    for c in order:
        b = bases[c]
        out[c] = labels[b:b + cpc].reshape(m.n).tolist() if m.chunks[c][0] == "cells" else int(labels[b])
    return count, out


def test_two_chunks_joined_through_one_face_pair_and_a_diagonal_that_is_none():
    m = R.Map(chunk_dims=(2, 2, 2))
    block(m, (0, 0, 0), FILLED, [((1, 1, 1), FREE)])
    block(m, (1, 0, 0), FILLED, [((0, 1, 1), FREE)])                           # global cells (1, 1, 1) and (2, 1, 1): face neighbours
    count, got = labels_of(m)
    assert count == 2
    assert got[(0, 0, 0)] == [[[1, 1], [1, 1]], [[1, 1], [1, 2]]]
    assert got[(1, 0, 0)] == [[[1, 1], [1, 2]], [[1, 1], [1, 1]]]
    # the second free cell one step down in z: (1, 1, 1) and (2, 1, 0) touch along an edge only
    m = R.Map(chunk_dims=(2, 2, 2))
    block(m, (0, 0, 0), FILLED, [((1, 1, 1), FREE)])
    block(m, (1, 0, 0), FILLED, [((0, 1, 0), FREE)])
    count, got = labels_of(m)
    assert count == 3
    assert got[(0, 0, 0)] == [[[1, 1], [1, 1]], [[1, 1], [1, 2]]]
    assert got[(1, 0, 0)] == [[[1, 1], [3, 1]], [[1, 1], [1, 1]]]


def test_a_chunk_filled_chunk_bridges_two_free_regions_and_an_absent_one_does_not():
    def build(middle):
        m = R.Map(chunk_dims=(2, 2, 2))
        block(m, (0, 0, 0), FILLED, [((1, 0, 0), FREE)])
        if middle is not None:
            m.set_chunk(centre((2, 0, 0)), middle)
        block(m, (2, 0, 0), FILLED, [((0, 1, 1), FREE)])
        return m
    count, got = labels_of(build(FREE))
    assert count == 3
    assert got[(0, 0, 0)] == [[[1, 1], [1, 1]], [[2, 1], [1, 1]]] and got[(1, 0, 0)] == 2
    assert got[(2, 0, 0)] == [[[3, 3], [3, 2]], [[3, 3], [3, 3]]]
    count, got = labels_of(build(None))                                        # the middle chunk absent: nothing bridges, and nothing is a node there
    assert count == 4 and (1, 0, 0) not in got
    assert got[(0, 0, 0)] == [[[1, 1], [1, 1]], [[2, 1], [1, 1]]]
    assert got[(2, 0, 0)] == [[[3, 3], [3, 4]], [[3, 3], [3, 3]]]
    count, got = labels_of(build(FILLED))                                      # a filled bridge joins the two filled regions instead
    assert count == 3 and got[(1, 0, 0)] == 1
    assert got[(0, 0, 0)] == [[[1, 1], [1, 1]], [[2, 1], [1, 1]]]
    assert got[(2, 0, 0)] == [[[1, 1], [1, 3]], [[1, 1], [1, 1]]]
    # two free chunk-filled chunks with an absent chunk between them, whatever the default says about it
    for default in (FREE, FILLED, UNKNOWN):
        m = R.Map(chunk_dims=(2, 2, 2), default=default)
        m.set_chunk(centre((0, 0, 0)), FREE)
        m.set_chunk(centre((4, 0, 0)), FREE)
        assert labels_of(m) == (2, {(0, 0, 0): 1, (2, 0, 0): 2})
        m.set_chunk(centre((2, 0, 0)), FREE)                                   # ... and with it: two links make one component of three nodes
        assert labels_of(m) == (1, {(0, 0, 0): 1, (1, 0, 0): 1, (2, 0, 0): 1})


def test_half_and_nan_under_both_rules():
    m = R.Map(chunk_dims=(1, 1, 6))
    for z, rec in enumerate([FREE, UNKNOWN, NAN, FREE, FILLED, NAN]):
        m.set_cell(centre((0, 0, z)), rec)
    assert labels_of(m, 0) == (3, {(0, 0, 0): [[[1, 1, 1, 1, 2, 3]]]})
    assert labels_of(m, C.UNKNOWN_APART) == (5, {(0, 0, 0): [[[1, 2, 2, 3, 4, 5]]]})
    half = np.float32(0.5)
    around = [np.nextafter(half, np.float32(0)), half, np.nextafter(half, np.float32(1)), np.float32("-inf"), np.float32("inf"), -np.float32(0)]
    recs = [R.record(v) for v in around]
    assert C.classes(recs, 0).tolist() == [0, 0, 1, 0, 1, 0] and C.classes(recs, C.UNKNOWN_APART).tolist() == [0, 2, 1, 0, 1, 0]
    assert C.classes([NAN, R.record_bits(0xFFC00001)], 0).tolist() == [0, 0] and C.classes([NAN, R.record_bits(0xFFC00001)], 1).tolist() == [2, 2]
    # a chunk-filled chunk of unknown space beside known-free cells: one component, or two
    m = R.Map(chunk_dims=(1, 1, 2))
    m.set_chunk(centre((0, 0, 0)), UNKNOWN)
    m.set_cell(centre((0, 0, 2)), FREE)
    m.set_cell(centre((0, 0, 3)), FREE)
    assert labels_of(m, 0) == (1, {(0, 0, 0): 1, (0, 0, 1): [[[1, 1]]]})
    assert labels_of(m, C.UNKNOWN_APART) == (2, {(0, 0, 0): 1, (0, 0, 1): [[[2, 2]]]})


def test_numbering_follows_export_order_not_insertion_order():
    m = R.Map(chunk_dims=(1, 1, 2))
    m.set_chunk(centre((0, 0, 4)), FILLED)                                     # chunk (0, 0, 2), inserted first
    m.set_cell(centre((0, 0, -2)), FREE)                                       # chunk (0, 0, -1), inserted last: the first in export order
    m.set_cell(centre((0, 0, -1)), FILLED)
    assert list(m.chunks) == [(0, 0, 2), (0, 0, -1)]
    assert labels_of(m) == (3, {(0, 0, -1): [[[1, 2]]], (0, 0, 2): 3})
    m.set_chunk(centre((0, 0, 0)), FILLED)                                     # (0, 0, 0) joins (0, 0, -1)'s filled cell, but not (0, 0, 2)
    assert labels_of(m) == (3, {(0, 0, -1): [[[1, 2]]], (0, 0, 0): 2, (0, 0, 2): 3})
    m.set_chunk(centre((0, 0, 2)), FILLED)                                     # (0, 0, 1) closes the gap
    assert labels_of(m) == (2, {(0, 0, -1): [[[1, 2]]], (0, 0, 0): 2, (0, 0, 1): 2, (0, 0, 2): 2})


def test_apply_writes_the_component_words_and_nothing_else():
    m = R.Map(chunk_dims=(2, 1, 2))
    m.set_cell(centre((0, 0, 0)), R.record(0.25, 77))
    m.set_cell(centre((1, 0, 1)), R.record(0.75, 78))
    m.set_chunk(centre((2, 0, 0)), R.record(0.9, 79))
    before = {c: (k, np.array(w, copy=True)) for c, (k, w) in m.chunks.items()}
    assert C.apply(m, 0) == 2
    chunks, cells = m.export()
    assert [(c, s, r >> 32) for c, s, r, _ in chunks] == [((0, 0, 0), R.FOUND_IN_CELL, 0), ((1, 0, 0), R.FOUND_IN_CHUNK, 2)]
    assert (cells.reshape(-1) >> np.uint64(32)).tolist() == [1, 1, 1, 2]
    for c, (kind, what) in m.chunks.items():
        assert np.array_equal(np.asarray(what, np.uint64) & np.uint64(0xFFFFFFFF), np.asarray(before[c][1], np.uint64) & np.uint64(0xFFFFFFFF))
    assert m.get(centre((1, 0, 1))) == (R.record(0.75, 2), R.FOUND_IN_CELL) and m.get(centre((3, 0, 1))) == (R.record(0.9, 2), R.FOUND_IN_CHUNK)
    assert C.components(R.Map(), 0)[:2][0] == 0                                # an empty map: K = 0


def test_header_declarations_and_exports(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sdfgpu.h")).read()
    assert "Dynamic spatial hashed map: connected components" in hdr and "SDFGPU_DSH_COMPONENTS_UNKNOWN_APART = 1" in hdr
    assert capi.DSH_COMPONENTS_UNKNOWN_APART == C.UNKNOWN_APART == 1
    assert "int sdfgpu_dsh_update_components(sdfgpu_dsh_map map, uint32_t flags, uint32_t* out_count, void* stream);" in hdr
    assert "int sdfgpu_dsh_components_info(sdfgpu_dsh_map map, uint32_t* out_count, uint32_t* out_flags, int* out_valid);" in hdr
    src, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "sdfgpu.h"\nint main(void) {\n'
                'int (*update)(sdfgpu_dsh_map, uint32_t, uint32_t*, void*) = sdfgpu_dsh_update_components;\n'
                'int (*info)(sdfgpu_dsh_map, uint32_t*, uint32_t*, int*) = sdfgpu_dsh_components_info;\n'
                'printf("flag %d size %zu %d\\n", SDFGPU_DSH_COMPONENTS_UNKNOWN_APART, sizeof(sdfgpu_dsh_counts), update == 0 || info == 0);\nreturn 0;\n}\n')
    pkg = os.path.join(ROOT, "sdf_tools_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", pkg, "-lsdfgpu", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["flag", "1", "size", str(capi.DSH_COUNTS_DTYPE.itemsize), "0"]           # (sdfgpu_dsh_counts is as it was: 7 uint64)
    assert capi.DSH_COUNTS_DTYPE.itemsize == 56
    for name in ("sdfgpu_dsh_update_components", "sdfgpu_dsh_components_info"):
        assert name in capi.EXPORTS and hasattr(capi.load_library(), name)
    assert callable(capi.DshMap.update_components) and callable(capi.DshMap.components_info)


def test_a_null_map_is_refused_without_a_gpu():                               # (-1: SDFGPU_ERR_INVALID_ARGUMENT)
    lib = capi.load_library()
    assert lib.sdfgpu_dsh_components_info(None, None, None, None) == -1
    assert lib.sdfgpu_dsh_update_components(None, 0, None, None) == -1


# ---- the host arithmetic under the sanitizers --------------------------------------------------------------------------------------------
def test_node_bases_size_edge_scratch_and_face_pairing_under_asan_and_ubsan(tmp_path):
    tests = os.path.join(ROOT, "tests")
    exe = str(tmp_path / "dsh_components_plan_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(tests, "dsh_components_plan_harness.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "dsh components plan OK" in r.stdout, r.stdout + r.stderr
