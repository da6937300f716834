"""GPU: the dynamic spatial hashed map (sdfgpu_dsh_*, include/sdfgpu.h "Dynamic spatial hashed map") against
the restatement of its contract (tests/dsh_restated.py): records compared as bytes, no cell excused."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dsh_restated as R
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 2, 5), (4, 4, 4), (8, 8, 32)]
NAN_A, NAN_B = R.record_bits(0x7FC00001, 5), R.record_bits(0xFFC12345, 0xFFFFFFFF)       # two NaN occupancies with payloads
VALUES = [R.record(1.0, 1), R.record(0.0, 2), R.record(0.5, 3), R.record(0.75, 0xDEADBEEF), NAN_A, NAN_B, R.record(-0.0, 0), R.record(0.25, 77)]
DEFAULT = R.record(0.0, 0xABCD)


def rigid(q, t):
    """(origin, inverse) of a rotation quaternion (w, x, y, z) and a translation, both 4 x 4 float64"""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    origin, inverse = np.eye(4), np.eye(4)
    origin[:3, :3], origin[:3, 3] = rot, t
    inverse[:3, :3], inverse[:3, 3] = rot.T, -rot.T @ np.asarray(t, np.float64)
    return origin, inverse


class Pair:
    """the map on the GPU and its restatement, driven together"""

    def __init__(self, ctx, inverse=None, cell_size=1.0, chunk_dims=(4, 4, 4), default=DEFAULT, **kw):
        self.gpu = ctx.dsh_create(inverse, cell_size, chunk_dims, default, **kw)
        self.ref = R.Map(inverse, cell_size, chunk_dims, default)

    def close(self):
        self.gpu.close()

    def set_cells(self, loc, value):
        got, want = self.gpu.set_cells(loc, value), self.ref.set_cells(loc, value)
        assert np.array_equal(got, want), "SetCell statuses"

    def set_chunks(self, loc, value):
        got, want = self.gpu.set_chunks(loc, value), self.ref.set_chunks(loc, value)
        assert np.array_equal(got, want), "SetChunk statuses"

    def check_get(self, loc, what=""):
        rec, st = self.gpu.get(loc)
        want_rec, want_st = self.ref.get_batch(loc)
        assert np.array_equal(st, want_st), "Get statuses " + what
        assert np.array_equal(rec, want_rec), "Get records " + what

    def check(self, what=""):
        """the full export and the counts equal the restatement's"""
        chunks, cells = self.gpu.export()
        want, want_cells = self.ref.export()
        assert len(chunks) == len(want), "%s: %d chunks, the restatement has %d" % (what, len(chunks), len(want))
        if want:
            assert np.array_equal(chunks["c"], np.array([w[0] for w in want], np.int64)), what + ": chunk coordinates or their order"
            assert np.array_equal(chunks["state"], np.array([w[1] for w in want], np.uint32)), what + ": chunk states"
            assert np.array_equal(chunks["record"], np.array([w[2] for w in want], np.uint64)), what + ": chunk records"
            assert np.array_equal(chunks["first_cell"], np.array([w[3] for w in want], np.int64)), what + ": cell offsets"
            assert not chunks["reserved"].any()
        assert cells.shape == want_cells.shape and np.array_equal(cells, want_cells), what + ": cell records"
        info = self.gpu.info()
        assert (info["chunk_filled"], info["cell_filled"]) == self.ref.counts(), what
        assert info["capacity_chunks"] >= len(want) and info["table_capacity"] >= 2 * len(want)
        assert info["bytes_held"] == info["table_capacity"] * 12 + info["capacity_chunks"] * (24 + 8 * self.gpu.cells_per_chunk)
        return info


@pytest.fixture
def pair(gpu):
    made = []

    def make(**kw):
        made.append(Pair(gpu, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


def boundary_locations(n, cell):
    """every combination of a few multiples of the cell size per axis: 0, the cell and chunk boundaries around it, negative multiples"""
    axes = []
    for a in range(3):
        k = sorted({0, 1, -1, n[a] - 1, n[a], n[a] + 1, -n[a] + 1, -n[a], -n[a] - 1, -2 * n[a], 2 * n[a]})
        axes.append(np.array(k, np.float64) * cell)
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    return g


# ---- exact-boundary locations --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("cell,shift", [(0.25, (0, 0, 0)), (2.0, (3, -5, 1))], ids=["quarter-identity", "two-translated"])
def test_locations_exactly_on_cell_and_chunk_boundaries(pair, dims, cell, shift):
    inverse = np.eye(4)
    inverse[:3, 3] = -np.asarray(shift, np.float64) * cell                 # the origin translated by whole cells
    p = pair(inverse=inverse, cell_size=cell, chunk_dims=dims)
    loc = boundary_locations(dims, cell) + np.asarray(shift, np.float64) * cell
    rng = np.random.default_rng(1)
    loc = loc[rng.permutation(len(loc))[:600]]
    values = rng.integers(1, 1 << 63, len(loc), dtype=np.uint64)
    for k, row in enumerate(loc):                                            # the restatement places each on the low side of its boundary
        assert p.ref.global_cell(row) == tuple(int(round(v / cell)) - s for v, s in zip(row, shift)), k
    p.set_cells(loc, values)
    p.check("cells on boundaries")
    p.check_get(loc)
    p.check_get(loc - cell / 4, "a quarter cell below")
    p.set_chunks(loc[::7], values[::7])
    p.check("chunks on boundaries")
    p.check_get(loc)


@pytest.mark.parametrize("dims", [(3, 2, 5), (8, 8, 32)], ids=lambda d: "x".join(map(str, d)))
def test_cell_centres_through_a_rotated_origin(pair, dims):
    origin, inverse = rigid((0.9, 0.1, -0.3, 0.25), (0.37, -1.21, 2.5))
    cell = 0.05
    p = pair(inverse=inverse, cell_size=cell, chunk_dims=dims)
    rng = np.random.default_rng(2)
    cells = rng.integers(-40, 40, (800, 3))
    centres = np.array([p.ref.cell_centre(origin, cell, c) for c in cells])
    for c, w in zip(cells, centres):
        assert p.ref.global_cell(w) == tuple(int(v) for v in c)              # half a cell from any boundary: all of them count
    values = rng.integers(1, 1 << 63, len(cells), dtype=np.uint64)
    p.set_cells(centres, values)
    p.check("rotated origin")
    p.check_get(centres)


# ---- the order inside a batch ----------------------------------------------------------------------------------------------------------
def test_one_cell_set_three_times_in_one_batch(pair):
    p = pair(chunk_dims=(3, 2, 5))
    loc = [(0.5, 0.5, 0.5), (7.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (7.5, 0.5, 0.5)]
    p.set_cells(loc, VALUES[:5])
    assert p.gpu.get([(0.5, 0.5, 0.5)])[0][0] == VALUES[3] and p.gpu.get([(7.5, 0.5, 0.5)])[0][0] == VALUES[4]
    p.check()
    p.set_cells(loc[::-1], VALUES[:5])
    assert p.gpu.get([(0.5, 0.5, 0.5)])[0][0] == VALUES[4]
    p.check()


def test_seventy_thousand_cell_sets_into_five_chunks(pair):
    p = pair(chunk_dims=(4, 4, 4), cell_size=0.5)
    rng = np.random.default_rng(3)
    corner = np.array([(0, 0, 0), (-4, 0, 0), (0, -4, 8), (12, 12, 12), (-8, -8, -8)])
    cells = corner[rng.integers(0, 5, 70000)] + rng.integers(0, 4, (70000, 3))           # 320 cells: about 220 writes each
    loc = (cells + rng.random((70000, 3)) * 0.98 + 0.01) * 0.5
    values = rng.integers(1, 1 << 63, 70000, dtype=np.uint64)
    p.set_cells(loc, values)
    info = p.check("70 000 sets")
    assert info["cell_filled"] == 5 and info["chunk_filled"] == 0


def test_duplicate_chunk_sets(pair):
    p = pair(chunk_dims=(3, 2, 5))
    rng = np.random.default_rng(4)
    loc = rng.integers(-9, 9, (3000, 3)).astype(np.float64) + 0.5
    values = rng.integers(1, 1 << 63, 3000, dtype=np.uint64)
    p.set_chunks(loc, values)
    p.check("duplicate chunk sets")
    p.set_chunks(loc[:11], VALUES[0])
    p.check("one value")


# ---- state changes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_operation", [False, True], ids=["one-value", "per-operation"])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_state_changes_and_get_in_all_three_states(pair, dims, per_operation):
    p = pair(chunk_dims=dims)
    n = np.asarray(dims, np.float64)
    inside = lambda c, f: (np.asarray(c) + np.asarray(f)) * n                # a location at fraction f of chunk c

    def val(k, count):
        return np.array([VALUES[(k + j) % len(VALUES)] for j in range(count)], np.uint64) if per_operation else VALUES[k % len(VALUES)]
    probes = np.array([inside(c, f) for c in [(0, 0, 0), (-1, 0, 0), (0, -1, 2), (5, 5, 5)] for f in [(0, 0, 0), (0.5, 0.5, 0.5), (0.99, 0.99, 0.99)]])
    p.check_get(probes, "empty map")
    # SetChunk, then SetCell: the other cells keep the chunk's record
    p.set_chunks([inside((0, 0, 0), (0.5, 0.5, 0.5)), inside((-1, 0, 0), (0, 0, 0))], val(0, 2))
    p.check("chunk-filled")
    p.check_get(probes, "chunk-filled")
    p.set_cells([inside((0, 0, 0), (0.99, 0.99, 0.99)), inside((0, -1, 2), (0, 0, 0))], val(3, 2))
    p.check("chunk -> cells, absent -> cells")
    p.check_get(probes, "all three states")
    # SetCell, then SetChunk: the cells are dropped
    p.set_chunks([inside((0, -1, 2), (0.5, 0.5, 0.5))], val(5, 1))
    p.check("cells -> chunk")
    p.check_get(probes, "cells -> chunk")
    # both changes of one chunk in consecutive batches, then NaN occupancies and full component words
    p.set_cells([inside((0, -1, 2), (0.5, 0.5, 0.5))], NAN_A)
    p.set_chunks([inside((5, 5, 5), (0, 0, 0))], NAN_B)
    p.check("NaN records")
    p.check_get(probes, "NaN records")
    rec, st = p.gpu.get([inside((0, -1, 2), (0.5, 0.5, 0.5)), inside((5, 5, 5), (0.5, 0.5, 0.5))])
    assert rec.tolist() == [NAN_A, NAN_B] and st.tolist() == [capi.DSH_FOUND_IN_CELL, capi.DSH_FOUND_IN_CHUNK]


def test_invalid_locations_in_the_middle_of_a_batch(pair):
    p = pair(chunk_dims=(3, 2, 5))
    edge = float(1 << 20)
    loc = np.array([(0.5, 0.5, 0.5), (np.nan, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (2.5, 0.5, 0.5),
                    (edge * 3, 0.5, 0.5), (0.5, -edge * 2 - 0.5, 0.5), (0.5, 0.5, edge * 5), (0.5, 0.5, -edge * 5), (0.5, 0.5, edge * 5 - 0.5),
                    (-edge * 3, -edge * 2, -edge * 5), (1e300, 0.5, 0.5), (0.5, 1.5, 0.5)])
    values = np.arange(1, len(loc) + 1, dtype=np.uint64)
    want = [2, 0, 2, 0, 0, 2, 0, 0, 0, 2, 2, 2, 0, 2]
    p.set_cells(loc, values)
    assert p.ref.set_cells(loc, values).tolist() == want
    p.check("cells")
    p.check_get(loc)
    p.set_chunks(loc, values)
    p.check("chunks")
    p.check_get(loc)
    rec, st = p.gpu.get(loc)
    assert [int(s != 0) for s in st] == [w // 2 for w in want] and all(int(r) == DEFAULT for r, s in zip(rec, st) if s == 0)


# ---- growth and long probe chains ------------------------------------------------------------------------------------------------------
def test_growth_from_the_smallest_table_and_a_one_chunk_pool(pair):
    p = pair(chunk_dims=(3, 2, 5), initial_chunks=1)
    info = p.gpu.info()
    assert info["table_capacity"] == 16 and info["capacity_chunks"] == 1
    rng = np.random.default_rng(5)
    n = np.array([3.0, 2.0, 5.0])
    line = np.arange(-1200, 1200)
    zeros = np.zeros_like(line)
    block = np.stack(np.meshgrid(np.arange(12) - 6, np.arange(12) + 100, np.arange(12) - 1000, indexing="ij"), -1).reshape(-1, 3)
    chunks = np.concatenate([np.stack([line, zeros, zeros], 1), np.stack([zeros, line, zeros - 1], 1), np.stack([zeros - 1, zeros - 1, line], 1), block])
    chunks = np.unique(chunks, axis=0)
    assert len(chunks) >= 8000
    chunks = chunks[rng.permutation(len(chunks))][:8000]
    loc = (chunks + rng.random(chunks.shape) * 0.98 + 0.01) * n
    values = rng.integers(1, 1 << 63, len(loc), dtype=np.uint64)
    p.set_cells(loc[:5000], values[:5000])
    info = p.check("5000 chunks in one batch")
    assert info["cell_filled"] == 5000 and info["capacity_chunks"] >= 5000
    seen = {(info["table_capacity"], info["capacity_chunks"])}
    for b in range(30):
        s = slice(5000 + 100 * b, 5100 + 100 * b)
        if b % 3 == 2:
            p.set_chunks(loc[s], values[s])
        else:
            p.set_cells(loc[s], values[s] if b % 2 else VALUES[b % len(VALUES)])
        info = p.check("batch %d" % b)
        seen.add((info["table_capacity"], info["capacity_chunks"]))
    assert len(seen) >= 2, "the map never grew after the first batch"
    assert info["chunk_filled"] + info["cell_filled"] == 8000
    p.check_get(loc[::5])


# ---- the byte limit --------------------------------------------------------------------------------------------------------------------
def test_a_batch_that_would_pass_the_byte_limit_is_refused_and_changes_nothing(pair, gpu):
    dims, cpc = (4, 4, 4), 64
    limit = 32 * 12 + 8 * (24 + 8 * cpc)                                    # a table of 32 entries and a pool of 8 chunks
    p = pair(chunk_dims=dims, initial_chunks=4, byte_limit=limit)
    at = lambda k: (4.0 * k + 0.5, 0.5, 0.5)
    p.set_cells([at(0), at(1), at(2)], VALUES[:3])
    p.set_chunks([at(3), at(4), at(5)], VALUES[3:6])
    before = p.check("six chunks")
    assert before["byte_limit"] == limit and before["bytes_held"] <= limit
    probes = np.array([at(k) for k in range(-2, 40)])

    def device(call, dtype):
        def run(loc, value):
            d = torch.from_numpy(np.ascontiguousarray(loc, dtype=dtype)).cuda()
            call(d.data_ptr(), len(loc), one_value=value) if call != p.gpu.insert_points_device else call(d.data_ptr(), len(loc), value)
            torch.cuda.synchronize()
        return run
    entries = {"set_cells": lambda loc, v: p.gpu.set_cells(loc, v), "set_chunks": lambda loc, v: p.gpu.set_chunks(loc, v),
               "set_cells_device": device(p.gpu.set_cells_device, np.float64), "set_chunks_device": device(p.gpu.set_chunks_device, np.float64),
               "insert_points_device": device(p.gpu.insert_points_device, np.float32)}
    for name, call in entries.items():
        # five new chunks beside the six: the table takes them (32 entries), the pool would need 11 chunks -- refused after the insert
        # 40 new chunks: the table itself would pass the limit -- refused before anything is enqueued
        for count in (5, 40):
            with pytest.raises(capi.SdfGpuError) as e:
                call([at(2)] + [at(10 + k) for k in range(count)], VALUES[0])
            assert e.value.code == -3 and "byte limit" in str(e.value), name
            after = p.check("%s refused with %d new chunks" % (name, count))
            assert after["bytes_held"] <= limit
            p.check_get(probes, name)
    # what fits is still taken, and the keys of the refused batches are not in the table
    p.set_cells([at(10), at(11)], VALUES[6:8])
    info = p.check("two more chunks")
    assert info["cell_filled"] + info["chunk_filled"] == 8 and info["bytes_held"] <= limit
    p.check_get(probes)
    with pytest.raises(capi.SdfGpuError):
        gpu.dsh_create(None, 1.0, dims, 0, initial_chunks=64, byte_limit=1000)


# ---- windows -----------------------------------------------------------------------------------------------------------------------------
def window_scene(pair):
    """chunks of 3 x 2 x 5 around the origin in all three states, with occupancies 0, exactly 0.5, above, and NaN"""
    p = pair(chunk_dims=(3, 2, 5), default=R.record(0.5, 0x11))
    rng = np.random.default_rng(6)
    n = np.array([3.0, 2.0, 5.0])
    chunk_filled = [(-2, -1, -2), (-1, 0, -1), (0, -1, 0), (1, 1, 3), (0, 0, 5), (-2, 0, 6)]
    p.set_chunks([(np.array(c) + 0.5) * n for c in chunk_filled], np.array([R.record(1.0, 1), R.record(0.5, 2), R.record(0.0, 3), NAN_A, R.record(0.75, 4), R.record(0.5, 5)], np.uint64))
    cell_filled = [(-2, -1, -1), (-1, -1, -2), (0, 0, 0), (1, 0, 2), (-1, 1, 4), (0, -1, 6), (1, -1, -2)]
    for c in cell_filled:
        loc = (np.array(c) + rng.random((20, 3))) * n
        occ = rng.choice(np.array([0.0, 0.5, 0.5, 1.0, 0.51, np.nan], np.float32), 20)
        p.set_cells(loc, np.array([R.record(o, k) for k, o in enumerate(occ)], np.uint64))
    return p


WINDOWS = [((-5, -2, -9), (5, 3, 33)), ((-4, -1, -7), (7, 6, 31)), ((-1, -2, -6), (4, 4, 64)), ((-6, -2, -6), (3, 3, 3))]


@pytest.mark.parametrize("lower,shape", WINDOWS, ids=["5x3x33", "7x6x31", "4x4x64", "3x3x3"])
def test_windows_over_chunks_of_all_three_states(pair, gpu, lower, shape):
    p = window_scene(pair)
    want = p.ref.window(lower, shape)
    n_vox = int(np.prod(shape))
    if shape != (3, 3, 3):
        touched = {(p.ref.split((lower[0] + x, lower[1] + y, lower[2] + z))[0]) for x in range(shape[0]) for y in range(shape[1]) for z in range(shape[2])}
        states = {p.ref.chunks[c][0] if c in p.ref.chunks else "absent" for c in touched}
        assert len(touched) >= 8 and states == {"absent", "chunk", "cells"} and any(l % m for l, m in zip(lower, (3, 2, 5)))
    assert (R.occupancy(want) == np.float32(0.5)).any()
    for unknown in (False, True):
        want_bits = R.pack_bits(R.classify(want, unknown))
        rec, bits = p.gpu.extract_window(lower, shape, unknown)
        assert np.array_equal(rec, want), "records"
        assert np.array_equal(bits, want_bits), "bits beside records"
        assert np.array_equal(bits, R.pack_bits(R.classify(rec, unknown))), "the bits are the classify of the records"
        assert np.array_equal(p.gpu.extract_window(lower, shape, unknown, records=False)[1], want_bits), "bits alone"
        assert np.array_equal(p.gpu.extract_window(lower, shape, unknown, bits=False)[0], want), "records alone"
        # the device form into buffers nobody cleared, then the SDF build that reads the bits in place
        d_rec = torch.full((n_vox,), -1, dtype=torch.int64, device="cuda")
        d_bits = torch.full(((n_vox + 31) // 32,), -1, dtype=torch.int32, device="cuda")
        d_sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        p.gpu.extract_window_device(lower, shape, unknown, d_rec.data_ptr(), d_bits.data_ptr(), stream)
        gpu.build_bits_device(d_bits.data_ptr(), shape, d_sdf.data_ptr(), 0.25, False, stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_rec.cpu().numpy().view(np.uint64).reshape(shape), want) and np.array_equal(d_bits.cpu().numpy().view(np.uint32), want_bits)
        want_sdf, _ = gpu.build_cells(want.view(np.float32), shape, 8, 0, unknown, 0.25, False)
        assert np.array_equal(d_sdf.cpu().numpy().view(np.uint32), want_sdf.view(np.uint32)), "the SDF of the bits differs from the SDF of the records"
        d_bits.fill_(-1)
        p.gpu.extract_window_device(lower, shape, unknown, 0, d_bits.data_ptr(), stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_bits.cpu().numpy().view(np.uint32), want_bits), "device bits alone"


def test_a_window_beyond_the_chunk_range_reads_the_default(pair):
    p = pair(chunk_dims=(1, 1, 1), default=R.record(1.0, 9))
    edge = 1 << 20
    p.set_cells([(edge - 0.5, 0.5, 0.5)], VALUES[1])
    lower, shape = (edge - 2, 0, 0), (4, 1, 2)
    rec, bits = p.gpu.extract_window(lower, shape, False)
    assert np.array_equal(rec, p.ref.window(lower, shape)) and rec[1, 0, 0] == VALUES[1] and rec[2, 0, 0] == R.record(1.0, 9)
    assert bits.tolist() == [0b11111011]                                    # voxel 2 = (1, 0, 0) is the one cell that was set, to free
    with pytest.raises(capi.SdfGpuError):
        p.gpu.extract_window((0, 0, 0), (1 << 16, 1 << 16, 1), False, records=False)


# ---- export ------------------------------------------------------------------------------------------------------------------------------
def test_export_lists_and_display_points(pair):
    origin, inverse = rigid((0.8, -0.2, 0.1, 0.55), (1.5, -0.25, 0.75))
    cell = 0.125
    p = pair(inverse=inverse, cell_size=cell, chunk_dims=(3, 2, 5))
    chunks, cells = p.gpu.export()
    assert len(chunks) == 0 and cells.shape == (0, 3, 2, 5) and p.gpu.info()["chunk_filled"] == 0        # an empty map: nothing to draw
    rng = np.random.default_rng(8)
    centres = np.array([p.ref.cell_centre(origin, cell, c) for c in rng.integers(-30, 30, (300, 3))])
    p.set_cells(centres[:200], rng.integers(1, 1 << 63, 200, dtype=np.uint64))
    p.set_chunks(centres[150:], rng.integers(1, 1 << 63, 150, dtype=np.uint64))
    p.check("export")
    chunks, cells = p.gpu.export()
    # the device form into the caller's buffers: the same lists
    d_chunks = torch.zeros(len(chunks) * 48, dtype=torch.uint8, device="cuda")
    d_cells = torch.zeros(max(cells.size, 1), dtype=torch.int64, device="cuda")
    assert p.gpu.export_device(0, 0, 0, 0) == (len(chunks), cells.size)
    assert p.gpu.export_device(d_chunks.data_ptr(), len(chunks) - 1, d_cells.data_ptr(), cells.size) == (len(chunks), cells.size)
    assert not d_chunks.any(), "a list whose capacity is too small must not be written"
    assert p.gpu.export_device(d_chunks.data_ptr(), len(chunks), d_cells.data_ptr(), cells.size, torch.cuda.current_stream().cuda_stream) == (len(chunks), cells.size)
    torch.cuda.synchronize()
    assert d_chunks.cpu().numpy().tobytes() == chunks.tobytes() and np.array_equal(d_cells.cpu().numpy().view(np.uint64)[:cells.size], cells.reshape(-1))
    # display points in double: chunk markers at chunk centres, cell markers at cell centres, in the export's order
    want_chunks, _ = p.ref.export()
    for got, (c, state, _, first) in zip(chunks, want_chunks):
        assert tuple(got["c"]) == c
        if state == R.FOUND_IN_CHUNK:
            centre = p.ref.chunk_centre(origin, cell, c)
            back = p.ref.global_cell(centre)
            assert p.ref.split(back)[0] == c


# ---- red zones -------------------------------------------------------------------------------------------------------------------------
def core_cases_on(ctx):
    made = []

    def make(**kw):
        made.append(Pair(ctx, **kw))
        return made[-1]
    try:
        test_one_cell_set_three_times_in_one_batch(make)
        test_duplicate_chunk_sets(make)
        test_invalid_locations_in_the_middle_of_a_batch(make)
        test_growth_from_the_smallest_table_and_a_one_chunk_pool(make)
        for lower, shape in WINDOWS:
            p = window_scene(make)
            rec, bits = p.gpu.extract_window(lower, shape, True)
            assert np.array_equal(rec, p.ref.window(lower, shape)) and np.array_equal(bits, R.pack_bits(R.classify(rec, True)))
        test_export_lists_and_display_points(make)
    finally:
        for p in made:
            p.close()


def test_the_core_cases_in_a_child_process_with_red_zones_from_the_environment():
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from sdf_tools_amd import capi\nimport test_gpu_dsh as T\n"
            "ctx = capi.SdfGpu(0)\nT.core_cases_on(ctx)\nctx.redzone_check()\nctx.close()\nprint('core cases clean')\n") % (tests, os.path.dirname(tests))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SDFGPU_REDZONE="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "core cases clean" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
