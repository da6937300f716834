"""GPU: the connected components of the dynamic spatial hashed map (sdfgpu_dsh_update_components, sdfgpu_dsh_components_info;
include/sdfgpu.h "Dynamic spatial hashed map: connected components") against the restatement of their contract
(tests/dsh_components_restated.py, a breadth-first search on a tests/dsh_restated.py map).  Every comparison is bit for bit: the
labels are read through the export and through Get on every cell of every live chunk, and everything but the component words must
be what it was."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dsh_components_restated as C
import dsh_restated as R
from sdf_tools_amd import capi
from test_gpu_dsh import Pair

pytestmark = pytest.mark.gpu

APART = capi.DSH_COMPONENTS_UNKNOWN_APART
RULES = (0, APART)
FREE, FILLED, UNKNOWN = R.record(0.0, 0x10), R.record(1.0, 0x20), R.record(0.5, 0x30)
NAN_CELL = R.record_bits(0x7FC00001, 5)
BELOW, ABOVE = R.record_bits(0x3EFFFFFF, 6), R.record_bits(0x3F000001, 7)     # the two float neighbours of 0.5f
DEFAULT = R.record(0.5, 0xABCD)
# chunk shapes, and the chunk coordinates a mixed scene of each uses (every shape has neighbours along all three axes that it has)
SHAPES = [(1, 1, 1), (3, 2, 5), (4, 4, 4), (8, 8, 32), (32, 32, 32), (32768, 1, 1), (1, 1, 32768), (20, 20, 41), (3, 1, 2731)]
CORNER = [(0, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (-1, -1, 0)]
DOZEN = [(x, y, z) for x in (-1, 0) for y in (-1, 0, 1) for z in (0, 1)]
BLOCKS = {(1, 1, 1): (6, 6, 6), (3, 2, 5): (3, 3, 3), (4, 4, 4): (3, 3, 3), (8, 8, 32): (3, 3, 2)}


def block(extent, first=(-1, -1, -1)):
    return [(first[0] + x, first[1] + y, first[2] + z) for x in range(extent[0]) for y in range(extent[1]) for z in range(extent[2])]


def centres(c, n):
    """the centres of chunk c's cells in slot order (identity origin, cell size 1), float64 [cells, 3]"""
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), -1).reshape(-1, 3)
    return idx + np.array(c) * np.array(n) + 0.5


class ComponentsPair(Pair):
    """the map on the GPU and its restatement; whole chunks are written at once, and an update is compared in every way the labels
    can be read"""

    def put_cells(self, c, records):
        """chunk c becomes cell-filled with these records [n_x, n_y, n_z]"""
        n = self.ref.n
        st = self.gpu.set_cells(centres(c, n), np.asarray(records, np.uint64).reshape(-1))
        assert (st == R.SET_CELL).all()
        self.ref.chunks[tuple(c)] = ("cells", np.array(records, np.uint64).reshape(n))

    def put_chunk(self, c, record):
        self.set_chunks([(np.array(c) + 0.5) * np.array(self.ref.n)], record)

    def remove(self, coords):
        n = np.array(self.ref.n)
        _, removed = self.gpu.remove_chunks([(np.array(c) + 0.5) * n for c in coords])
        assert removed == len(coords)
        for c in coords:
            del self.ref.chunks[tuple(c)]

    def every_cell(self):
        """(locations of every cell of every live chunk, the records Get must return there)"""
        loc, want = [], []
        for c, (kind, what) in self.ref.chunks.items():
            loc.append(centres(c, self.ref.n))
            want.append(np.asarray(what, np.uint64).reshape(-1) if kind == "cells" else np.full(len(loc[-1]), what, np.uint64))
        return (np.concatenate(loc), np.concatenate(want)) if loc else (np.zeros((0, 3)), np.zeros(0, np.uint64))

    def update(self, flags, what=""):
        """update the components on the GPU and in the restatement; compare K, the info, the export, Get everywhere, and what must stay"""
        chunks0, cells0 = self.gpu.export()
        info0 = self.gpu.info()
        count = self.gpu.update_components(flags)
        want = C.apply(self.ref, flags)
        assert count == want, "%s: K = %d, the restatement has %d (flags %d)" % (what, count, want, flags)
        assert self.gpu.components_info() == (want, flags, True), what
        info = self.check(what + ": the export after the update")
        drop = lambda i: {k: v for k, v in i.items() if k != "scratch_bytes"}
        assert drop(info) == drop(info0), what + ": info"
        chunks, cells = self.gpu.export()
        low = np.uint64(0xFFFFFFFF)
        assert np.array_equal(cells & low, cells0 & low) and np.array_equal(chunks["record"] & low, chunks0["record"] & low), what + ": an occupancy changed"
        for field in ("c", "state", "reserved", "first_cell"):
            assert np.array_equal(chunks[field], chunks0[field]), what + ": " + field
        loc, want_records = self.every_cell()
        if len(loc):
            rec, st = self.gpu.get(loc)
            assert np.array_equal(rec, want_records), "%s: %d records differ through Get" % (what, (rec != want_records).sum())
            assert (st != R.NOT_FOUND).all()
        return count

    def update_both(self, what=""):
        return [self.update(flags, "%s, flags %d" % (what, flags)) for flags in RULES]


@pytest.fixture
def pair(gpu):
    made = []

    def make(**kw):
        kw.setdefault("default", DEFAULT)
        made.append(ComponentsPair(gpu, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


def bernoulli(rng, n, prob, sprinkle=True):
    """records [n]: filled with probability prob, else free; a few cells of exactly 0.5, its float neighbours and NaN among them"""
    cells = np.where(rng.random(n) < prob, np.uint64(FILLED), np.uint64(FREE))
    if sprinkle:
        odd = rng.random(n)
        for k, rec in enumerate((UNKNOWN, NAN_CELL, BELOW, ABOVE)):
            cells = np.where((odd >= 0.03 * k) & (odd < 0.03 * (k + 1)), np.uint64(rec), cells)
    return cells


def mixed_scene(p, rng, coords, prob=0.5, cells_share=0.6):
    """chunks of every state on `coords`: cell-filled ones (Bernoulli), chunk-filled ones of all three classes"""
    for k, c in enumerate(coords):
        if k == 0 or rng.random() < cells_share:
            p.put_cells(c, bernoulli(rng, p.ref.n, prob))
        else:
            p.put_chunk(c, (FREE, FILLED, UNKNOWN, NAN_CELL)[int(rng.integers(0, 4))])


# ---- chunk shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_a_mixed_scene_of_each_chunk_shape_under_both_rules(pair, dims):
    rng = np.random.default_rng(sum(dims))
    p = pair(chunk_dims=dims)
    coords = block(BLOCKS[dims]) if dims in BLOCKS else DOZEN if max(dims) == 32768 else CORNER
    mixed_scene(p, rng, coords, cells_share=0.75)
    counts = p.update_both("x".join(map(str, dims)))
    assert counts[1] >= counts[0] >= 2


# ---- maps ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob", [0.3, 0.5, 0.7])
def test_bernoulli_occupancies_over_a_block_of_chunks_with_some_removed(pair, prob):
    rng = np.random.default_rng(int(prob * 10))
    p = pair(chunk_dims=(4, 4, 4))
    coords = block((3, 3, 3))                                                  # chunk coordinates -1 .. 1: negative, and straddling 0
    mixed_scene(p, rng, coords, prob, cells_share=0.8)
    p.update_both("the whole block")
    gone = [coords[k] for k in rng.choice(len(coords), 6, replace=False)]
    p.remove(gone)
    assert p.gpu.components_info()[2] is False
    p.update_both("six chunks removed")


def test_all_four_state_pairs_along_all_three_axes(pair):
    rng = np.random.default_rng(4)
    p = pair(chunk_dims=(3, 2, 5))
    for axis in range(3):
        for k, (low_cells, high_cells) in enumerate([(True, True), (True, False), (False, True), (False, False)]):
            for same_class in (False, True):
                c = [10 * axis, 3 * (2 * k + same_class), 0]                   # every pair stands alone
                for cells, step in ((low_cells, 0), (high_cells, 1)):
                    at = list(c)
                    at[axis] += step
                    if cells:
                        p.put_cells(at, bernoulli(rng, p.ref.n, 0.5))
                    else:
                        p.put_chunk(at, FREE if same_class or step == 0 else FILLED)
    p.update_both("state pairs")
    # two chunk-filled chunks of one class are one component, of two classes two
    pairs = p.ref.chunks[(0, 18, 0)], p.ref.chunks[(1, 18, 0)], p.ref.chunks[(0, 21, 0)], p.ref.chunks[(1, 21, 0)]
    assert all(kind == "chunk" for kind, _ in pairs)
    assert pairs[0][1] >> 32 != pairs[1][1] >> 32 and pairs[2][1] >> 32 == pairs[3][1] >> 32


def test_chunks_at_both_ends_of_the_key_range(pair):
    rng = np.random.default_rng(5)
    p = pair(chunk_dims=(2, 2, 2))
    lo, hi = -(1 << 20), (1 << 20) - 1
    p.put_cells((lo, lo, lo), bernoulli(rng, (2, 2, 2), 0.5, False))
    p.put_cells((lo + 1, lo, lo), bernoulli(rng, (2, 2, 2), 0.5, False))
    p.put_chunk((lo, lo + 1, lo), FREE)
    p.put_cells((hi, hi, hi), bernoulli(rng, (2, 2, 2), 0.5, False))
    p.put_chunk((hi, hi, hi - 1), FILLED)
    p.put_cells((hi - 1, hi, hi), bernoulli(rng, (2, 2, 2), 0.5, False))
    p.put_cells((lo, 0, hi), bernoulli(rng, (2, 2, 2), 0.5, False))
    p.update_both("key edges")


def serpentine(size):
    """filled everywhere but a corridor of free cells that snakes through every row of every second layer of a size^3 block"""
    occ = np.ones((size, size, size), bool)
    for z in range(0, size, 2):
        for y in range(0, size, 2):
            occ[:, y, z] = False
            if y + 2 < size:
                occ[size - 1 if (y // 2) % 2 == 0 else 0, y + 1, z] = False     # the turn into the next row
        if z + 2 < size:
            last = size - 2 if size % 2 == 0 else size - 1                     # the last row of this layer, and the end the snake leaves it at
            occ[size - 1 if (last // 2) % 2 == 0 else 0, last, z + 1] = False   # straight up: the layer above runs its rows the same way
    return occ


def test_a_serpentine_corridor_through_a_block_of_chunks(pair):
    p = pair(chunk_dims=(4, 4, 4))
    occ = serpentine(16)
    for c in block((4, 4, 4), (0, 0, 0)):
        part = occ[4 * c[0]:4 * c[0] + 4, 4 * c[1]:4 * c[1] + 4, 4 * c[2]:4 * c[2] + 4]
        p.put_cells(c, np.where(part, np.uint64(FILLED), np.uint64(FREE)))
    count = p.update(0, "serpentine")
    labels = np.concatenate([np.asarray(w, np.uint64).reshape(-1) >> np.uint64(32) for _, w in p.ref.chunks.values()])
    free = np.concatenate([R.occupancy(np.asarray(w).reshape(-1)) < 0.5 for _, w in p.ref.chunks.values()])
    assert len(set(labels[free].tolist())) == 1, "the corridor is one component"
    assert count == 1 + len(set(labels[~free].tolist()))


def test_a_checkerboard_has_as_many_components_as_nodes(pair):
    p = pair(chunk_dims=(3, 2, 5))
    for c in block((2, 2, 2)):
        g = np.floor(centres(c, (3, 2, 5))).astype(np.int64)                  # global cells
        p.put_cells(c, np.where(g.sum(1) % 2 == 0, np.uint64(FILLED), np.uint64(FREE)))
    assert p.update(0, "checkerboard") == 8 * 30
    assert p.update(APART, "checkerboard") == 8 * 30
    _, cells = p.gpu.export()
    assert np.array_equal(cells.reshape(-1) >> np.uint64(32), np.arange(1, 241, dtype=np.uint64))


def test_an_empty_map_and_a_map_of_one_chunk_filled_chunk(pair):
    p = pair(chunk_dims=(4, 4, 4))
    assert p.gpu.components_info() == (0, 0, False)
    assert p.update(APART, "empty") == 0 and p.gpu.components_info() == (0, APART, True)
    p.put_chunk((3, -2, 1), R.record(0.25, 99))
    assert p.gpu.components_info() == (0, APART, False)
    assert p.update(0, "one chunk") == 1
    chunks, _ = p.gpu.export()
    assert chunks["record"].tolist() == [R.record(0.25, 1)]
    p.remove([(3, -2, 1)])
    assert p.update(0, "empty again") == 0


# ---- slot order against key order ----------------------------------------------------------------------------------------------------------
def test_labels_do_not_depend_on_the_order_chunks_were_inserted_in(pair):
    coords = block((3, 3, 3))
    scenes = {c: bernoulli(np.random.default_rng(7 + k), (3, 2, 5), 0.5) if k % 4 else None for k, c in enumerate(coords)}
    rng = np.random.default_rng(8)
    exports = []
    for order in ("ascending", "descending", "shuffled"):
        p = pair(chunk_dims=(3, 2, 5))
        seq = list(coords) if order == "ascending" else list(reversed(coords)) if order == "descending" else [coords[k] for k in rng.permutation(len(coords))]
        extra = (5, 5, 5)
        for k, c in enumerate(seq):
            if order == "shuffled" and k == 9:
                p.put_cells(extra, bernoulli(rng, (3, 2, 5), 0.5))             # a chunk that goes again: the removal moves another into its slot
            if order == "shuffled" and k == 18:
                p.remove([extra, seq[3]])
                seq.append(seq[3])
            p.put_cells(c, scenes[c]) if scenes[c] is not None else p.put_chunk(c, FREE)
        for flags in RULES:
            p.update(flags, order)
            chunks, cells = p.gpu.export()
            exports.append((flags, chunks.tobytes(), cells.tobytes()))
    for flags in RULES:
        same = [e[1:] for e in exports if e[0] == flags]
        assert same[0] == same[1] == same[2], "the labels depend on the insertion order"


# ---- 0.5 and NaN ------------------------------------------------------------------------------------------------------------------------------
def test_cells_at_exactly_half_and_nan_under_both_rules(pair):
    p = pair(chunk_dims=(1, 1, 8))
    p.put_cells((0, 0, 0), [FREE, UNKNOWN, NAN_CELL, FREE, BELOW, ABOVE, NAN_CELL, UNKNOWN])
    p.put_chunk((0, 0, 1), UNKNOWN)
    p.put_chunk((0, 0, 2), NAN_CELL)
    p.put_cells((0, 0, 3), [UNKNOWN, FREE, FREE, FREE, FREE, FREE, FREE, FILLED])
    assert p.update(0, "half and NaN") == 4
    assert (p.ref.chunks[(0, 0, 0)][1].reshape(-1) >> np.uint64(32)).tolist() == [1, 1, 1, 1, 1, 2, 3, 3]
    assert p.update(APART, "half and NaN") == 7
    assert (p.ref.chunks[(0, 0, 0)][1].reshape(-1) >> np.uint64(32)).tolist() == [1, 2, 2, 3, 3, 4, 5, 5]
    assert p.ref.chunks[(0, 0, 1)][1] >> 32 == p.ref.chunks[(0, 0, 2)][1] >> 32 == 5
    assert (p.ref.chunks[(0, 0, 3)][1].reshape(-1) >> np.uint64(32)).tolist() == [5, 6, 6, 6, 6, 6, 6, 7]


# ---- validity ----------------------------------------------------------------------------------------------------------------------------------
def test_the_validity_table(pair, gpu):
    dims, cpc = (4, 4, 4), 64
    limit = 32 * 12 + 8 * (24 + 8 * cpc)                                       # a table of 32 entries and a pool of 8 chunks
    p = pair(chunk_dims=dims, initial_chunks=4, byte_limit=limit)
    at = lambda k: (4.0 * k + 0.5, 0.5, 0.5)
    for k in range(4):                                                         # (batches of three: the table of 32 entries takes live + operations <= 16)
        p.set_cells([(4.0 * k + 0.5, 0.5, 0.5), (4.0 * k + 1.5, 0.5, 0.5), (4.0 * k + 3.5, 3.5, 3.5)], [FREE, FILLED, UNKNOWN])
    p.put_chunk((4, 0, 0), FREE)
    p.put_chunk((5, 0, 0), FILLED)
    valid = lambda: p.gpu.components_info()[2]

    def fresh(flags=0):
        count = p.update(flags, "validity")
        assert p.gpu.components_info() == (count, flags, True)
        return count

    def sync_ref():
        """the restatement's records from the map's export (for calls the restatement does not model)"""
        chunks, cells = p.gpu.export()
        p.ref.chunks = {}
        for ch in chunks:
            c = tuple(int(v) for v in ch["c"])
            p.ref.chunks[c] = ("chunk", int(ch["record"])) if ch["state"] == R.FOUND_IN_CHUNK else ("cells", cells[int(ch["first_cell"]) // cpc].copy())

    device = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
    assert not valid()
    count = fresh(APART)
    # calls that change nothing keep it: reads, a refused batch, a batch of invalid locations only, empty batches, a removal that removes nothing
    p.gpu.get([at(0)]); p.gpu.export(); p.gpu.info(); p.gpu.extract_window((0, 0, 0), (4, 4, 4)); p.gpu.frontier_cells()
    p.gpu.cast_segments([at(0)], [at(3)], 100.0)
    assert p.gpu.components_info() == (count, APART, True)
    with pytest.raises(capi.SdfGpuError) as e:
        p.gpu.set_cells([at(2)] + [at(10 + k) for k in range(5)], FILLED)       # the pool would need 11 chunks
    assert e.value.code == -3 and valid()
    with pytest.raises(capi.SdfGpuError) as e:
        p.gpu.set_chunks([at(10 + k) for k in range(40)], FILLED)               # the table itself would pass the limit
    assert e.value.code == -3 and valid()
    bad = [(np.nan, 0.0, 0.0), (np.inf, 0.0, 0.0), (1e30, 0.0, 0.0)]
    assert (p.gpu.set_cells(bad, FILLED) == R.NOT_SET).all() and valid()
    assert (p.gpu.set_chunks(bad, FILLED) == R.NOT_SET).all() and valid()
    d_bad = device(bad, np.float32)
    p.gpu.insert_points_device(d_bad.data_ptr(), len(bad), FILLED)
    torch.cuda.synchronize()
    assert valid()
    p.gpu.set_cells(np.zeros((0, 3)), FILLED)
    assert p.gpu.insert_rays(at(0), np.zeros((0, 3), np.float32), 50.0, FREE, FILLED)[1]["rays_hit"] == 0 and valid()
    assert p.gpu.fuse_rays(at(0), np.array([[np.nan, 0, 0]], np.float32), 50.0)[1]["rays_skipped"] == 1 and valid()
    assert p.gpu.remove_chunks([at(20), bad[0]])[1] == 0 and valid()
    assert p.gpu.retain_box((0, 0, 0), (24, 4, 4)) == 0 and valid()
    with pytest.raises(capi.SdfGpuError) as e:
        p.gpu.update_components(2)                                              # an unknown flag bit: refused, and nothing changes
    assert e.value.code == -1 and p.gpu.components_info() == (count, APART, True)
    with pytest.raises(capi.SdfGpuError):
        p.gpu.update_components(0x80000001)
    p.check("nothing has changed the map")
    # shrink moves records byte for byte: it keeps the validity and the labels
    p.gpu.shrink(0)
    assert p.gpu.components_info() == (count, APART, True)
    p.check("after shrink")
    rec, _ = p.gpu.get(p.every_cell()[0])
    assert np.array_equal(rec, p.every_cell()[1])
    # every call that changes the content clears it
    mutators = {
        "set_cells": lambda: p.set_cells([at(1)], FILLED),
        "set_chunks": lambda: p.set_chunks([at(5)], FREE),
        "set_cells_device": lambda: p.gpu.set_cells_device(device([at(0), bad[0]], np.float64).data_ptr(), 2, one_value=FREE),
        "set_chunks_device": lambda: p.gpu.set_chunks_device(device([at(4)], np.float64).data_ptr(), 1, one_value=UNKNOWN),
        "insert_points_device": lambda: p.gpu.insert_points_device(device([at(2)], np.float32).data_ptr(), 1, FILLED),
        "insert_rays": lambda: p.gpu.insert_rays(at(0), np.array([at(3)], np.float32), 50.0, FREE, FILLED),
        "fuse_rays": lambda: p.gpu.fuse_rays(at(0), np.array([at(3)], np.float32), 50.0),
        "insert_rays_device": lambda: p.gpu.insert_rays_device(at(0), device([at(2)], np.float32).data_ptr(), 1, 50.0, FREE, FILLED),
        "fuse_rays_device": lambda: p.gpu.fuse_rays_device(at(0), device([at(2)], np.float32).data_ptr(), 1, 50.0),
        "remove_chunks": lambda: p.gpu.remove_chunks([at(5)]),
        "remove_chunks_device": lambda: p.gpu.remove_chunks_device(device([at(4)], np.float64).data_ptr(), 1),
        "retain_box": lambda: p.gpu.retain_box((0, 0, 0), (12, 4, 4)),
        "remove_box": lambda: p.gpu.remove_box((8, 0, 0), (4, 4, 4)),
        "clear": lambda: p.gpu.clear(),
    }
    for k, (name, call) in enumerate(mutators.items()):
        flags = RULES[k % 2]
        sync_ref()
        count = fresh(flags)
        call()
        torch.cuda.synchronize()
        assert p.gpu.components_info() == (count, flags, False), name
    assert p.gpu.info()["chunk_filled"] + p.gpu.info()["cell_filled"] == 0


def test_two_class_copies_agree_on_the_validity(gpu):
    """two C++ copies of a grid are two names for one map: whatever one of them does, both say the same about the components"""
    import copy
    from sdf_tools_amd._bindings import load_pysdf_tools
    P = load_pysdf_tools()
    a = P.DynamicSpatialHashedCollisionMapGrid("world", 1.0, 3, 2, 5, P.COLLISION_CELL(0.5))
    b = copy.copy(a)
    agree = lambda: (a.AreComponentsValid(), a.GetNumConnectedComponents(), a.components_info()) == (b.AreComponentsValid(), b.GetNumConnectedComponents(), b.components_info())
    rng = np.random.default_rng(13)
    loc = rng.integers(-6, 6, (200, 3)) + 0.5
    a.SetCells(loc, np.array([(FREE, FILLED, UNKNOWN)[k % 3] for k in range(200)], np.uint64))
    assert agree() and not b.AreComponentsValid()
    count = a.UpdateConnectedComponents(True)
    assert agree() and b.AreComponentsValid() and b.GetNumConnectedComponents() == (count, True) and count > 3
    assert b.UpdateConnectedComponents(True) == count and b.components_info() == (count, 1, True)     # the stored count, through the other name
    mutators = [lambda g: g.SetCell(0.5, 0.5, 0.5, P.COLLISION_CELL(1.0)), lambda g: g.SetChunk(0.5, 0.5, 0.5, P.COLLISION_CELL(0.0)),
                lambda g: g.SetCells(loc[:3], P.COLLISION_CELL(1.0)), lambda g: g.FusePointCloudRays(np.array([[4.5, 0.5, 0.5]], np.float32), (0.5, 0.5, 0.5), 20.0),
                lambda g: g.RemoveChunk(0.5, 0.5, 0.5), lambda g: g.RemoveBox((-6, -6, -6), 6, 6, 6), lambda g: g.Clear()]
    for k, change in enumerate(mutators):
        first, second = (a, b) if k % 2 else (b, a)
        plain = first.UpdateConnectedComponents()                              # (the other rule: computed again)
        assert agree() and second.AreComponentsValid() and second.components_info() == (plain, 0, True)
        second.ShrinkToFit()
        assert agree() and first.AreComponentsValid(), "shrink keeps the validity"
        change(second)
        assert agree() and not first.AreComponentsValid() and first.GetNumConnectedComponents() == (plain, False), k
    assert a.GetCounts() == b.GetCounts() and a.GetCounts()["cell_filled"] + a.GetCounts()["chunk_filled"] == 0


def test_a_second_update_after_a_fused_frame(pair):
    rng = np.random.default_rng(10)
    p = pair(chunk_dims=(8, 8, 8))
    sensor = (4.5, 4.5, 4.5)
    ends = rng.normal(size=(400, 3))
    ends = (np.array(sensor) + 14.0 * ends / np.linalg.norm(ends, axis=1, keepdims=True)).astype(np.float32)

    def from_export():
        chunks, cells = p.gpu.export()
        p.ref.chunks = {tuple(int(v) for v in ch["c"]): ("chunk", int(ch["record"])) if ch["state"] == R.FOUND_IN_CHUNK
                        else ("cells", cells[int(ch["first_cell"]) // 512].copy()) for ch in chunks}
    for frame in range(2):
        p.gpu.fuse_rays(sensor, ends[200 * frame:200 * frame + 200], 20.0)
        assert p.gpu.components_info()[2] is False
        from_export()
        counts = p.update_both("frame %d" % frame)
        assert counts[1] > counts[0] >= 2                                      # never-seen cells of live chunks stand apart from the carved ones


def test_a_window_carries_the_labels(pair):
    rng = np.random.default_rng(11)
    p = pair(chunk_dims=(3, 2, 5))
    mixed_scene(p, rng, block((2, 2, 2)))
    p.update(APART, "window")
    for lower, shape in (((-3, -2, -5), (6, 4, 10)), ((-4, -3, -6), (8, 6, 12)), ((-1, 0, -2), (3, 1, 6))):
        rec, _ = p.gpu.extract_window(lower, shape)
        want = p.ref.window(lower, shape)
        assert np.array_equal(rec, want)
    inside = p.gpu.extract_window((-3, -2, -5), (6, 4, 10))[0] >> np.uint64(32)
    assert inside.min() >= 1 and inside.max() == p.gpu.components_info()[0]     # (every cell of the eight chunks is a node)


# ---- red zones ---------------------------------------------------------------------------------------------------------------------------------
def core_cases_on(ctx):
    made = []

    def make(**kw):
        kw.setdefault("default", DEFAULT)
        made.append(ComponentsPair(ctx, **kw))
        return made[-1]
    try:
        for dims in [(1, 1, 1), (3, 2, 5), (20, 20, 41), (3, 1, 2731)]:
            test_a_mixed_scene_of_each_chunk_shape_under_both_rules(make, dims)
        test_all_four_state_pairs_along_all_three_axes(make)
        test_chunks_at_both_ends_of_the_key_range(make)
        test_an_empty_map_and_a_map_of_one_chunk_filled_chunk(make)
        test_a_checkerboard_has_as_many_components_as_nodes(make)
    finally:
        for p in made:
            p.close()


def test_the_core_cases_in_a_child_process_with_red_zones_from_the_environment():
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from sdf_tools_amd import capi\nimport test_gpu_dsh_components as T\n"
            "ctx = capi.SdfGpu(0)\nT.core_cases_on(ctx)\nctx.redzone_check()\nctx.close()\nprint('core cases clean')\n") % (tests, os.path.dirname(tests))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SDFGPU_REDZONE="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "core cases clean" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
