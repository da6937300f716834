"""GPU: removal from the dynamic spatial hashed map (sdfgpu_dsh_remove_chunks*, sdfgpu_dsh_retain_box, sdfgpu_dsh_shrink;
include/sdfgpu.h "Removal") against the restatement of its contract (tests/dsh_remove_restated.py): the full
export, Get at probe locations and the counts compared as bytes after every step, no cell excused.

Which pool slot a chunk lives in is not visible through the interface, but a batch of ONE new chunk takes slot n_live: the pattern
tests build their maps one chunk per batch, so that chunk k lives in slot k and a pattern of slots can be named."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dsh_fusion_restated as F
import dsh_rays_restated as RR
import dsh_remove_restated as X
import dsh_restated as R
from sdf_tools_amd import capi
from test_gpu_dsh import NAN_A, SHAPES, VALUES, Pair
from test_gpu_dsh_rays import FRAMES, to_world

pytestmark = pytest.mark.gpu

DEFAULT = R.record(0.5, 0xABCD)                                              # unknown: a fused frame can move it both ways
POISON, POISON_CELL = R.record_bits(0x7FC0DEAD, 0xDEADDEAD), R.record_bits(0xFFC0BEEF, 0xBEEFBEEF)   # what a freed slot is left holding
FREE, HIT = R.record(0.0, 1), R.record(1.0, 2)
HELD = ("capacity_chunks", "table_capacity", "bytes_held", "byte_limit")


class RemovePair(Pair):
    """the map on the GPU and its restatement, driven together through removals (and the frames that reuse what they free)"""

    def __init__(self, ctx, default=DEFAULT, **kw):
        Pair.__init__(self, ctx, default=default, **kw)

    def remove_chunks(self, loc, what=""):
        held = self.held()
        got, removed = self.gpu.remove_chunks(loc)
        want = X.remove_chunks(self.ref, loc)
        assert np.array_equal(got, want), what + ": removal statuses"
        assert removed == int(want.sum()), what + ": removed count"
        assert self.held() == held, what + ": a removal changed what the map holds"
        return want

    def retain_box(self, lower, extent, invert=False, what=""):
        held = self.held()
        got = self.gpu.retain_box(lower, extent, invert)
        want = X.retain_box(self.ref, lower, extent, invert)
        assert got == want, "%s: %d chunks removed, the restatement removes %d" % (what, got, want)
        assert self.held() == held, what + ": a removal changed what the map holds"
        return want

    def insert_rays(self, sensor, points, max_range, what=""):
        st, counts = self.gpu.insert_rays(sensor, points, max_range, FREE, HIT)
        want_st, want_counts = RR.insert_rays(self.ref, sensor, points, max_range, FREE, HIT)
        assert np.array_equal(st, want_st) and counts == want_counts, what + ": carved frame"

    def fuse_rays(self, sensor, points, max_range, what=""):
        st, counts = self.gpu.fuse_rays(sensor, points, max_range, None)
        want_st, want_counts = F.fuse_rays(self.ref, sensor, points, max_range, None)
        assert np.array_equal(st, want_st) and counts == want_counts, what + ": fused frame"

    def held(self):
        info = self.gpu.info()
        return tuple(info[k] for k in HELD)


@pytest.fixture
def pair(gpu):
    made = []

    def make(**kw):
        made.append(RemovePair(gpu, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


def lattice(rng, count, half=12):
    """`count` distinct chunk coordinates around the origin, negative ones among them, in a random order"""
    side = np.arange(-half, half)
    c = np.stack(np.meshgrid(side, side, side, indexing="ij"), -1).reshape(-1, 3)
    return c[rng.permutation(len(c))[:count]]


def inside(p, chunks, rng, origin=np.eye(4), cell=1.0):
    """a location inside each chunk (a cell centre), in world coordinates"""
    n = np.array(p.ref.n)
    return to_world(origin, np.asarray(chunks) * n + rng.integers(0, n, (len(chunks), 3)) + 0.5, cell)


def build_in_slot_order(p, loc, rng):
    """one chunk per batch: chunk k takes pool slot k.  Every third is chunk-filled, the others cell-filled (one cell written)"""
    values = rng.integers(1, 1 << 63, len(loc), dtype=np.uint64)
    for k in range(len(loc)):
        if k % 3 == 0:
            assert p.gpu.set_chunks(loc[k:k + 1], values[k:k + 1], statuses=False) is None
            p.ref.set_chunk(loc[k], values[k])
        else:
            assert p.gpu.set_cells(loc[k:k + 1], values[k:k + 1], statuses=False) is None
            p.ref.set_cell(loc[k], values[k])


# ---- patterns of slots ---------------------------------------------------------------------------------------------------------------------
def slots_of(pattern, n, rng):
    """the slots a pattern removes from a map of n chunks in slots 0 .. n - 1"""
    if pattern == "all":
        return np.arange(n)
    if pattern == "tail":                                                      # the survivors are where they must be: no moves
        return np.arange(n - max(1, n // 3), n)
    if pattern == "head":                                                      # more removed than kept, all in front: every survivor moves
        return np.arange(max(1, (2 * n + 2) // 3))
    if pattern == "alternating":
        return np.arange(0, n, 2)
    if pattern == "keep-holes":                                                # every slot below `keep` is a hole
        keep = n // 2
        return np.concatenate([np.arange(keep), np.arange(2 * keep, n)])
    assert pattern == "half"
    return np.sort(rng.permutation(n)[:(n + 1) // 2])


COUNTS = [1, 2, 255, 256, 257, 513, 8000]
PATTERNS = ["none", "all", "tail", "head", "alternating", "keep-holes", "half"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("count", COUNTS)
def test_patterns_of_removed_slots(pair, count, pattern):
    """8 000 chunks cross the pairing scan's tiles (4 096 slots) and start from a 16-entry table and a one-chunk pool"""
    dims = (3, 2, 5) if count % 2 else (4, 4, 4)                               # 30 cells: no 16-byte path; 64 cells: the 16-byte path
    p = pair(chunk_dims=dims, initial_chunks=1)
    assert p.gpu.info()["table_capacity"] == 16 and p.gpu.info()["capacity_chunks"] == 1
    rng = np.random.default_rng(1000 * count + PATTERNS.index(pattern))
    chunks = lattice(rng, count + 3)
    loc = inside(p, chunks, rng)
    loc, absent = loc[:count], loc[count:]
    build_in_slot_order(p, loc, rng)
    before = p.check("built")
    probes = np.concatenate([loc, absent])
    if pattern == "none":
        exported = p.gpu.export()
        st = p.remove_chunks(np.concatenate([absent, [[np.nan, 0, 0]]]), "remove none")
        same = [k for k in before if k != "scratch_bytes"]                     # (the call's scratch is kept between calls)
        assert not st.any() and [p.gpu.info()[k] for k in same] == [before[k] for k in same], "removing nothing must leave the map untouched, table_capacity included"
        after = p.gpu.export()
        assert np.array_equal(exported[0], after[0]) and np.array_equal(exported[1], after[1])
        p.check_get(probes)
        return
    gone = slots_of(pattern, count, rng)
    st = p.remove_chunks(inside(p, chunks[gone], rng)[rng.permutation(len(gone))], pattern)      # other cells of the chunks, in any order
    assert st.all() and len(p.ref.chunks) == count - len(gone)
    p.check(pattern)
    p.check_get(probes, pattern)                                               # every kept chunk is still found, every removed one is not
    # the freed slots are drawn again: cell sets into three removed chunks and into new ones, then a second removal
    again = np.concatenate([loc[gone[:3]], absent])
    p.set_cells(again, VALUES[:len(again)])
    p.check(pattern + ", slots reused")
    live = np.array(sorted(p.ref.chunks))
    second = live[rng.permutation(len(live))[:(len(live) + 2) // 3]]
    assert p.remove_chunks(inside(p, second, rng), pattern + ", second removal").all()
    p.check(pattern + ", second removal")
    p.check_get(probes, pattern + ", second removal")


# ---- shapes and frames; what a freed slot leaves behind ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_freed_slots_are_reused_clean_in_every_chunk_shape(pair, dims, frame):
    """Every chunk's cells are poisoned before it is removed, so whatever a freed slot still holds is poison: a chunk made in such a
    slot by SetCell, SetChunk, a carved frame or a fused frame must show the default (or the chunk's record) in its other cells."""
    origin, inverse, cell = FRAMES[frame]
    p = pair(inverse=inverse, cell_size=cell, chunk_dims=dims)
    rng = np.random.default_rng(7)
    n = np.array(dims)
    side = [np.arange(-2, 2), np.arange(-2, 2), np.arange(-1, 2)]
    chunks = np.stack(np.meshgrid(*side, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(48)]
    loc = inside(p, chunks, rng, origin, cell)
    p.set_chunks(loc, POISON)
    p.set_cells(loc[:40], POISON_CELL)                                         # 40 cell-filled chunks of poison, 8 chunk-filled
    p.check("poisoned")
    # by box: the half x < 0 goes (24 chunks, both states among them and among the movers)
    lower, extent = (n * [-2, -2, -1]).tolist(), (n * [2, 4, 3]).tolist()
    assert p.retain_box(lower, extent, invert=True, what="half the block") == 24
    p.check("half the block removed")
    p.check_get(loc)
    gone = chunks[chunks[:, 0] < 0]
    a, b, c = inside(p, gone[:3], rng, origin, cell)
    p.set_cells([a], VALUES[0])                                                # a fresh cell-filled chunk: the default beside the cell
    p.set_chunks([b], VALUES[1])
    p.set_cells([b, c, c], VALUES[2:5])                                        # the chunk's record beside the cell; the last write wins
    p.check("SetCell and SetChunk into removed chunks")
    reach = 3.0 * float(n.min()) + 2.0
    sensor = to_world(origin, (-n[0] - 0.5, 0.5, 0.5), cell)[0]                  # inside the removed half
    d = rng.normal(size=(60, 3))
    ends = to_world(origin, np.array([-n[0] - 0.5, 0.5, 0.5]) + d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(1.0, reach, (60, 1)), cell).astype(np.float32)
    p.insert_rays(sensor, ends, reach * 0.8 * cell, "a carved frame through freed slots")
    p.check("carved frame")
    assert p.retain_box(lower, extent, invert=True, what="the half again") > 0
    p.check("the half removed again")
    p.fuse_rays(sensor, ends, reach * 0.8 * cell, "a fused frame through freed slots")
    p.check("fused frame")
    p.fuse_rays(sensor, ends[::2], reach * cell, "a second fused frame")     # the marks were left clean, no touched flag is stale
    p.check("second fused frame")
    live = np.array(sorted(p.ref.chunks))
    assert p.remove_chunks(inside(p, live[::2], rng, origin, cell), "by list behind the frames").all()
    p.check("by list behind the frames")
    p.fuse_rays(sensor, ends[1::2], reach * cell, "a third fused frame")
    p.check("third fused frame")
    p.check_get(np.concatenate([loc, ends.astype(np.float64)]))
    lower_w = (-2 * n - 1).tolist()
    shape = tuple(int(v) for v in np.minimum(4 * n + 2, [12, 12, 40]))
    rec, bits = p.gpu.extract_window(lower_w, shape, True)
    assert np.array_equal(rec, p.ref.window(lower_w, shape)) and np.array_equal(bits, R.pack_bits(R.classify(rec, True)))


# ---- by list -------------------------------------------------------------------------------------------------------------------------------
def test_duplicates_absent_and_invalid_locations_inside_one_list(pair):
    p = pair(chunk_dims=(3, 2, 5))
    at = lambda k, l=0: (3.0 * k + 0.5 + l, 0.5, 0.5)
    p.set_cells([at(k) for k in range(6)], VALUES[:6])
    p.set_chunks([at(k) for k in range(6, 10)], VALUES[:4])
    far = float(1 << 20) * 3
    loc = [at(2), at(2, 1), (np.nan, 0, 0), at(50), at(7), (far, 0, 0), at(7, 2), at(2), (0, -np.inf, 0), at(-1), at(9)]
    st = p.remove_chunks(loc, "mixed list")
    assert st.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1]
    p.check("mixed list")
    p.check_get([at(k, l) for k in range(-2, 12) for l in (0, 2)])
    # no operation; no statuses asked for (host and device form)
    held = p.gpu.info()
    assert p.gpu.remove_chunks(np.zeros((0, 3)))[1] == 0 and p.gpu.info() == held
    st, removed = p.gpu.remove_chunks([at(0), at(0), at(60)], statuses=False)
    X.remove_chunks(p.ref, [at(0)])
    assert st is None and removed == 1
    p.check("no statuses")
    d = torch.from_numpy(np.array([at(1), at(1, 1), at(3)], np.float64)).cuda()
    assert p.gpu.remove_chunks_device(d.data_ptr(), 3) == 2 and p.gpu.remove_chunks_device(d.data_ptr(), 0) == 0
    X.remove_chunks(p.ref, [at(1), at(3)])
    p.check("device form without statuses")
    d_st = torch.full((3,), 7, dtype=torch.uint8, device="cuda")
    d = torch.from_numpy(np.array([at(4), at(1), at(4)], np.float64)).cuda()
    assert p.gpu.remove_chunks_device(d.data_ptr(), 3, d_st.data_ptr()) == 1 and d_st.cpu().tolist() == [1, 0, 0]
    X.remove_chunks(p.ref, [at(4)])
    p.check("device form")
    with pytest.raises(capi.SdfGpuError) as e:
        p.gpu.remove_chunks_device(d.data_ptr(), -1)
    assert e.value.code == -1
    p.check("refused")


def test_seventy_thousand_removals_that_name_five_chunks(pair):
    p = pair(chunk_dims=(4, 4, 4))
    rng = np.random.default_rng(3)
    chunks = np.array([(0, 0, 0), (-1, 0, 0), (5, -7, 2), (0, 1, 0), (-3, -3, -3), (2, 2, 2), (1, 0, 0)])
    p.set_cells(inside(p, chunks, rng), VALUES[:7])
    named = np.repeat(np.arange(5), 14000)[rng.permutation(70000)]
    loc = (chunks[named] * 4 + rng.integers(0, 4, (70000, 3)) + rng.random((70000, 3)) * 0.98 + 0.01).astype(np.float64)
    st = p.remove_chunks(loc, "70 000 operations")
    first = [int(np.argmax(named == k)) for k in range(5)]
    assert sorted(np.flatnonzero(st).tolist()) == sorted(first), "only the first operation in list order that names a chunk removes it"
    info = p.check("70 000 operations")
    assert info["cell_filled"] == 2


# ---- by box --------------------------------------------------------------------------------------------------------------------------------
def test_boxes_whose_faces_cut_chunks_by_one_cell(pair):
    dims = (3, 2, 5)
    p = pair(chunk_dims=dims)
    rng = np.random.default_rng(9)
    side = np.arange(-3, 4)
    chunks = np.stack(np.meshgrid(side, side, side, indexing="ij"), -1).reshape(-1, 3)
    loc = inside(p, chunks, rng)
    values = rng.integers(1, 1 << 63, len(loc), dtype=np.uint64)

    def refill():
        p.set_chunks(loc, values)
        p.set_cells(loc[::2], values[::2])
    cases = []
    for a in range(3):
        s = dims[a]
        for lower_a, extent_a in [(0, s), (-1, s + 1), (0, s + 1), (-1, s + 2), (s - 1, 1), (s, 1), (-1, 1), (-s, s), (-s - 1, 2), (-2 * s + 1, 4 * s - 2)]:
            lower, extent = [-d for d in dims], [2 * d for d in dims]
            lower[a], extent[a] = lower_a, extent_a
            cases.append((lower, extent))
    cases += [([-4, -3, 2], [9, 4, 1]), ([1, 1, 1], [1, 1, 1]), ([-100, -100, -100], [200, 200, 200]), ([-9, -6, -15], [18, 12, 30])]
    assert len(cases) == 34                                                    # even cases retain, odd ones remove: the box over everything retains
    counts = set()
    for k, (lower, extent) in enumerate(cases):
        refill()
        removed = p.retain_box(lower, extent, invert=bool(k % 2), what="box %s + %s" % (lower, extent))
        p.check("box %s + %s" % (lower, extent))
        counts.add(removed)
        if k % 5 == 0:
            p.check_get(loc)
    assert len(counts) > 8 and 0 in counts and 216 in counts
    p.check_get(loc)


def test_empty_boxes_boxes_beyond_the_key_range_and_the_refusals(pair):
    p = pair(chunk_dims=(4, 4, 4))
    rng = np.random.default_rng(13)
    chunks = lattice(rng, 300, 5)
    loc = inside(p, chunks, rng)
    edge = [((1 << 20) * 4 - 0.5, 0.5, 0.5), (-(1 << 20) * 4 + 0.5, 0.5, 0.5)]    # chunks at the two ends of the key range along x
    p.set_cells(loc, NAN_A)
    p.set_chunks(edge, VALUES[:2])
    big = 1 << 40
    for extent in [(0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)]:
        assert p.retain_box((0, 0, 0), extent, invert=True) == 0
    assert p.retain_box((big - 8, 0, 0), (8, 4, 4), invert=True) == 0       # cells whose chunks lie beyond the key range
    assert p.retain_box((-big, -big, -big), (2 * 20, big, big), invert=True) == 0
    assert 0 < p.retain_box((-big, -big, -big), (big, big, big)) < 302
    p.check("the octant below the origin kept")
    p.set_cells(loc, NAN_A)
    p.set_chunks(edge, VALUES[:2])
    assert p.retain_box((-big, 0, 0), (big, 1, 1), invert=True) == 1 + sum(1 for c in chunks if c[0] < 0 and c[1] == 0 and c[2] == 0)
    assert p.gpu.get(edge)[1].tolist() == [1, 0]
    before, exported = p.check("before the refusals"), p.gpu.export()
    for lower, extent in [((big + 1, 0, 0), (1, 1, 1)), ((0, -big - 1, 0), (1, 1, 1)), ((0, 0, 0), (1, -1, 1)), ((0, 0, 0), (1, 1, big + 1)),
                          ((0, 0, -(1 << 62)), (4, 4, 4)), ((0, 0, 0), ((1 << 62), 4, 4))]:
        for invert in (False, True):
            assert not X.box_ok(lower, extent)
            with pytest.raises(capi.SdfGpuError) as e:
                p.gpu.retain_box(lower, extent, invert)
            assert e.value.code == -1 and "2^40" in str(e.value)
    after = p.gpu.export()
    assert p.check("refused") == before and np.array_equal(exported[0], after[0]) and np.array_equal(exported[1], after[1])
    live = len(p.ref.chunks)
    assert p.retain_box((0, 0, 0), (4, 0, 4)) == live > 200                   # the empty box retains nothing
    assert p.gpu.clear() == 0 and not p.ref.chunks
    info = p.check("cleared")
    assert info["chunk_filled"] + info["cell_filled"] == 0 and p.held() == tuple(before[k] for k in HELD)
    p.set_cells(loc[:5], VALUES[:5])                                           # an emptied map takes chunks again
    p.check("five chunks after the clear")
    assert p.gpu.remove_box((-big, -big, -big), (big, big, big)) == X.retain_box(p.ref, (-big, -big, -big), (big, big, big), True)
    p.check("remove_box")


# ---- the byte limit ----------------------------------------------------------------------------------------------------------------------
def test_a_map_at_its_byte_limit_takes_frames_again_after_retain_box(pair):
    dims, cpc = (4, 4, 4), 64
    limit = 32 * 12 + 8 * (24 + 8 * cpc)                                    # a table of 32 entries and a pool of 8 chunks
    p = pair(chunk_dims=dims, initial_chunks=4, byte_limit=limit)
    at = lambda k: (4.0 * k + 0.5, 0.5, 0.5)
    p.set_cells([at(k) for k in range(4)], VALUES[:4])
    p.set_chunks([at(k) for k in range(4, 8)], VALUES[4:8])
    full = p.check("eight chunks")
    assert full["capacity_chunks"] == 8 and full["bytes_held"] <= limit

    def frame(k):
        """one ray from chunk k - 1 into chunk k, fused"""
        return np.array(at(k - 1)) + (2.0, 0, 0), np.array([at(k)], np.float32), 6.0
    for call in (lambda: p.gpu.fuse_rays(*frame(8)), lambda: p.gpu.set_cells([at(8)], VALUES[0])):
        with pytest.raises(capi.SdfGpuError) as e:
            call()
        assert e.value.code == -3 and "byte limit" in str(e.value)
        assert p.check("refused at the limit")["bytes_held"] <= limit
    p.check_get([at(k) for k in range(-1, 12)])
    # a region of four chunks around the sensor slides along x: every frame goes in, what lies behind is forgotten
    for k in range(8, 20):
        removed = p.retain_box((4 * (k - 3), 0, 0), (16, 4, 4), what="slide to %d" % k)
        assert removed == (5 if k == 8 else 1)                                 # chunks k - 3 .. k - 1 stay, chunk k comes with the frame
        p.fuse_rays(*frame(k), what="frame %d" % k)
        info = p.check("frame %d" % k)
        assert info["bytes_held"] <= limit and info["capacity_chunks"] == 8 and info["chunk_filled"] + info["cell_filled"] == 4
    assert p.gpu.get([at(k) for k in range(0, 16)])[1].tolist() == [0] * 16  # behind the sensor: NOT_FOUND


# ---- shrink --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spare", [0, 10])
def test_shrink_after_removing_7900_of_8000_chunks(pair, spare):
    dims, cpc = (3, 2, 5), 30
    p = pair(chunk_dims=dims, initial_chunks=1)
    rng = np.random.default_rng(17)
    chunks = lattice(rng, 8400)
    loc = inside(p, chunks, rng)
    p.set_chunks(loc[:8000], rng.integers(1, 1 << 63, 8000, dtype=np.uint64))
    p.set_cells(loc[:8000:2], rng.integers(1, 1 << 63, 4000, dtype=np.uint64))
    # a frame whose rays stay inside chunk 0 (it adds no chunk)
    corner = chunks[0] * np.array(dims)
    sensor, ends = corner + (1.5, 0.5, 2.5), (corner + np.array([(1.5, 0.5, 0.5), (1.5, 0.5, 4.5), (1.5, 1.5, 2.5), (2.5, 0.5, 2.5)])).astype(np.float32)
    p.fuse_rays(sensor, ends, 20.0, "a fused frame makes the mark plane")
    grown = p.check("8 000 chunks and a frame")
    assert grown["chunk_filled"] + grown["cell_filled"] == 8000 and grown["scratch_bytes"] >= grown["capacity_chunks"] * cpc
    keep = np.concatenate([[0], 1 + rng.permutation(7999)[:99]])
    gone = np.setdiff1d(np.arange(8000), keep)
    assert p.remove_chunks(loc[gone], "7 900 removed").sum() == 7900
    live = 100
    before = p.check("a hundred left")
    assert p.held() == tuple(grown[k] for k in HELD) and before["chunk_filled"] + before["cell_filled"] == live
    exported = p.gpu.export()
    p.gpu.shrink(spare)
    plan = X.shrink_plan(live, spare, before["capacity_chunks"], before["table_capacity"], cpc)
    info = p.check("shrunk")
    assert (info["capacity_chunks"], info["table_capacity"], info["bytes_held"]) == plan
    assert plan[:2] == (live + spare, 256)
    assert info["scratch_bytes"] == before["scratch_bytes"] - before["capacity_chunks"] * cpc, "the mark plane must be freed"
    after = p.gpu.export()
    assert np.array_equal(exported[0], after[0]) and np.array_equal(exported[1], after[1]), "shrink changed the content"
    p.check_get(loc[:8000:7])
    p.gpu.shrink(spare)                                                        # already tight: nothing changes
    assert p.gpu.info() == info
    p.gpu.shrink(spare + 1000000)                                              # only ever downwards
    assert p.gpu.info() == info
    p.set_cells(loc[8000:8300], VALUES[3])                                     # a following batch grows the pool again
    more = p.check("300 more chunks")
    assert more["capacity_chunks"] >= live + 300 > info["capacity_chunks"]
    p.fuse_rays(sensor, ends, 20.0, "a fused frame makes the mark plane again")
    last = p.check("fused after the shrink")
    assert last["scratch_bytes"] >= last["capacity_chunks"] * cpc
    p.fuse_rays(sensor, ends[::3], 20.0, "and again")
    p.check("fused twice after the shrink")
    with pytest.raises(capi.SdfGpuError) as e:
        p.gpu.shrink(-1)
    assert e.value.code == -1


def test_shrink_on_an_empty_map_and_a_fresh_one(pair):
    p = pair(chunk_dims=(8, 8, 32))
    p.gpu.shrink(64)
    assert p.held()[:2] == (64, 128)                                           # as created: nothing is smaller
    p.set_cells([(0.5, 0.5, 0.5), (8.5, 0.5, 0.5)], VALUES[:2])
    p.gpu.shrink()
    assert p.held()[:3] == (2, 16, 16 * 12 + 2 * (24 + 8 * 2048))
    p.check("two chunks, tight")
    assert p.gpu.clear() == 2
    X.retain_box(p.ref, (0, 0, 0), (0, 0, 0))
    p.gpu.shrink()
    assert p.held()[:3] == (1, 16, 16 * 12 + 1 * (24 + 8 * 2048))
    p.set_cells([(0.5, 0.5, 0.5), (8.5, 0.5, 0.5), (16.5, 0.5, 0.5)], VALUES[:3])
    p.check("three chunks after the shrink to one")


# ---- red zones -------------------------------------------------------------------------------------------------------------------------
def core_cases_on(ctx):
    made = []

    def make(**kw):
        made.append(RemovePair(ctx, **kw))
        return made[-1]
    try:
        test_patterns_of_removed_slots(make, 257, "alternating")
        test_patterns_of_removed_slots(make, 256, "head")
        test_freed_slots_are_reused_clean_in_every_chunk_shape(make, (3, 2, 5), "rotated-quarter")
        test_freed_slots_are_reused_clean_in_every_chunk_shape(make, (8, 8, 32), "identity")
        test_duplicates_absent_and_invalid_locations_inside_one_list(make)
        test_boxes_whose_faces_cut_chunks_by_one_cell(make)
        test_a_map_at_its_byte_limit_takes_frames_again_after_retain_box(make)
        test_shrink_after_removing_7900_of_8000_chunks(make, 10)
        test_shrink_on_an_empty_map_and_a_fresh_one(make)
    finally:
        for p in made:
            p.close()


def test_one_removal_of_each_kind_in_a_child_process_with_red_zones_from_the_environment():
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from sdf_tools_amd import capi\nimport test_gpu_dsh_remove as T\n"
            "ctx = capi.SdfGpu(0)\nT.core_cases_on(ctx)\nctx.redzone_check()\nctx.close()\nprint('core cases clean')\n") % (tests, os.path.dirname(tests))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SDFGPU_REDZONE="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "core cases clean" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
