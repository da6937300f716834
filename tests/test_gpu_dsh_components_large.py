"""GPU: the connected components of a dynamic spatial hashed map past 2^31 nodes, in the setup of
tests/test_gpu_dsh_large.py: 65 544 cell-filled chunks of 32^3 cells, N = 2 147 745 792 nodes, so node indices pass 2^31, the label
words' byte offsets 2^33 and the pool's 2^34.  The pattern needs no search to judge.  Every chunk starts uniform, filled where its
c_x is odd and free where it is even, which makes one slab per c_x.  The four chunks with the highest node bases, (63, 31, 28 .. 31),
then get free planes at every 4th local x: structure inside chunks, across their z faces and across the tiles of the local kernel
(x = 8, 16 and 24 start a tile of 8192 slots), all at node indices past 2^31.  The plane at x = 0 touches the free slab of c_x = 62
and joins it; the seven others are components of their own.  Two single cells of the other class, one in the first chunk of the
export order and one in the last, are components too.  K and every label follow in closed form.  (Planes through all 65 544 chunks
would take 537 M cell sets, 13 GB of locations: the four chunks take 32 768.)  About 27 GB of free device memory: the pool's
16 GiB, 8 GiB of label words and the rank tables."""
import numpy as np
import pytest

import dsh_restated as R
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

FREE, FILLED = R.record(0.0, 0x21), R.record(1.0, 0x20)
LOW = np.uint64(0xFFFFFFFF)


def test_slabs_and_planes_of_a_map_past_two_to_the_31_nodes(gpu):
    dims, cpc = (32, 32, 32), 32768
    first = np.stack(np.meshgrid(np.arange(64), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 3)          # 65 536 chunks
    last = np.stack(np.meshgrid([-2, -1], [-2, -1], [-2, -1], indexing="ij"), -1).reshape(-1, 3)                         # 8 more, in the highest slots
    chunks = np.concatenate([first, last])
    n = len(chunks)
    assert n == 65544 and n * cpc > 1 << 31
    planed = (chunks[:, 0] == 63) & (chunks[:, 1] == 31) & (chunks[:, 2] >= 28)
    assert planed.sum() == 4 and planed[65532:65536].all(), "the last four chunks of the export order: node bases from 2 147 614 720 on"
    rng = np.random.default_rng(12)
    local = rng.integers(0, 32, (n, 3))
    local[(local == 6).all(1)] = 7                                             # (6, 6, 6) is kept for the two single cells
    local[planed, 0] = 1                                                       # (off the planes)
    centre = lambda c, l: (c * 32 + l + 0.5).astype(np.float64)
    values = np.where(chunks[:, 0] % 2 == 1, np.uint64(FILLED), np.uint64(FREE))
    m = gpu.dsh_create(None, 1.0, dims, R.record(0.5, 0x55), initial_chunks=n)
    try:
        assert (m.set_chunks(centre(chunks, 16)[:65536], values[:65536]) == capi.DSH_SET_CHUNK).all()
        assert (m.set_chunks(centre(chunks, 16)[65536:], values[65536:]) == capi.DSH_SET_CHUNK).all()
        assert (m.set_cells(centre(chunks, local), values) == capi.DSH_SET_CELL).all()            # every chunk becomes cell-filled, still uniform
        yz = np.stack(np.meshgrid(np.arange(32), np.arange(32 * 28, 32 * 32), indexing="ij"), -1).reshape(-1, 2)          # y of c_y = 31, z of c_z = 28 .. 31
        planes = np.concatenate([np.column_stack([np.full(len(yz), 63 * 32 + x), 31 * 32 + yz[:, 0], yz[:, 1]]) for x in range(0, 32, 4)])
        assert len(planes) == 8 * 32 * 128
        assert (m.set_cells(planes + 0.5, FREE) == capi.DSH_SET_CELL).all()
        singles = np.array([[-2, -2, -2], [63, 31, 31]])                        # the first and the last chunk of the export order
        assert (m.set_cells(centre(singles, 6), [FILLED, FREE]) == capi.DSH_SET_CELL).all()   # (x = 6: between the planes at 4 and 8)
        info = m.info()
        assert (info["chunk_filled"], info["cell_filled"], info["capacity_chunks"]) == (0, n, n)
        # Export order: c_x = -2 (free; its single filled cell is the second component), c_x = -1, then c_x = 0 .. 63 as 4 .. 67.  The
        # planes' first nodes lie in chunk (63, 31, 28), behind every slab's: x = 4, 8, .. 28 are 68 .. 74, and the single free cell
        # of (63, 31, 31) starts the last component, 75.  The eight chunks below zero touch the others along an edge at most.
        label_of = lambda cx: np.where(cx == -2, 1, np.where(cx == -1, 3, cx + 4))
        for flags in (0, capi.DSH_COMPONENTS_UNKNOWN_APART):
            assert m.update_components(flags) == 75 and m.components_info() == (75, flags, True)
            rec, st = m.get(centre(chunks, local))
            assert (st == capi.DSH_FOUND_IN_CELL).all()
            assert np.array_equal(rec & LOW, values & LOW), "an occupancy changed"
            assert np.array_equal(rec >> np.uint64(32), label_of(chunks[:, 0]).astype(np.uint64)), "slab labels"
            rec, _ = m.get(centre(chunks, 0))                                  # every chunk's first cell, where the chunk's nodes start
            want = label_of(chunks[:, 0]).astype(np.uint64)
            want[planed] = 66                                                   # the plane at x = 0 belongs to the free slab of c_x = 62
            assert np.array_equal(rec >> np.uint64(32), want)
            rec, _ = m.get(planes + 0.5)                                        # every cell of every plane
            plane_label = np.where(planes[:, 0] == 63 * 32, 66, 67 + (planes[:, 0] - 63 * 32) // 4).astype(np.uint64)
            assert np.array_equal(rec & LOW, np.full(len(planes), FREE, np.uint64) & LOW) and np.array_equal(rec >> np.uint64(32), plane_label)
            rec, _ = m.get(planes + 0.5 + [1.0, 0.0, 0.0])                      # the filled cells beside them: all of the slab of c_x = 63
            assert np.array_equal(rec >> np.uint64(32), np.full(len(planes), 67, np.uint64))
            rec, _ = m.get(centre(singles, 6))
            assert rec.tolist() == [R.record(1.0, 2), R.record(0.0, 75)]
            rec, _ = m.get(centre(singles, 6) + [0.0, 0.0, 1.0])                 # their neighbours belong to the slabs
            assert rec.tolist() == [(FREE & 0xFFFFFFFF) | 1 << 32, (FILLED & 0xFFFFFFFF) | 67 << 32]
        after = m.info()
        assert after == dict(info, scratch_bytes=after["scratch_bytes"]) and after["scratch_bytes"] > n * cpc * 4
    finally:
        m.close()
