"""GPU: frontier cells read from a dynamic spatial hashed map past 2^31 cells, in the setup of
tests/test_gpu_dsh_large.py: 65 536 chunk-filled chunks of 32^3 cells hold slots 0 .. 65 535 of the pool, so the chunks that a handful
of cell sets make take slots from 65 536 on, whose cells start at cell 2^31 and byte 2^34 of the pool.  The frontier cells lie only in
those chunks; they are listed through a box and through a window of 1625^3 voxels (4 291 015 625, bits only), and the restatement
judges the boxed chunks only.  About 20 GB of free device memory: the pool's 16 GiB, the list form's masks of 4 KiB per live chunk
(268 MB) and the window's 536 MB of bits."""
import numpy as np
import pytest
import torch

import dsh_frontier_restated as F
import dsh_restated as R
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

DEFAULT, FILLED, FREE = R.record(0.5, 0x55), R.record(1.0, 0x20), R.record(0.0, 0x21)


def test_frontier_cells_in_chunks_past_two_to_the_31_cells(gpu):
    dims, cpc = (32, 32, 32), 32768
    first = np.stack(np.meshgrid(np.arange(64), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 3)          # 65 536 chunks
    assert len(first) * cpc == 1 << 31
    rng = np.random.default_rng(349)
    centres = first * 32 + 16.0
    room = 64
    m = gpu.dsh_create(None, 1.0, dims, DEFAULT, initial_chunks=len(first) + room)
    ref = R.Map(None, 1.0, dims, DEFAULT)
    try:
        # the first 65 536 slots: filled chunks, which hold no frontier cell and are unknown to nobody
        assert (m.set_chunks(centres, FILLED) == capi.DSH_SET_CHUNK).all()
        for k in np.flatnonzero(first[:, 0] == 0):                             # the filled chunks that touch the box below
            ref.set_chunk(centres[k], FILLED)
        # free cells in the absent (unknown) space at negative x: eight fresh chunks at most, every one in a slot past 65 535
        targets = np.concatenate([rng.integers(-64, 0, (400, 1)), rng.integers(0, 64, (400, 2))], axis=1)
        targets[:40, 0] = -1                                                   # some against the filled chunks' face
        assert (m.set_cells(targets + 0.5, FREE) == capi.DSH_SET_CELL).all()
        ref.set_cells(targets + 0.5, FREE)
        info = m.info()
        fresh = sum(k == "cells" for k, _ in ref.chunks.values())
        assert 4 <= fresh == info["cell_filled"] and info["chunk_filled"] == len(first) and info["capacity_chunks"] == len(first) + room
        assert info["bytes_held"] > 1 << 34
        box = ((-64, 0, 0), (64, 64, 64))
        lower, side = (-800, -780, -790), 1625
        assert side ** 3 == 4291015625 and all(lower[a] <= box[0][a] and box[0][a] + 64 <= lower[a] + side for a in range(3))
        d_bits = torch.empty((side ** 3 + 31) // 32, dtype=torch.int32, device="cuda")
        for flags in (0, capi.DSH_FRONTIER_26):
            want = F.frontier_cells(ref, box, flags)
            assert len(want) > 300
            got = m.frontier_cells(box[0], box[1], flags)
            assert got.tobytes() == want.tobytes()
            assert m.frontier_cells(None, None, flags).tobytes() == want.tobytes(), "the whole map holds no other frontier cell"
            m.frontier_window_device(lower, (side, side, side), flags, d_bits.data_ptr())
            torch.cuda.synchronize()
            assert int(torch.count_nonzero(d_bits)) <= len(want)
            v = ((want[:, 0] - lower[0]) * side + (want[:, 1] - lower[1])) * side + (want[:, 2] - lower[2])
            set_bits = torch.nonzero(d_bits).reshape(-1).cpu().numpy()          # the words that hold a bit
            back = d_bits[torch.from_numpy(set_bits).cuda()].cpu().numpy().view(np.uint32)
            listed = sorted(int(w) * 32 + b for w, word in zip(set_bits, back) for b in range(32) if (int(word) >> b) & 1)
            assert listed == sorted(int(x) for x in v), "popcount and set bits of the window equal the list"
        assert m.info() == dict(info, scratch_bytes=m.info()["scratch_bytes"])
    finally:
        m.close()
