"""GPU: removal from the dynamic spatial hashed map past 2^31 cells, as tests/test_gpu_dsh_large.py builds it:
65 544 chunks of 32^3 cells, every one turned into cells.  The eight chunks of the last batch live in the slots from 65 536 on, whose
cells start at index 2^31 and byte 2^34 of the pool; removing eight chunks of the first batch makes them the movers, so the move
kernel's source offsets pass 2^34 bytes.  About 18 GB of device memory."""
import numpy as np
import pytest

import dsh_remove_restated as X
import dsh_restated as R
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu


def test_movers_from_slots_past_two_to_the_31_cells(gpu):
    dims, cpc = (32, 32, 32), 32768
    first = np.stack(np.meshgrid(np.arange(64), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 3)          # 65 536 chunks
    last = np.stack(np.meshgrid([-2, -1], [-2, -1], [-2, -1], indexing="ij"), -1).reshape(-1, 3)                         # 8 more
    chunks = np.concatenate([first, last])
    n = len(chunks)
    assert n == 65544 and len(first) * cpc == 1 << 31 and len(first) * cpc * 8 == 1 << 34
    rng = np.random.default_rng(12)
    chunk_values = rng.integers(1, 1 << 63, n, dtype=np.uint64)
    cell_values = rng.integers(1, 1 << 63, n, dtype=np.uint64)
    local = rng.integers(0, 32, (n, 3))
    other = (local + 1 + rng.integers(0, 31, (n, 3))) % 32                   # another cell of the same chunk
    centre = lambda l: (chunks * 32 + l + 0.5).astype(np.float64)
    m = gpu.dsh_create(None, 1.0, dims, R.record(0.0, 0x55), initial_chunks=n)
    ref = R.Map(None, 1.0, dims, R.record(0.0, 0x55))
    try:
        assert (m.set_chunks(centre(other)[:65536], chunk_values[:65536]) == capi.DSH_SET_CHUNK).all()
        assert (m.set_chunks(centre(other)[65536:], chunk_values[65536:]) == capi.DSH_SET_CHUNK).all()
        assert (m.set_cells(centre(local), cell_values) == capi.DSH_SET_CELL).all()
        held = m.info()
        assert (held["chunk_filled"], held["cell_filled"], held["capacity_chunks"]) == (0, n, n)
        # eight chunks of the first batch go: keep = 65 536, so every slot from 65 536 on is a mover, whichever eight slots are the holes
        gone = rng.permutation(65536)[:8]
        st, removed = m.remove_chunks(centre(other)[gone])
        assert st.tolist() == [1] * 8 and removed == 8
        info = m.info()
        assert (info["chunk_filled"], info["cell_filled"]) == (0, n - 8)
        assert all(info[k] == held[k] for k in ("capacity_chunks", "table_capacity", "bytes_held"))
        # the moved chunks: the cell that was set, and another one, which keeps the chunk's record; so does every chunk that stayed
        keep = np.setdiff1d(np.arange(n), gone)
        rec, st = m.get(centre(local)[keep])
        assert (st == capi.DSH_FOUND_IN_CELL).all() and np.array_equal(rec, cell_values[keep])
        rec, st = m.get(centre(other)[keep])
        assert (st == capi.DSH_FOUND_IN_CELL).all() and np.array_equal(rec, chunk_values[keep])
        rec, st = m.get(centre(local)[gone])
        assert (st == capi.DSH_NOT_FOUND).all() and (rec == np.uint64(R.record(0.0, 0x55))).all()
        # a window over the eight moved chunks (and absent chunks beside them), against the restatement of those eight
        for k in range(65536, n):
            ref.set_chunk(centre(other)[k], chunk_values[k])
            ref.set_cell(centre(local)[k], cell_values[k])
        lower, shape = (-35, -33, -34), (38, 3, 66)
        rec, bits = m.extract_window(lower, shape, True)
        want = ref.window(lower, shape)
        assert np.array_equal(rec, want) and np.array_equal(bits, R.pack_bits(R.classify(want, True)))
        assert len(np.unique(want)) >= 8
        # by box: everything with x >= 0 goes; the eight stay (now in slots 0 .. 7) and a cell set draws a freed slot again
        assert m.retain_box((-64, -64, -64), (64, 64, 64)) == X.retain_box(ref, (-64, -64, -64), (64, 64, 64)) + 65528
        info = m.info()
        assert (info["chunk_filled"], info["cell_filled"], info["capacity_chunks"]) == (0, 8, n)
        rec, bits = m.extract_window(lower, shape, True)
        assert np.array_equal(rec, want)
        assert m.set_cells(centre(local)[:1], cell_values[:1]).tolist() == [capi.DSH_SET_CELL]
        rec, st = m.get(np.concatenate([centre(local)[:1], centre(other)[:1]]))
        assert st.tolist() == [2, 2] and rec.tolist() == [int(cell_values[0]), R.record(0.0, 0x55)]
    finally:
        m.close()
