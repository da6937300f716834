"""GPU: the dynamic spatial hashed map past 2^31 cells: 65 544 chunks of 32^3 cells, every one turned into cells,
so that the pool's cell index passes 2^31 and its byte offset 2^34.  About 18 GB of device memory."""
import numpy as np
import pytest

import dsh_restated as R
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu


def test_a_pool_past_two_to_the_31_cells(gpu):
    dims, cpc = (32, 32, 32), 32768
    first = np.stack(np.meshgrid(np.arange(64), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 3)          # 65 536 chunks
    last = np.stack(np.meshgrid([-2, -1], [-2, -1], [-2, -1], indexing="ij"), -1).reshape(-1, 3)                         # 8 more
    chunks = np.concatenate([first, last])
    n = len(chunks)
    assert n == 65544 and len(first) * cpc == 1 << 31 and len(first) * cpc * 8 == 1 << 34
    rng = np.random.default_rng(11)
    chunk_values = rng.integers(1, 1 << 63, n, dtype=np.uint64)
    cell_values = rng.integers(1, 1 << 63, n, dtype=np.uint64)
    local = rng.integers(0, 32, (n, 3))
    other = (local + 1 + rng.integers(0, 31, (n, 3))) % 32                   # another cell of the same chunk
    centre = lambda l: (chunks * 32 + l + 0.5).astype(np.float64)
    m = gpu.dsh_create(None, 1.0, dims, R.record(0.0, 0x55), initial_chunks=n)
    ref = R.Map(None, 1.0, dims, R.record(0.0, 0x55))
    try:
        # the 65 536 chunks take slots 0 .. 65 535 in some order; the batch of 8 behind them takes the slots from 65 536 on, whose
        # cells start at index 2^31 and byte 2^34 of the pool
        assert (m.set_chunks(centre(other)[:65536], chunk_values[:65536]) == capi.DSH_SET_CHUNK).all()
        assert (m.set_chunks(centre(other)[65536:], chunk_values[65536:]) == capi.DSH_SET_CHUNK).all()
        info = m.info()
        assert (info["chunk_filled"], info["cell_filled"], info["capacity_chunks"]) == (n, 0, n)
        assert (m.set_cells(centre(local), cell_values) == capi.DSH_SET_CELL).all()
        info = m.info()
        assert (info["chunk_filled"], info["cell_filled"], info["capacity_chunks"]) == (0, n, n), "the pool grew or a chunk kept its state"
        assert info["bytes_held"] == info["table_capacity"] * 12 + n * (24 + 8 * cpc) > 1 << 34
        # Get in every chunk: the cell that was set, and another one, which keeps the chunk's record
        rec, st = m.get(centre(local))
        assert (st == capi.DSH_FOUND_IN_CELL).all() and np.array_equal(rec, cell_values)
        rec, st = m.get(centre(other))
        assert (st == capi.DSH_FOUND_IN_CELL).all() and np.array_equal(rec, chunk_values)
        # a window over the eight chunks in the highest slots (and absent chunks beside them), against the restatement of those eight
        for k in range(65536, n):
            ref.set_chunk(centre(other)[k], chunk_values[k])
            ref.set_cell(centre(local)[k], cell_values[k])
        lower, shape = (-35, -33, -34), (38, 3, 66)
        rec, bits = m.extract_window(lower, shape, True)
        want = ref.window(lower, shape)
        assert np.array_equal(rec, want) and np.array_equal(bits, R.pack_bits(R.classify(want, True)))
        assert len(np.unique(want)) >= 8
    finally:
        m.close()
