"""GPU: ray casts that read a dynamic spatial hashed map past 2^31 cells, in the setup of
tests/test_gpu_dsh_rays_large.py: 65 536 chunk-filled chunks of 32^3 cells hold slots 0 .. 65 535 of the pool, so the chunks that a
handful of cell sets make take slots from 65 536 on, whose cells start at cell 2^31 and byte 2^34 of the pool.  Rays whose blockers are
those cells, and rays that read the free cells around them, judged by the restatement.  About 18 GB of device memory."""
import numpy as np
import pytest

import dsh_cast_restated as C
import dsh_restated as R
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

DEFAULT, FILLED = R.record(0.0, 0x55), R.record(1.0, 0x20)


def test_casts_through_chunks_past_two_to_the_31_cells(gpu):
    dims, cpc = (32, 32, 32), 32768
    first = np.stack(np.meshgrid(np.arange(64), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 3)          # 65 536 chunks
    assert len(first) * cpc == 1 << 31
    rng = np.random.default_rng(336)
    values = rng.integers(1, 1 << 63, len(first), dtype=np.uint64)
    centres = first * 32 + 16.0
    room = 64
    m = gpu.dsh_create(None, 1.0, dims, DEFAULT, initial_chunks=len(first) + room)
    ref = R.Map(None, 1.0, dims, DEFAULT)
    try:
        assert (m.set_chunks(centres, values) == capi.DSH_SET_CHUNK).all()
        for k in np.flatnonzero((first <= 3).all(axis=1)):                     # the chunk-filled chunks the rays can reach
            ref.set_chunk(centres[k], values[k])
        # twelve filled cells in the absent space at negative x: eight fresh chunks at most, every one in a slot past 65 535
        targets = np.concatenate([rng.integers(-64, 0, (12, 1)), rng.integers(0, 64, (12, 2))], axis=1) + 0.5
        assert (m.set_cells(targets, FILLED) == capi.DSH_SET_CELL).all()
        ref.set_cells(targets, FILLED)
        info = m.info()
        fresh = sum(k == "cells" for k, _ in ref.chunks.values())
        assert 4 <= fresh == info["cell_filled"] and info["chunk_filled"] == len(first) and info["capacity_chunks"] == len(first) + room
        assert info["bytes_held"] > 1 << 34
        # segments through a target each (from anywhere in the fresh chunks to half as far again behind it), segments that read only
        # free cells there, and segments on into the chunk-filled chunks at positive x
        n = 600
        starts = np.concatenate([rng.uniform(-64, 0, (n, 1)), rng.uniform(0, 64, (n, 2))], axis=1)
        ends = starts + rng.uniform(-40, 40, (n, 3))
        through = targets[rng.integers(0, len(targets), n // 2)]
        ends[:n // 2] = starts[:n // 2] + 1.5 * (through - starts[:n // 2])
        ends[-100:, 0] = rng.uniform(5, 90, 100)
        for flags in (0, C.SKIP_FIRST | C.UNKNOWN_IS_FILLED):
            st, hits = m.cast_segments(starts, ends, 70.0, flags)
            want_st, want_hits = C.cast_segments(ref, starts, ends, 70.0, flags)
            assert np.array_equal(st, want_st) and hits.tobytes() == want_hits.tobytes()
            on_target = (st == C.CAST_BLOCKED) & (hits["found"] == R.FOUND_IN_CELL) & (hits["record"] == np.uint64(FILLED))
            assert on_target.sum() > 150, "blockers among the cells past 2^31"
            assert ((st != C.CAST_BLOCKED) & (hits["found"] == R.FOUND_IN_CELL) & (hits["record"] == np.uint64(DEFAULT))).sum() > 50, "free cells read past 2^31"
            assert (hits["found"][-100:] == R.FOUND_IN_CHUNK).sum() > 20
        sensor = (-30.5, 33.5, 31.5)
        pts = ends.astype(np.float32)
        st, hits = m.cast_rays(sensor, pts, 55.0, 0)
        want_st, want_hits = C.cast_rays(ref, sensor, pts, 55.0, 0)
        assert np.array_equal(st, want_st) and hits.tobytes() == want_hits.tobytes()
        assert set(np.unique(st).tolist()) == {C.CAST_CLEAR, C.CAST_CLEAR_IN_RANGE, C.CAST_BLOCKED}
        assert m.info() == dict(info, scratch_bytes=m.info()["scratch_bytes"])
    finally:
        m.close()
