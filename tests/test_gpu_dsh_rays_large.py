"""GPU: a frame of sensor rays into a dynamic spatial hashed map past 2^31 cells: 65 536 live chunks of 32^3
cells hold slots 0 .. 65 535 of the pool, so every chunk the frame makes takes a slot from 65 536 on, whose cells start at cell 2^31
and byte 2^34 of the pool.  Checked by Get on every cell the restatement's walks name and on a sample of cells no ray touched, not by
a full export.  About 18 GB of device memory."""
import numpy as np
import pytest

import dsh_restated as R
import dsh_rays_restated as RR
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

DEFAULT, FREE, HIT = R.record(0.5, 0x55), R.record(0.0, 0x10), R.record(1.0, 0x20)


def test_rays_into_chunks_past_two_to_the_31_cells(gpu):
    dims, cpc = (32, 32, 32), 32768
    first = np.stack(np.meshgrid(np.arange(64), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 3)          # 65 536 chunks
    assert len(first) * cpc == 1 << 31 and len(first) * cpc * 8 == 1 << 34
    rng = np.random.default_rng(36)
    values = rng.integers(1, 1 << 63, len(first), dtype=np.uint64)
    centres = first * 32 + 16.0
    room = 256
    m = gpu.dsh_create(None, 1.0, dims, DEFAULT, initial_chunks=len(first) + room)
    ref = R.Map(None, 1.0, dims, DEFAULT)
    try:
        assert (m.set_chunks(centres, values) == capi.DSH_SET_CHUNK).all()
        near = np.flatnonzero((first <= 3).all(axis=1))                      # the chunk-filled chunks the frame and the samples can reach
        assert len(near) == 64
        for k in near:
            ref.set_chunk(centres[k], values[k])
        # a sensor in absent space beside chunk (0, 0, 0): the rays make chunks at negative coordinates and turn chunk-filled ones into cells
        sensor = (-20.5, 10.5, 10.5)
        d = rng.normal(size=(400, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        pts = (np.asarray(sensor) + d * rng.uniform(3.0, 75.0, (400, 1))).astype(np.float32)
        _, carved, hits = RR.frame(ref, sensor, pts, 60.0)
        named = sorted({c for cells in carved for c in cells} | {h for h in hits if h is not None})
        assert len(named) > 10000
        st, counts = m.insert_rays(sensor, pts, 60.0, FREE, HIT)
        want_st, want_counts = RR.insert_rays(ref, sensor, pts, 60.0, FREE, HIT)
        assert np.array_equal(st, want_st) and counts == want_counts
        assert counts["new_chunks"] >= 8 and counts["rays_truncated"] > 20 and counts["rays_hit"] > 100
        info = m.info()
        cells_now = sum(k == "cells" for k, _ in ref.chunks.values())
        assert cells_now > counts["new_chunks"], "no chunk-filled chunk was crossed"
        assert (info["chunk_filled"], info["cell_filled"]) == (len(first) - (cells_now - counts["new_chunks"]), cells_now)
        assert info["capacity_chunks"] == len(first) + room, "the pool grew: the new chunks' slots are not where the test wants them"
        assert info["bytes_held"] > 1 << 34
        # every cell the walks name, then cells no ray touched: in the new chunks, in the chunks that turned into cells, in absent space
        loc = np.asarray(named, np.float64) + 0.5
        rec, status = m.get(loc)
        want_rec, want_status = ref.get_batch(loc)
        assert np.array_equal(status, want_status) and (status == capi.DSH_FOUND_IN_CELL).all() and np.array_equal(rec, want_rec)
        assert set(np.unique(rec).tolist()) == {FREE, HIT}
        sample = rng.integers(-100, 100, (6000, 3)).astype(np.float64) + 0.5
        rec, status = m.get(sample)
        want_rec, want_status = ref.get_batch(sample)
        assert np.array_equal(status, want_status) and np.array_equal(rec, want_rec)
        assert set(np.unique(status).tolist()) == {0, 1, 2} and DEFAULT in rec[status == 2].tolist()
        # a second frame from the other side sees through the first one's hits
        sensor2 = (25.5, 40.5, 12.5)
        st, counts = m.insert_rays(sensor2, pts, 200.0, HIT, FREE)
        want_st, want_counts = RR.insert_rays(ref, sensor2, pts, 200.0, HIT, FREE)
        assert np.array_equal(st, want_st) and counts == want_counts and counts["rays_truncated"] == 0
        rec, status = m.get(sample)
        want_rec, want_status = ref.get_batch(sample)
        assert np.array_equal(status, want_status) and np.array_equal(rec, want_rec)
    finally:
        m.close()
