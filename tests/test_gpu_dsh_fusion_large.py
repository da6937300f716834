"""GPU: a fused frame of sensor rays into a dynamic spatial hashed map past 2^31 cells: 65 536 live chunks of
32^3 cells hold slots 0 .. 65 535 of the pool, so every chunk the frame makes takes a slot from 65 536 on, whose cells start at cell
2^31 of the pool and whose marks start at byte 2^31 of the mark plane.  Checked by Get on every cell the restatement's walks name and
on a sample of cells no ray touched, not by a full export.  About 20 GB of device memory (the pool's 17 GB and 2 GB of marks)."""
import numpy as np
import pytest

import dsh_restated as R
import dsh_rays_restated as RR
import dsh_fusion_restated as F
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

DEFAULT = R.record(0.5, 0x55)


def test_fused_rays_into_chunks_past_two_to_the_31_cells(gpu):
    dims, cpc = (32, 32, 32), 32768
    first = np.stack(np.meshgrid(np.arange(64), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 3)          # 65 536 chunks
    assert len(first) * cpc == 1 << 31
    rng = np.random.default_rng(49)
    values = np.array([R.record(o, c) for o, c in zip(rng.choice([0.0, 0.3, 0.5, 0.8, 1.0], len(first)), rng.integers(1, 1 << 32, len(first)))], np.uint64)
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
        d = rng.normal(size=(200, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        pts = (np.asarray(sensor) + d * rng.uniform(3.0, 75.0, (200, 1))).astype(np.float32)
        _, carved, hits = RR.frame(ref, sensor, pts, 60.0)
        H, M = F.sets_of(carved, hits)
        named = sorted(H | M)
        assert len(named) > 5000
        sample = rng.integers(-100, 100, (4000, 3)).astype(np.float64) + 0.5
        for k, (at, max_range, model) in enumerate([(sensor, 60.0, None), ((25.5, 40.5, 12.5), 200.0, (0.9, 0.45, 0.2, 0.8)), (sensor, 60.0, None)]):
            st, counts = m.fuse_rays(at, pts, max_range, model)
            want_st, want_counts = F.fuse_rays(ref, at, pts, max_range, model)
            assert np.array_equal(st, want_st) and counts == want_counts, "frame %d" % k
            if k == 0:
                assert counts["new_chunks"] >= 8 and counts["rays_truncated"] > 10 and counts["rays_hit"] > 50
                cells_now = sum(kind == "cells" for kind, _ in ref.chunks.values())
                assert cells_now > counts["new_chunks"], "no chunk-filled chunk was crossed"
                info = m.info()
                assert (info["chunk_filled"], info["cell_filled"]) == (len(first) - (cells_now - counts["new_chunks"]), cells_now)
                assert info["capacity_chunks"] == len(first) + room, "the pool grew: the new chunks' slots are not where the test wants them"
                assert info["scratch_bytes"] > 1 << 31, "the mark plane covers the pool: its bytes past 2^31 belong to the new chunks"
            # every cell the walks name, then cells no ray touched: in the new chunks, in the chunks that turned into cells, in absent space
            for loc in (np.asarray(named, np.float64) + 0.5, sample):
                rec, status = m.get(loc)
                want_rec, want_status = ref.get_batch(loc)
                assert np.array_equal(status, want_status) and np.array_equal(rec, want_rec), "frame %d" % k
        assert set(np.unique(status).tolist()) == {0, 1, 2}
    finally:
        m.close()
