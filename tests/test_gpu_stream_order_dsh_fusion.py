"""GPU: sdfgpu_dsh_fuse_rays_device on a NON-BLOCKING side stream whose points arrive late (tests/stream_harness.py, as
tests/test_gpu_stream_order_dsh_rays.py does for the carve).

The points hold decoys; behind a measured delay on the side stream the real ones are copied over them.  Every kernel, memset, copy
and read-back of the call -- the mark plane's clearing among them -- must run on that stream: the map must end in the state of the REAL
frame (the restatement, tests/dsh_fusion_restated.py, applies the same sequence: the harness's two warm calls on the decoys, then the
real one), the statuses and the counts must be the real frame's, and the witnesses on the null stream and on a second side stream must
still hold the decoys."""
import numpy as np
import pytest

import dsh_restated as R
import dsh_fusion_restated as F
import stream_harness as H

pytestmark = pytest.mark.gpu

DIMS, N = (3, 2, 5), 240
DEFAULT = R.record(0.5, 0x77)
SENSOR, MAX_RANGE, MODEL = (0.5, -0.25, 1.5), 14.0, (0.8, 0.35, 0.1, 0.95)


@pytest.fixture(scope="module")
def delay():
    return H.Delay()


@pytest.fixture(scope="module")
def streams(delay):
    return H.pick_streams(delay)


def points(seed, bad_at):
    rng = np.random.default_rng(seed)
    pts = (rng.integers(-12, 12, (N, 3)) + rng.choice([0.0, 0.25, 0.5], (N, 3))).astype(np.float32)
    pts[bad_at] = np.nan
    return pts


@pytest.mark.parametrize("grow", [False, True], ids=["room-in-the-map", "table-pool-and-marks-grow"])
def test_fuse_rays_honours_its_stream(gpu, delay, streams, grow):
    """with `grow` the map starts with a 16-entry table and a one-chunk pool, so the warm calls and the real one run the count pass,
    the rehash, the pool's copies and the mark plane's clearing on the side stream as well"""
    m = gpu.dsh_create(None, 1.0, DIMS, DEFAULT, initial_chunks=1 if grow else 4096)
    ref = R.Map(None, 1.0, DIMS, DEFAULT)
    try:
        decoy, real = points(1, 5), points(2, 9)
        case = H.Case(delay, streams[0], streams[1])
        p_pts = case.input("points", decoy.view(np.uint8).reshape(-1), real.view(np.uint8).reshape(-1))
        p_st = case.output("statuses", N)
        counts = []

        def call():
            counts.append(m.fuse_rays_device(SENSOR, p_pts, N, MAX_RANGE, MODEL, d_statuses=p_st, stream=case.side.cuda_stream))
        case.warm(call)
        case.arm()
        call()
        case.consume()
        got = case.finish()
        decoy_statuses, decoy_counts = F.fuse_rays(ref, SENSOR, decoy, MAX_RANGE, MODEL)
        F.fuse_rays(ref, SENSOR, decoy, MAX_RANGE, MODEL)
        want_statuses, want_counts = F.fuse_rays(ref, SENSOR, real, MAX_RANGE, MODEL)
        H.expect("the statuses", H.view(got["statuses"], np.uint8), want_statuses, decoy_statuses)
        assert counts[0] == decoy_counts and counts[-1] == want_counts and want_counts["rays_truncated"] > 10 and want_counts["new_chunks"] > 0
        chunks, cells = m.export()
        want, want_cells = ref.export()
        assert [tuple(c) for c in chunks["c"]] == [w[0] for w in want] and chunks["state"].tolist() == [w[1] for w in want]
        assert np.array_equal(cells, want_cells)
    finally:
        m.close()
