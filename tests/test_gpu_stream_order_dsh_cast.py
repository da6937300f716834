"""GPU: sdfgpu_dsh_cast_rays_device and sdfgpu_dsh_cast_segments_device on a NON-BLOCKING side stream whose points (or starts) arrive
late (tests/stream_harness.py, as tests/test_gpu_stream_order_dsh_rays.py does for a frame).

The input holds decoys; behind a measured delay on the side stream the real one is copied over them.  The call's one kernel must run
on that stream: the statuses and the hit records must be the real input's (the restatement, tests/dsh_cast_restated.py), and the
witnesses on the null stream and on a second side stream must still hold the decoys.  A cast synchronises nothing: the call returns
while the delay is still running, which the harness's witnesses rely on."""
import numpy as np
import pytest

import dsh_cast_restated as C
import dsh_restated as R
import stream_harness as H

pytestmark = pytest.mark.gpu

DIMS, N = (3, 2, 5), 240
DEFAULT, FREE, FILLED = R.record(0.5, 0x77), R.record(0.0, 1), R.record(1.0, 2)
SENSOR, MAX_RANGE = (0.5, -0.25, 1.5), 11.0


def ends(seed, bad_at, dtype):
    rng = np.random.default_rng(seed)
    pts = (rng.integers(-12, 12, (N, 3)) + rng.choice([0.0, 0.25, 0.5], (N, 3))).astype(dtype)
    pts[bad_at] = np.nan
    return pts


@pytest.fixture(scope="module")
def delay():
    return H.Delay()


@pytest.fixture(scope="module")
def streams(delay):
    return H.pick_streams(delay)


@pytest.fixture
def scene(gpu):
    m = gpu.dsh_create(None, 1.0, DIMS, DEFAULT)
    ref = R.Map(None, 1.0, DIMS, DEFAULT)
    rng = np.random.default_rng(335)
    chunks, cells = rng.uniform(-12, 12, (40, 3)), rng.uniform(-12, 12, (500, 3))
    chunk_values = np.array([[FREE, FILLED][k % 2] for k in range(40)], np.uint64)
    cell_values = np.array([[FILLED, FREE, DEFAULT][k % 3] for k in range(500)], np.uint64)
    for target in (m, ref):
        target.set_chunks(chunks, chunk_values)
        target.set_cells(cells, cell_values)
        target.set_chunks([SENSOR], FREE)
    yield m, ref
    m.close()


@pytest.mark.parametrize("form", ["rays", "segments"])
def test_a_cast_honours_its_stream(scene, delay, streams, form):
    m, ref = scene
    flags = C.SKIP_FIRST
    case = H.Case(delay, streams[0], streams[1])
    if form == "rays":
        decoy, real = ends(1, 5, np.float32), ends(2, 9, np.float32)
        p_in = case.input("points", decoy.view(np.uint8).reshape(-1), real.view(np.uint8).reshape(-1))
        want, want_decoy = C.cast_rays(ref, SENSOR, real, MAX_RANGE, flags), C.cast_rays(ref, SENSOR, decoy, MAX_RANGE, flags)
    else:
        decoy, real = ends(3, 5, np.float64), ends(4, 9, np.float64)            # the STARTS arrive late; the ends are there from the beginning
        fixed = ends(5, 17, np.float64)
        p_in = case.input("starts", decoy.view(np.uint8).reshape(-1), real.view(np.uint8).reshape(-1))
        d_ends = H.to_device(fixed)
        want, want_decoy = C.cast_segments(ref, real, fixed, MAX_RANGE, flags), C.cast_segments(ref, decoy, fixed, MAX_RANGE, flags)
    p_st, p_hits = case.output("statuses", N), case.output("hits", N * 48)

    def call():
        if form == "rays":
            m.cast_rays_device(SENSOR, p_in, N, MAX_RANGE, flags, p_st, p_hits, case.side.cuda_stream)
        else:
            m.cast_segments_device(p_in, d_ends.data_ptr(), N, MAX_RANGE, flags, p_st, p_hits, case.side.cuda_stream)
    before = m.export()
    case.warm(call)
    case.arm()
    call()
    case.consume()
    got = case.finish()
    H.expect("the statuses", H.view(got["statuses"], np.uint8), want[0], want_decoy[0])
    H.expect("the hits", H.view(got["hits"], np.uint8), want[1].view(np.uint8).reshape(-1), want_decoy[1].view(np.uint8).reshape(-1))
    assert (want[0] == C.CAST_BLOCKED).sum() > 50 and (want[0] == C.CAST_SKIPPED).sum() >= 1 and (want[0] == C.CAST_CLEAR_IN_RANGE).sum() > 5
    after = m.export()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
