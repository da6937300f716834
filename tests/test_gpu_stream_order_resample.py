"""GPU: sdfgpu_resample_cells_device on a NON-BLOCKING side stream whose source arrives late (tests/stream_harness.py, as
tests/test_gpu_stream_order.py does for the other device entry points).

The source buffer holds a decoy (other records of the same shape); behind a measured delay on the side stream the real records are
copied over it.  The memset of the winner words, both kernels and the read-back of the counter must run on that stream: the
consumer, a clone enqueued there, must see the result of the REAL source, and the witnesses on the null stream and on a second side
stream must still hold the decoy.  Once without the count (the call returns with its work pending, 32-bit winner words) and once
with out_cells_written requested (the call synchronises its stream); red zones off and on."""
import numpy as np
import pytest

import resample_restated as R
import stream_harness as H

pytestmark = pytest.mark.gpu

SHAPE, CB, CELL, RATIO = (33, 17, 96), 16, 0.05, 2.0
ORIGIN = R.origins()["general"]


@pytest.fixture(scope="module")
def delay():
    return H.Delay()


@pytest.fixture(scope="module")
def streams(delay):
    return H.pick_streams(delay)


@pytest.fixture(params=[0, 1], ids=["asynchronous", "redzones"])
def ctx(gpu, request):
    gpu.set_option("redzone", request.param)
    gpu.redzones = bool(request.param)
    yield gpu
    gpu.set_option("redzone", 0)


@pytest.fixture(scope="module")
def scene():
    real = R.payload(SHAPE, CB, seed=7)
    decoy = real ^ np.uint8(0x55)
    fill = R.oob_record(CB)
    want = [R.restated(x, CELL, ORIGIN, CELL * RATIO, fill) for x in (decoy, real)]
    return decoy, real, fill, want


@pytest.mark.parametrize("count", [False, True], ids=["pending", "count"])
def test_resample_honours_its_stream(ctx, delay, streams, scene, count):
    decoy, real, fill, want = scene
    case = H.Case(delay, streams[0], streams[1])
    src = case.input("source", decoy, real)
    dst = case.output("result", want[1].cells.nbytes)
    s = case.side.cuda_stream

    def call():
        return ctx.resample_cells_device(src, SHAPE, CELL, ORIGIN, want[1].inverse, want[1].inv_cell, dst, want[1].shape, fill, CB,
                                         count=count, stream=s)
    case.warm(call)
    case.arm()
    written = call()
    if not count and not ctx.redzones:
        case.witness("when the asynchronous call had returned")
    case.consume()
    got = case.finish()
    H.expect("the result", H.view(got["result"], np.uint8, want[1].cells.shape), want[1].cells, want[0].cells)
    assert written == (want[1].written if count else None)
