"""GPU: sdfgpu_rasterize_shapes_device on a NON-BLOCKING side stream whose shapes arrive late (tests/stream_harness.py, as
tests/test_gpu_stream_order_resample.py does for Resample).

The shape buffer holds decoys (the same shapes elsewhere, with other ids); behind a measured delay on the side stream the real
shapes are copied over them.  The memset of the status word, the three kernels and the read-back of the status word must run on
that stream: the consumer, clones enqueued there, must see bits, mask and ids of the REAL shapes, and the witnesses on the null
stream and on a second side stream must still hold the decoys.  Once without the check (the call returns with its work pending)
and once with it (the call synchronises its stream); red zones off and on."""
import numpy as np
import pytest

import scene_cases as SC
import scene_raster_restated as R
import stream_harness as H
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

GRID, RES = (33, 17, 96), SC.RES
ORIGIN = SC.origins()["general"]


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
    ext = np.asarray(GRID) * RES

    def shapes(shift, first_id):
        items = []
        for i, (kind, where) in enumerate([(SC.CYLINDER, (0.3, 0.5, 0.3)), (SC.BOX, (0.6, 0.4, 0.6)), (SC.SPHERE, (0.5, 0.6, 0.8))]):
            pose = ORIGIN @ SC._local(SC.GENERIC_Q, ext * (np.asarray(where) + shift))
            items.append((kind, first_id + i, SC._dims(kind, np.full(3, 6.3 * RES)), pose))
        return capi.make_shapes(items)

    decoy, real = shapes(-0.08, 11), shapes(0.0, 1)
    return decoy, real, [R.restated(s, ORIGIN, RES, GRID) for s in (decoy, real)]


@pytest.mark.parametrize("check", [False, True], ids=["pending", "checked"])
def test_rasterize_shapes_honours_its_stream(ctx, delay, streams, scene, check):
    decoy, real, want = scene
    case = H.Case(delay, streams[0], streams[1])
    n = int(np.prod(GRID))
    d_shapes = case.input("shapes", decoy.view(np.uint8), real.view(np.uint8))
    d_bits, d_mask, d_ids = case.output("bits", (n + 31) // 32 * 4), case.output("mask", n), case.output("ids", n * 4)
    s = case.side.cuda_stream

    def call():
        return ctx.rasterize_shapes_device(d_shapes, len(real), ORIGIN, RES, GRID, d_bits, d_mask, d_ids, check=check, stream=s)
    case.warm(call)
    case.arm()
    bad = call()
    if not check and not ctx.redzones:
        case.witness("when the asynchronous call had returned")
    case.consume()
    got = case.finish()
    H.expect("the bits", H.view(got["bits"], np.uint32), want[1][2], want[0][2])
    H.expect("the mask", H.view(got["mask"], np.uint8, GRID), want[1][0], want[0][0])
    H.expect("the ids", H.view(got["ids"], np.uint32, GRID), want[1][1], want[0][1])
    assert bad == (-1 if check else None)
