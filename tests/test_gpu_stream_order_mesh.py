"""GPU: sdfgpu_rasterize_meshes_device on a NON-BLOCKING side stream whose inputs arrive late (tests/stream_harness.py, as
tests/test_gpu_stream_order_scene.py does for the shape rasteriser).

The mesh records, the vertices and the triangles hold decoys (the meshes elsewhere, with other ids, other vertices and fewer
triangles); behind a measured delay on the side stream the real ones are copied over them.  The memsets, the five kernels and the
read-back of the status word must run on that stream: the consumer, clones enqueued there, must see bits, mask and ids of the REAL
meshes, and the witnesses on the null stream and on a second side stream must still hold the decoys.  Once without the check (the
call returns with its work pending) and once with it (the call synchronises its stream); red zones off and on."""
import numpy as np
import pytest

import mesh_cases as MC
import mesh_raster_restated as R
import stream_harness as H
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

GRID, RES = (33, 17, 96), MC.RES
ORIGIN = MC.origins()["general"]


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

    def meshes(shift, first_id, scale):
        items = []
        for i, where in enumerate([(0.3, 0.5, 0.3), (0.6, 0.4, 0.6), (0.5, 0.6, 0.8)]):
            v, t = MC.icosahedron(scale * (2.0 + i) * RES) if i != 1 else MC.box_triangles(np.full(3, scale * 5.3 * RES))
            items.append((first_id + i, v, t, ORIGIN @ MC._local(MC.GENERIC_Q, ext * (np.asarray(where) + shift))))
        return capi.make_meshes(items)

    decoy, real = meshes(-0.08, 11, 0.8), meshes(0.0, 1, 1.0)
    decoy[2][:] = decoy[2][:, ::-1]                                            # (same counts, other index orders: the arrays differ)
    return decoy, real, [R.restated(*s, ORIGIN, RES, GRID) for s in (decoy, real)]


@pytest.mark.parametrize("check", [False, True], ids=["pending", "checked"])
def test_rasterize_meshes_honours_its_stream(ctx, delay, streams, scene, check):
    decoy, real, want = scene
    case = H.Case(delay, streams[0], streams[1])
    n = int(np.prod(GRID))
    d_in = [case.input(name, np.ascontiguousarray(d).view(np.uint8).reshape(-1), np.ascontiguousarray(r).view(np.uint8).reshape(-1))
            for name, d, r in zip(("meshes", "vertices", "triangles"), decoy, real)]
    d_bits, d_mask, d_ids = case.output("bits", (n + 31) // 32 * 4), case.output("mask", n), case.output("ids", n * 4)
    s = case.side.cuda_stream

    def call():
        return ctx.rasterize_meshes_device(d_in[0], len(real[0]), d_in[1], len(real[1]), d_in[2], len(real[2]), ORIGIN, RES, GRID, d_bits, d_mask, d_ids,
                                           check=check, stream=s)
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
    assert not np.array_equal(want[0][0], want[1][0])
