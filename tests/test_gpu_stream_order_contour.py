"""GPU: sdfgpu_display_select_contour_device on a NON-BLOCKING side stream whose input arrives late (tests/stream_harness.py, as
tests/test_gpu_stream_order_display.py does for the other selections).

The record buffer holds a decoy; behind a measured delay on the side stream the real records are copied over it.  The memset of the
status words, k_dp_contour, the upload of the draw keys, the compaction, the sort, the group steps and the read-backs must all run on
that stream: the call's totals and the consumer's clones must be those of the REAL records.  Red zones off and on."""
import numpy as np
import pytest

import contour_cases as K
import display_cases as C
import display_restated as R
import stream_harness as H

pytestmark = pytest.mark.gpu

SHAPE = (33, 17, 96)
N = int(np.prod(SHAPE))


@pytest.fixture(scope="module")
def delay():
    return H.Delay()


@pytest.fixture(scope="module")
def streams(delay):
    return H.pick_streams(delay)


@pytest.fixture(params=[0, 1], ids=["asynchronous", "redzones"])
def ctx(gpu, request):
    gpu.set_option("redzone", request.param)
    yield gpu
    gpu.set_option("redzone", 0)


def _records(seed):
    rng = np.random.default_rng(seed)
    occ = np.where(rng.random(SHAPE) < 0.8, np.float32(1.0), rng.choice(C.OCC_VALUES, size=SHAPE)).astype(np.float32)
    x = np.arange(SHAPE[0])[:, None, None] * 5 // SHAPE[0]
    keys = np.array([0, 3, 300, 70000, 2 ** 32 - 1], np.uint32)[(x + seed) % 5] * np.ones(SHAPE, np.uint32)
    keys[rng.random(SHAPE) < 0.02] = 9
    return occ, keys


def _words(raw, count):
    w = H.view(raw, np.uint32)
    assert (H.view(raw, np.uint8)[count * 4:] == H.SENTINEL).all(), "words behind the result were written"
    return w[:count]


def test_select_contour_honours_its_stream(ctx, delay, streams):
    opts = dict(draw_keys=[3, 9, 300, 2 ** 32 - 1], unknown_is_filled=True, draw_zero=False)
    (d_occ, d_keys), (r_occ, r_keys) = _records(1), _records(2)
    want = [K.reference(o, k, 3, True, **opts) for o, k in ((d_occ, d_keys), (r_occ, r_keys))]
    case = H.Case(delay, streams[0], streams[1])
    cells = case.input("cells", R.cells_of(d_occ, d_keys, 16, 8), R.cells_of(r_occ, r_keys, 16, 8))
    outs = [case.output(name, N * 4) for name in ("indices", "keys")] + [case.output("group_keys", 8 * 4), case.output("group_offsets", 9 * 4)]
    s = case.side.cuda_stream

    def call():
        return ctx.display_select_contour_device(cells, SHAPE, 3, 16, 0, 8, grouped=True, d_indices=outs[0], d_keys=outs[1], capacity=N,
                                                 d_group_keys=outs[2], d_group_offsets=outs[3], group_capacity=8, stream=s, **opts)
    case.warm(call)
    case.arm()
    total, groups = call()
    case.consume()
    got = case.finish()
    assert (total, groups) == (len(want[1][0]), len(want[1][2])), "the status words were read ahead of the work"
    assert len(want[0][0]) != len(want[1][0]) and groups == 4
    for name, w_real, w_decoy, count in zip(("indices", "keys", "group_keys", "group_offsets"), want[1], want[0],
                                            (total, total, groups, groups + 1)):
        H.expect(name, _words(got[name], count), w_real, w_decoy if len(w_decoy) != len(w_real) or not H.same(w_decoy, w_real) else None)
