"""GPU: the display export's device entry points on a NON-BLOCKING side stream whose inputs arrive late (tests/stream_harness.py, as
tests/test_gpu_stream_order_resample.py does for the resample).

Every input buffer holds a decoy; behind a measured delay on the side stream the real input is copied over it.  The memsets, the
kernels, the upload of the draw keys and the read-backs of the status words must all run on that stream: the consumer, clones
enqueued there, must see the result of the REAL input, and the witnesses on the null stream and on a second side stream must still
hold the decoy.  sdfgpu_display_expand_device returns with its kernel pending; the others synchronise their stream.  Red zones off
and on."""
import numpy as np
import pytest

import display_cases as C
import display_restated as R
import stream_harness as H
from sdf_tools_amd import capi

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
    gpu.redzones = bool(request.param)
    yield gpu
    gpu.set_option("redzone", 0)


def _records(seed):
    rng = np.random.default_rng(seed)
    occ = rng.choice(C.OCC_VALUES, size=SHAPE)
    keys = rng.choice(np.array([0, 3, 300, 70000, 2 ** 32 - 1], np.uint32), size=SHAPE)
    return occ, keys


def _words(raw, count):
    w = H.view(raw, np.uint32)
    assert (H.view(raw, np.uint8)[count * 4:] == H.SENTINEL).all(), "words behind the result were written"
    return w[:count]


@pytest.mark.parametrize("rule", [capi.DISPLAY_OCCUPANCY, capi.DISPLAY_KEY_FIELD], ids=["occupancy", "key_field"])
def test_select_cells_honours_its_stream(ctx, delay, streams, rule):
    opts = dict(class_mask=5, surface_only=True) if rule == capi.DISPLAY_OCCUPANCY else dict(draw_keys=[3, 300, 2 ** 32 - 1], draw_zero=False)
    (d_occ, d_keys), (r_occ, r_keys) = _records(1), _records(2)
    want = [C.reference(o, k, rule, True, **opts) for o, k in ((d_occ, d_keys), (r_occ, r_keys))]
    case = H.Case(delay, streams[0], streams[1])
    cells = case.input("cells", R.cells_of(d_occ, d_keys, 16), R.cells_of(r_occ, r_keys, 16))
    outs = [case.output(name, N * 4) for name in ("indices", "keys")] + [case.output("group_keys", 8 * 4), case.output("group_offsets", 9 * 4)]
    s = case.side.cuda_stream

    def call():
        return ctx.display_select_cells_device(cells, SHAPE, rule, 16, 0, 4, grouped=True, d_indices=outs[0], d_keys=outs[1], capacity=N,
                                               d_group_keys=outs[2], d_group_offsets=outs[3], group_capacity=8, stream=s, **opts)
    case.warm(call)
    case.arm()
    total, groups = call()
    case.consume()
    got = case.finish()
    assert (total, groups) == (len(want[1][0]), len(want[1][2])), "the status words were read ahead of the work"
    assert len(want[0][0]) != len(want[1][0])
    for name, w_real, w_decoy, count in zip(("indices", "keys", "group_keys", "group_offsets"), want[1], want[0],
                                            (total, total, groups, groups + 1)):
        H.expect(name, _words(got[name], count), w_real, w_decoy if len(w_decoy) != len(w_real) or not H.same(w_decoy, w_real) else None)


def test_select_sdf_honours_its_stream(ctx, delay, streams):
    rng = np.random.default_rng(3)
    fields = [rng.standard_normal(SHAPE).astype(np.float32) for _ in range(2)]
    want = [R.select_sdf(f)[0] for f in fields]
    case = H.Case(delay, streams[0], streams[1])
    sdf = case.input("sdf", *fields)
    out = case.output("indices", N * 4)
    s = case.side.cuda_stream

    def call():
        return ctx.display_select_sdf_device(sdf, SHAPE, out, N, stream=s)
    case.warm(call)
    case.arm()
    total = call()
    case.consume()
    got = case.finish()
    assert total == len(want[1]) != len(want[0])
    H.expect("indices", _words(got["indices"], total), want[1], want[0])


def test_expand_honours_its_stream(ctx, delay, streams):
    rng = np.random.default_rng(4)
    count, cell, default = 50000, (0.1, 0.25, 3.0), (0.5, 0.25, 0.125, 1.0)
    idx = [rng.integers(0, N, size=count).astype(np.uint32) for _ in range(2)]
    keys = [rng.integers(0, 6, size=count).astype(np.uint32) for _ in range(2)]
    table = [rng.random((4, 4)).astype(np.float32) for _ in range(2)]
    case = H.Case(delay, streams[0], streams[1])
    d_idx, d_keys, d_table = case.input("indices", *idx), case.input("keys", *keys), case.input("table", *table)
    pts, col = case.output("points", count * 24), case.output("colors", count * 16)
    s = case.side.cuda_stream

    def call():
        ctx.display_expand_device(d_idx, count, SHAPE, cell, d_points=pts, d_colors=col, d_keys=d_keys, d_color_table=d_table, table_entries=4,
                                  default_color=default, stream=s)
    case.warm(call)
    case.arm()
    call()
    if not ctx.redzones:
        case.witness("when the asynchronous call had returned")
    case.consume()
    got = case.finish()
    H.expect("points", H.view(got["points"], np.float64, (count, 3)), R.points(idx[1], SHAPE, cell), R.points(idx[0], SHAPE, cell))
    H.expect("colors", H.view(got["colors"], np.float32, (count, 4)), R.table_colors(keys[1], table[1], default),
             R.table_colors(keys[0], table[0], default))


def test_sdf_colors_honours_its_stream(ctx, delay, streams):
    rng = np.random.default_rng(5)
    fields = [(rng.standard_normal(SHAPE) * scale).astype(np.float32) for scale in (1.0, 3.0)]
    case = H.Case(delay, streams[0], streams[1])
    sdf = case.input("sdf", *fields)
    out = case.output("colors", N * 16)
    s = case.side.cuda_stream

    def call():
        ctx.display_sdf_colors_device(sdf, SHAPE, 0.5, out, stream=s)
    case.warm(call)
    case.arm()
    call()
    case.consume()
    got = case.finish()
    H.expect("colors", H.view(got["colors"], np.float32, SHAPE + (4,)), R.sdf_colors(fields[1], 0.5), R.sdf_colors(fields[0], 0.5))
