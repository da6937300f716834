"""GPU: every sdfgpu_dsh_*_device entry point on a NON-BLOCKING side stream whose inputs arrive late (tests/stream_harness.py, as
tests/test_gpu_stream_order_mesh.py does for the mesh rasteriser), and two calls on one map from two side streams.

The locations and values hold decoys; behind a measured delay on the side stream the real ones are copied over them.  Every kernel,
memset, copy and read-back of a call must run on that stream: the map must end in the state of the REAL operations (the restatement,
tests/dsh_restated.py, applies the same sequence: the harness's two warm calls on the decoys, then the real one), and the witnesses
on the null stream and on a second side stream must still hold the decoys."""
import numpy as np
import pytest
import torch

import dsh_restated as R
import stream_harness as H
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

DIMS, N = (3, 2, 5), 240
DEFAULT = R.record(0.5, 0x77)


@pytest.fixture(scope="module")
def delay():
    return H.Delay()


@pytest.fixture(scope="module")
def streams(delay):
    return H.pick_streams(delay)


def operations(seed, bad_at, dtype=np.float64):
    rng = np.random.default_rng(seed)
    loc = (rng.integers(-20, 20, (N, 3)) + 0.5).astype(dtype)
    loc[bad_at] = np.nan
    return loc, rng.integers(1, 1 << 63, N, dtype=np.uint64)


class Maps:
    def __init__(self, gpu):
        self.gpu = gpu.dsh_create(None, 1.0, DIMS, DEFAULT)
        self.ref = R.Map(None, 1.0, DIMS, DEFAULT)

    def check(self):
        chunks, cells = self.gpu.export()
        want, want_cells = self.ref.export()
        assert [tuple(c) for c in chunks["c"]] == [w[0] for w in want] and chunks["state"].tolist() == [w[1] for w in want]
        assert chunks["record"].tolist() == [w[2] for w in want] and np.array_equal(cells, want_cells)


@pytest.fixture
def maps(gpu):
    m = Maps(gpu)
    yield m
    m.gpu.close()


@pytest.mark.parametrize("kind", ["set_cells", "set_chunks", "insert_points"])
def test_the_setters_honour_their_stream(maps, delay, streams, kind):
    dtype = np.float32 if kind == "insert_points" else np.float64
    (d_loc, d_val), (r_loc, r_val) = operations(1, 5, dtype), operations(2, 9, dtype)
    case = H.Case(delay, streams[0], streams[1])
    p_loc = case.input("locations", d_loc.view(np.uint8).reshape(-1), r_loc.view(np.uint8).reshape(-1))
    p_val = case.input("values", d_val.view(np.uint8), r_val.view(np.uint8))
    p_st = case.output("statuses", N)
    s = case.side.cuda_stream
    one = R.record(1.0, 3)
    call = {"set_cells": lambda: maps.gpu.set_cells_device(p_loc, N, d_values=p_val, d_statuses=p_st, stream=s),
            "set_chunks": lambda: maps.gpu.set_chunks_device(p_loc, N, d_values=p_val, d_statuses=p_st, stream=s),
            "insert_points": lambda: maps.gpu.insert_points_device(p_loc, N, one, d_statuses=p_st, stream=s)}[kind]
    apply = {"set_cells": lambda l, v: maps.ref.set_cells(l, v), "set_chunks": lambda l, v: maps.ref.set_chunks(l, v),
             "insert_points": lambda l, v: maps.ref.insert_points(l, one)}[kind]
    case.warm(call)
    case.arm()
    call()
    case.consume()
    got = case.finish()
    apply(d_loc, d_val)
    apply(d_loc, d_val)
    decoy_statuses = np.where(np.isnan(d_loc[:, 0]), 0, 1 if kind == "set_chunks" else 2).astype(np.uint8)
    H.expect("the statuses", H.view(got["statuses"], np.uint8), apply(r_loc, r_val), decoy_statuses)
    maps.check()


def test_get_honours_its_stream(maps, delay, streams):
    (d_loc, d_val), (r_loc, r_val) = operations(3, 5), operations(4, 9)
    for loc, val in ((d_loc, d_val), (r_loc[::2], r_val[::2])):
        maps.gpu.set_cells(loc[:100], val[:100])
        maps.ref.set_cells(loc[:100], val[:100])
        maps.gpu.set_chunks(loc[100:], val[100:])
        maps.ref.set_chunks(loc[100:], val[100:])
    case = H.Case(delay, streams[0], streams[1])
    p_loc = case.input("locations", d_loc.view(np.uint8).reshape(-1), r_loc.view(np.uint8).reshape(-1))
    p_rec, p_st = case.output("records", N * 8), case.output("statuses", N)

    def call():
        maps.gpu.get_device(p_loc, N, p_rec, p_st, stream=case.side.cuda_stream)
    case.warm(call)
    case.arm()
    call()
    case.witness("when the asynchronous call had returned")
    case.consume()
    got = case.finish()
    want, decoy = maps.ref.get_batch(r_loc), maps.ref.get_batch(d_loc)
    H.expect("the records", H.view(got["records"], np.uint64), want[0], decoy[0])
    H.expect("the statuses", H.view(got["statuses"], np.uint8), want[1], decoy[1])


@pytest.mark.parametrize("what", ["window", "export"])
def test_window_and_export_see_the_sets_in_front_of_them_on_their_stream(maps, delay, streams, what):
    """the input that arrives late is the map's content: a cell batch on the same stream, in front of the read"""
    (d_loc, d_val), (r_loc, r_val) = operations(5, 5), operations(6, 9)
    lower, shape = (-7, -3, -9), (7, 6, 31)
    n_vox = int(np.prod(shape))
    case = H.Case(delay, streams[0], streams[1])
    p_loc = case.input("locations", d_loc.view(np.uint8).reshape(-1), r_loc.view(np.uint8).reshape(-1))
    p_val = case.input("values", d_val.view(np.uint8), r_val.view(np.uint8))
    s = case.side.cuda_stream
    if what == "window":
        p_rec, p_bits = case.output("records", n_vox * 8), case.output("bits", (n_vox + 31) // 32 * 4)
    else:
        cap_chunks, cap_cells = 3 * N, 3 * N * 30
        p_chunks, p_cells = case.output("chunks", cap_chunks * 48), case.output("cells", cap_cells * 8)
    counts = []

    def call():
        maps.gpu.set_cells_device(p_loc, N, d_values=p_val, stream=s)
        if what == "window":
            maps.gpu.extract_window_device(lower, shape, True, p_rec, p_bits, stream=s)
        else:
            counts.append(maps.gpu.export_device(p_chunks, cap_chunks, p_cells, cap_cells, stream=s))
    case.warm(call)
    case.arm()
    call()
    case.consume()
    got = case.finish()
    maps.ref.set_cells(d_loc, d_val)
    maps.ref.set_cells(d_loc, d_val)
    if what == "window":
        decoy = maps.ref.window(lower, shape)
        maps.ref.set_cells(r_loc, r_val)
        want = maps.ref.window(lower, shape)
        H.expect("the records", H.view(got["records"], np.uint64, shape), want, decoy)
        H.expect("the bits", H.view(got["bits"], np.uint32), R.pack_bits(R.classify(want, True)), R.pack_bits(R.classify(decoy, True)))
    else:
        n_decoy = len(maps.ref.chunks)
        maps.ref.set_cells(r_loc, r_val)
        want, want_cells = maps.ref.export()
        assert counts[-1] == (len(want), want_cells.size) and len(want) > n_decoy
        chunks = np.frombuffer(got["chunks"].tobytes()[:len(want) * 48], capi.DSH_CHUNK_DTYPE)
        assert [tuple(c) for c in chunks["c"]] == [w[0] for w in want] and chunks["first_cell"].tolist() == [w[3] for w in want]
        assert np.array_equal(H.view(got["cells"], np.uint64)[:want_cells.size], want_cells.reshape(-1))
    maps.check()


def test_two_calls_on_two_side_streams(maps, delay, streams):
    """a Get pending on one side stream behind late locations, then a chunk batch on the other: the batch must wait for the Get on the
    device (the map's event), so the Get still sees the map as it was"""
    (d_loc, d_val), (r_loc, r_val) = operations(7, 5), operations(8, 9)
    maps.gpu.set_cells(r_loc[::3], r_val[::3])
    maps.ref.set_cells(r_loc[::3], r_val[::3])
    case = H.Case(delay, streams[0])
    p_loc = case.input("locations", d_loc.view(np.uint8).reshape(-1), r_loc.view(np.uint8).reshape(-1))
    p_rec, p_st = case.output("records", N * 8), case.output("statuses", N)
    over = torch.from_numpy(np.nan_to_num(r_loc, nan=0.5)).cuda()
    overwrite = R.record(1.0, 0xFEED)
    torch.cuda.synchronize()
    before = maps.ref.get_batch(r_loc), maps.ref.get_batch(d_loc)

    def call(second=True):
        maps.gpu.get_device(p_loc, N, p_rec, p_st, stream=case.side.cuda_stream)
        if second:
            maps.gpu.set_chunks_device(over.data_ptr(), N, one_value=overwrite, stream=streams[1].cuda_stream)
    case.warm(lambda: call(False))
    case.arm()
    call()
    case.consume()
    got = case.finish()
    H.expect("the records", H.view(got["records"], np.uint64), before[0][0], before[1][0])
    H.expect("the statuses", H.view(got["statuses"], np.uint8), before[0][1], before[1][1])
    maps.ref.set_chunks(np.nan_to_num(r_loc, nan=0.5), overwrite)
    maps.check()
    assert (maps.gpu.get(np.nan_to_num(r_loc, nan=0.5))[0] == np.uint64(overwrite)).all()
