"""GPU: sdfgpu_dsh_update_components among calls on other NON-BLOCKING streams (tests/stream_harness.py, in the style of
tests/test_gpu_stream_order_dsh_frontier.py).

Case 1: a cell batch on a side stream whose locations and values hold decoys until the real ones are copied over them behind a
measured delay, then an update on ANOTHER side stream: the labels must be those of the map after the real batch.  Case 2: a Get on
a THIRD stream behind the update must see the new labels.  What orders the three is the map's own event, nothing else."""
import numpy as np
import pytest
import torch

import dsh_components_restated as C
import dsh_restated as R
import stream_harness as H
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

DIMS, N = (3, 2, 5), 240
DEFAULT = R.record(0.5, 0x77)
VALUES = [R.record(0.0, 1), R.record(0.0, 2), R.record(1.0, 3), R.record(0.5, 4)]


@pytest.fixture(scope="module")
def delay():
    return H.Delay()


@pytest.fixture(scope="module")
def streams(delay):
    return H.pick_streams(delay)


def operations(seed, bad_at):
    rng = np.random.default_rng(seed)
    loc = rng.integers(-9, 9, (N, 3)) + 0.5
    loc[bad_at] = np.nan
    return loc, np.array([VALUES[int(k)] for k in rng.integers(0, 4, N)], np.uint64)


@pytest.mark.parametrize("flags", [0, capi.DSH_COMPONENTS_UNKNOWN_APART])
def test_an_update_follows_a_late_batch_on_another_stream_and_a_get_on_a_third_sees_it(gpu, delay, streams, flags):
    m, ref = gpu.dsh_create(None, 1.0, DIMS, DEFAULT), R.Map(None, 1.0, DIMS, DEFAULT)
    try:
        (d_loc, d_val), (r_loc, r_val) = operations(361, 5), operations(362, 9)
        probes = np.stack(np.meshgrid(*[np.arange(-10, 10)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5
        d_probes = torch.from_numpy(probes).cuda()
        case = H.Case(delay, streams[0])                                       # (the second side stream runs the update)
        p_loc = case.input("locations", d_loc.view(np.uint8).reshape(-1), r_loc.view(np.uint8).reshape(-1))
        p_val = case.input("values", d_val.view(np.uint8), r_val.view(np.uint8))
        p_rec, p_st = case.output("records", len(probes) * 8), case.output("statuses", len(probes))
        third = torch.cuda.Stream()
        counts = []

        def call():
            m.set_cells_device(p_loc, N, d_values=p_val, stream=case.side.cuda_stream)
            counts.append(m.update_components(flags, stream=streams[1].cuda_stream))
            m.get_device(d_probes.data_ptr(), len(probes), p_rec, p_st, stream=third.cuda_stream)
            third.synchronize()                                                # (the consumer below reads on the side stream)
        case.warm(call)
        case.arm()
        call()
        case.consume()
        got = case.finish()
        ref.set_cells(d_loc, d_val)
        decoy_count = C.apply(ref, flags)
        decoy_rec, _ = ref.get_batch(probes)
        ref.set_cells(r_loc, r_val)
        want_count = C.apply(ref, flags)
        want_rec, want_st = ref.get_batch(probes)
        assert counts == [decoy_count, decoy_count, want_count] and want_count > 3
        assert m.components_info() == (want_count, flags, True)
        H.expect("the records a Get on a third stream sees", H.view(got["records"], np.uint64), want_rec, decoy_rec)
        H.expect("its statuses", got["statuses"], want_st)
        chunks, cells = m.export()
        want_chunks, want_cells = ref.export()
        assert [tuple(c) for c in chunks["c"]] == [w[0] for w in want_chunks] and np.array_equal(cells, want_cells)
    finally:
        m.close()
