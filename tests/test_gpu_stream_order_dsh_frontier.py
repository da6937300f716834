"""GPU: sdfgpu_dsh_frontier_window_device, sdfgpu_dsh_frontier_cells_device and sdfgpu_component_stats_device on a NON-BLOCKING side
stream whose inputs arrive late (tests/stream_harness.py, as tests/test_gpu_stream_order_dsh.py does for the window and the export).

For the two frontier forms the input that arrives late is the map's content: a cell batch on the same stream, in front of the read,
whose locations and values hold decoys until the real ones are copied over them behind a measured delay.  For the statistics it is
the bit field and the labels themselves.  The results must be those of the real input (the restatement,
tests/dsh_frontier_restated.py), and the witnesses on the null stream and on a second side stream must still hold the decoys."""
import numpy as np
import pytest

import dsh_frontier_restated as F
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


@pytest.mark.parametrize("what", ["window", "cells"])
@pytest.mark.parametrize("flags", [0, capi.DSH_FRONTIER_26])
def test_the_frontier_forms_see_the_sets_in_front_of_them_on_their_stream(gpu, delay, streams, what, flags):
    m, ref = gpu.dsh_create(None, 1.0, DIMS, DEFAULT), R.Map(None, 1.0, DIMS, DEFAULT)
    try:
        (d_loc, d_val), (r_loc, r_val) = operations(351, 5), operations(352, 9)
        lower, shape = (-7, -3, -9), (7, 6, 31)
        n_vox = int(np.prod(shape))
        case = H.Case(delay, streams[0], streams[1])
        p_loc = case.input("locations", d_loc.view(np.uint8).reshape(-1), r_loc.view(np.uint8).reshape(-1))
        p_val = case.input("values", d_val.view(np.uint8), r_val.view(np.uint8))
        s = case.side.cuda_stream
        capacity = 2 * N * 30
        p_out = case.output("bits", (n_vox + 31) // 32 * 4) if what == "window" else case.output("cells", capacity * 24)
        totals = []

        def call():
            m.set_cells_device(p_loc, N, d_values=p_val, stream=s)
            if what == "window":
                m.frontier_window_device(lower, shape, flags, p_out, stream=s)
            else:
                totals.append(m.frontier_cells_device(None, None, flags, p_out, capacity, stream=s))
        case.warm(call)
        case.arm()
        call()
        case.consume()
        got = case.finish()
        ref.set_cells(d_loc, d_val)
        ref.set_cells(d_loc, d_val)
        if what == "window":
            decoy = F.frontier_window_bits(ref, lower, shape, flags)
            ref.set_cells(r_loc, r_val)
            want = F.frontier_window_bits(ref, lower, shape, flags)
            assert int(np.unpackbits(want.view(np.uint8)).sum()) > 10
            H.expect("the bits", H.view(got["bits"], np.uint32), want, decoy)
        else:
            decoy = F.frontier_cells(ref, None, flags)
            ref.set_cells(r_loc, r_val)
            want = F.frontier_cells(ref, None, flags)
            assert totals[-1] == len(want) > 50 and totals[-2] == len(decoy) and len(want) <= capacity
            listed = H.view(got["cells"], np.int64)
            H.expect("the list", listed[:3 * len(want)], want.reshape(-1), decoy.reshape(-1)[:3 * len(want)] if len(decoy) >= len(want) else None)
            assert (got["cells"][24 * len(want):] == H.SENTINEL).all(), "nothing is written behind the list"
        chunks, cells = m.export()
        want_chunks, want_cells = ref.export()
        assert [tuple(c) for c in chunks["c"]] == [w[0] for w in want_chunks] and np.array_equal(cells, want_cells)
    finally:
        m.close()


def test_the_statistics_honour_their_stream(gpu, delay, streams):
    shape = (5, 3, 33)
    n = int(np.prod(shape))

    def scene(seed):
        filled = np.random.default_rng(seed).random(shape) < 0.55
        labels, count = gpu.components(filled)
        return filled, labels, count
    (d_filled, d_labels, d_count), (r_filled, r_labels, r_count) = scene(353), scene(354)
    label_count = max(d_count, r_count)
    case = H.Case(delay, streams[0], streams[1])
    p_bits = case.input("bits", R.pack_bits(d_filled).view(np.uint8), R.pack_bits(r_filled).view(np.uint8))
    p_labels = case.input("labels", d_labels.reshape(-1).view(np.uint8), r_labels.reshape(-1).view(np.uint8))
    p_stats = case.output("stats", label_count * 64)
    totals = []

    def call():
        totals.append(gpu.component_stats_device(p_bits, p_labels, shape, label_count, p_stats, label_count, stream=case.side.cuda_stream))
    case.warm(call)
    case.arm()
    call()
    case.consume()
    got = case.finish()
    want = F.component_stats_records(F.component_stats(r_filled, r_labels, shape, label_count), capi.COMPONENT_STATS_DTYPE)
    decoy = F.component_stats_records(F.component_stats(d_filled, d_labels, shape, label_count), capi.COMPONENT_STATS_DTYPE)
    assert totals[-1] == len(want) > 5 and totals[-2] == len(decoy) and n == 495
    k = min(len(want), len(decoy)) * 64
    H.expect("the records", got["stats"][:len(want) * 64], want.view(np.uint8).reshape(-1))
    assert not H.same(want.view(np.uint8).reshape(-1)[:k], decoy.view(np.uint8).reshape(-1)[:k]), "the decoy's records differ from the real input's"
    assert (got["stats"][len(want) * 64:] == H.SENTINEL).all(), "nothing is written behind the records"
