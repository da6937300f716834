"""GPU: sdfgpu_dsh_remove_chunks_device and sdfgpu_dsh_retain_box on a NON-BLOCKING side stream whose locations arrive late
(tests/stream_harness.py, as tests/test_gpu_stream_order_dsh_fusion.py does for a fused frame).

The locations hold decoys; behind a measured delay on the side stream the real ones are copied over them.  Every kernel, memset and
read-back of the removal -- the flags, the pairing scan, the moves, the table's clearing and its rehash -- must run on that stream: the
map must end in the state the restatement (tests/dsh_remove_restated.py) reaches through the same sequence (the harness's two warm
calls on the decoys, then the real one; each call is a removal by list, a retain_box and a Get of probe locations on the side stream),
the statuses and the counts must be the real list's, and the witnesses on the null stream and on a second side stream must still hold
the decoys."""
import numpy as np
import pytest

import dsh_remove_restated as X
import dsh_restated as R
import stream_harness as H

pytestmark = pytest.mark.gpu

DIMS, N = (3, 2, 5), 120
DEFAULT = R.record(0.5, 0x77)
BOXES = [(-4, 8), (-3, 6), (-3, 5)]                                          # chunks kept per axis by the box of call 0, 1 and 2: first, count


@pytest.fixture(scope="module")
def delay():
    return H.Delay()


@pytest.fixture(scope="module")
def streams(delay):
    return H.pick_streams(delay)


def centres(chunks, rng):
    n = np.array(DIMS)
    return (np.asarray(chunks) * n + rng.integers(0, n, (len(chunks), 3)) + 0.5).astype(np.float64)


@pytest.mark.parametrize("grow", [False, True], ids=["room-in-the-map", "grown-from-one-chunk"])
def test_removals_honour_their_stream(gpu, delay, streams, grow):
    """with `grow` the map starts with a 16-entry table and a one-chunk pool, so what the removals compact and rebuild was grown"""
    m = gpu.dsh_create(None, 1.0, DIMS, DEFAULT, initial_chunks=1 if grow else 4096)
    ref = R.Map(None, 1.0, DIMS, DEFAULT)
    try:
        rng = np.random.default_rng(5)
        side = np.arange(-5, 5)
        chunks = np.stack(np.meshgrid(side, side, side, indexing="ij"), -1).reshape(-1, 3)
        chunks = chunks[rng.permutation(len(chunks))]
        loc = centres(chunks, rng)
        values = rng.integers(1, 1 << 63, len(loc), dtype=np.uint64)
        for call, ref_call, s in ((m.set_chunks, ref.set_chunks, slice(None)), (m.set_cells, ref.set_cells, slice(0, None, 2))):
            call(loc[s], values[s])
            ref_call(loc[s], values[s])
        inner = chunks[(np.abs(chunks + 0.5) < 2).all(axis=1)]               # the 64 chunks that every box keeps
        assert len(inner) == 64
        names_decoy, names_real = inner[:30], inner[30:60]
        decoy = centres(names_decoy[rng.integers(0, 30, N)], rng)
        real = centres(names_real[rng.integers(0, 30, N)], rng)
        decoy[5], real[9] = np.nan, np.inf
        probe_locations = centres(chunks, rng)
        probes = H.to_device(probe_locations)

        case = H.Case(delay, streams[0], streams[1])
        p_loc = case.input("locations", decoy.view(np.uint8).reshape(-1), real.view(np.uint8).reshape(-1))
        p_st = case.output("statuses", N)
        p_found = case.output("found", len(chunks))
        removed = []

        def call():
            first, count = BOXES[len(removed)]
            lower, extent = [first * d for d in DIMS], [count * d for d in DIMS]
            by_list = m.remove_chunks_device(p_loc, N, d_statuses=p_st, stream=case.side.cuda_stream)
            removed.append((by_list, m.retain_box(lower, extent, stream=case.side.cuda_stream)))
            m.get_device(probes.data_ptr(), len(chunks), d_statuses=p_found, stream=case.side.cuda_stream)
        case.warm(call)
        case.arm()
        call()
        case.consume()
        got = case.finish()

        want_removed, statuses = [], []
        for k, locations in enumerate([decoy, decoy, real]):
            first, count = BOXES[k]
            statuses.append(X.remove_chunks(ref, locations))
            want_removed.append((int(statuses[-1].sum()), X.retain_box(ref, [first * d for d in DIMS], [count * d for d in DIMS])))
        assert removed == want_removed, "(by list, by box) of the two warm calls and the real one"
        assert want_removed[0][0] > 20 and want_removed[1][0] == 0 and want_removed[2][0] > 20 and all(r[1] > 0 for r in want_removed)
        H.expect("the statuses", H.view(got["statuses"], np.uint8), statuses[2], statuses[1])
        want_found = ref.get_batch(probe_locations)[1]
        assert np.array_equal(H.view(got["found"], np.uint8)[:len(chunks)], want_found) and 0 < want_found.sum() < len(chunks)
        got_chunks, cells = m.export()
        want, want_cells = ref.export()
        assert [tuple(c) for c in got_chunks["c"]] == [w[0] for w in want] and got_chunks["state"].tolist() == [w[1] for w in want]
        assert np.array_equal(got_chunks["record"], np.array([w[2] for w in want], np.uint64)) and np.array_equal(cells, want_cells)
    finally:
        m.close()
