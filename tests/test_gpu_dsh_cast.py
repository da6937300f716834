"""GPU: ray casts through the dynamic spatial hashed map (sdfgpu_dsh_cast_*, include/sdfgpu.h "Ray casts")
against the restatement of their contract (tests/dsh_cast_restated.py on a tests/dsh_restated.py map): the statuses and all 48 bytes of
every hit record compared, no ray excused, and the map's export and info compared around every cast."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dsh_cast_restated as C
import dsh_restated as R
import dsh_rays_restated as RR
from sdf_tools_amd import capi
from test_gpu_dsh import Pair, rigid
from test_gpu_dsh_rays import FRAMES, SHAPES, random_frame, to_world

pytestmark = pytest.mark.gpu

FREE, FILLED, UNKNOWN = R.record(0.0, 0x10), R.record(1.0, 0x20), R.record(0.5, 0x30)
NAN_CELL = R.record_bits(0x7FC00001, 5)                                       # a NaN occupancy never blocks
DEFAULTS = [R.record(0.5, 0xABCD), R.record(0.0, 0xABCE), R.record(1.0, 0xABCF)]
ALL_FLAGS = range(8)


class CastPair(Pair):
    """the map on the GPU and its restatement; every cast is compared with the restatement's and must leave the map as it was"""

    def snapshot(self):
        chunks, cells = self.gpu.export()
        return chunks.tobytes(), cells.tobytes(), self.gpu.info()

    def unchanged(self, before, host_form, what):
        after = self.snapshot()
        assert after[:2] == before[:2], what + ": the cast changed the map's export"
        staged = ("scratch_bytes",) if host_form else ()                       # (a host form's first call may grow the staging buffer)
        assert {k: v for k, v in after[2].items() if k not in staged} == {k: v for k, v in before[2].items() if k not in staged}, what + ": info"

    def compare(self, got, traces, flags, what):
        want_st, want_hits = C.decide_all(traces, flags)
        st, hits = got
        if st is not None:
            assert np.array_equal(st, want_st), "%s: statuses differ at %s" % (what, np.flatnonzero(st != want_st)[:5])
        if hits is not None:
            bad = np.flatnonzero((hits.view(np.uint8).reshape(-1, 48) != want_hits.view(np.uint8).reshape(-1, 48)).any(1))
            assert len(bad) == 0, "%s: %d hit records differ, first ray %d: got %r, want %r" % (what, len(bad), bad[0], hits[bad[0]], want_hits[bad[0]])
        return want_st, want_hits

    def cast_rays(self, sensor, points, max_range, flags, traces=None, what="", **kw):
        before = self.snapshot()
        got = self.gpu.cast_rays(sensor, points, max_range, flags, **kw)
        self.unchanged(before, True, what)
        traces = C.trace_rays(self.ref, sensor, points, max_range) if traces is None else traces
        return self.compare(got, traces, flags, what) + (traces,)

    def cast_segments(self, starts, ends, max_range, flags, traces=None, what="", **kw):
        before = self.snapshot()
        got = self.gpu.cast_segments(starts, ends, max_range, flags, **kw)
        self.unchanged(before, True, what)
        traces = C.trace_segments(self.ref, starts, ends, max_range) if traces is None else traces
        return self.compare(got, traces, flags, what) + (traces,)


@pytest.fixture
def pair(gpu):
    made = []

    def make(**kw):
        made.append(CastPair(gpu, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


def build_scene(p, rng, origin, cell, dims, half, keep_free):
    """Chunks of all three states within `half` cells of the grid's origin: of the chunks there about half chunk-filled free, a tenth
    chunk-filled blocking, the rest absent; then single cells of every kind, which make cell-filled chunks out of all three; the
    chunks of `keep_free` (world locations: where rays start) are chunk-filled free at the end."""
    n = np.array(dims)
    lo, hi = np.floor(-half / n).astype(int), np.floor(half / n).astype(int)
    coords = np.stack(np.meshgrid(*[np.arange(l, h + 1) for l, h in zip(lo, hi)], indexing="ij"), -1).reshape(-1, 3)
    kind = rng.random(len(coords))
    centre = lambda c: to_world(origin, (c + 0.5) * n, cell)
    p.set_chunks(centre(coords[kind < 0.5]), FREE)
    blocking = coords[(kind >= 0.5) & (kind < 0.6)]
    p.set_chunks(centre(blocking), np.array([R.record(0.75 + 0.01 * (k % 20), k) for k in range(len(blocking))], np.uint64))
    cells = rng.integers(-half, half, (len(coords) // 2 + 20, 3)) + 0.5
    kinds = [FILLED, FREE, UNKNOWN, FILLED, NAN_CELL, FREE]
    p.set_cells(to_world(origin, cells, cell), np.array([kinds[k % 6] for k in range(len(cells))], np.uint64))
    p.set_chunks(keep_free, FREE)


def random_segments(rng, origin, cell, n, half, reach):
    s = rng.uniform(-half, half, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    e = s + d * rng.uniform(0.0, reach, (n, 1))
    return to_world(origin, s, cell), to_world(origin, e, cell)


def one_case(make, dims, frame, n_rays=500):
    """Three maps (defaults 0.5, 0.0, 1.0), each cast through in both forms under all eight flag combinations.  Returns the case's
    statuses and the found states of its blockers, for the conditions that keep it from being trivial."""
    origin, inverse, cell = FRAMES[frame]
    reach = 14 if dims == (1, 1, 1) else 30
    half = reach // 2 if max(dims) <= 5 else reach                             # (a few chunks across, whatever their size)
    seen_status, seen_found = [], []
    for k, default in enumerate(DEFAULTS):
        rng = np.random.default_rng(330 + k)
        p = make(inverse=inverse, cell_size=cell, chunk_dims=dims, default=default)
        sensor, pts = random_frame(rng, origin, cell, n_rays, reach)
        starts, ends = random_segments(rng, origin, cell, n_rays, half, reach)
        build_scene(p, rng, origin, cell, dims, half, np.concatenate([sensor[None], starts[:4]]))
        max_range = reach * 0.6 * cell
        ray_traces = seg_traces = None
        for flags in ALL_FLAGS:
            st, hits, ray_traces = p.cast_rays(sensor, pts, max_range, flags, ray_traces, "default %d, rays, flags %d" % (k, flags))
            st2, hits2, seg_traces = p.cast_segments(starts, ends, max_range, flags, seg_traces, "default %d, segments, flags %d" % (k, flags))
            for s, h in ((st, hits), (st2, hits2)):
                seen_status.append(s)
                seen_found.append(h["found"][s == C.CAST_BLOCKED])
    return np.concatenate(seen_status), np.concatenate(seen_found)


# ---- shapes, frames, defaults, flags ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_random_casts_in_every_chunk_shape(pair, dims, frame):
    status, found = one_case(pair, dims, frame)
    assert len(status) == 3 * 2 * 8 * 500
    # the conditions under which the case says something (the restatement alone decides them: the GPU's output equals it by now)
    assert (status == C.CAST_BLOCKED).sum() >= len(status) // 4
    assert (status == C.CAST_CLEAR).sum() >= 50 and (status == C.CAST_CLEAR_IN_RANGE).sum() >= 50
    for state in (R.NOT_FOUND, R.FOUND_IN_CHUNK, R.FOUND_IN_CELL):
        assert (found == state).sum() >= 20, "blockers found as %d" % state


# ---- special rays --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [1.0, 0.25])
def test_tie_rays_face_rays_and_rays_between_cell_and_chunk_boundaries(pair, cell):
    dims = (3, 2, 5)
    p = pair(cell_size=cell, chunk_dims=dims, default=DEFAULTS[0])
    rng = np.random.default_rng(331)
    build_scene(p, rng, np.eye(4), cell, dims, 12, np.zeros((1, 3)))
    # the hand-worked rays of tests/test_dsh_rays_cpu.py, in both forms, under every flag combination
    hand = [((0.5, 0.5, 0.5), (8.5, 8.5, 8.5)), ((0.5, 1.0, 0.5), (4.5, 1.0, 0.5)), ((0.5, 2.0, 0.5), (2.5, 2.0, 2.5)), ((2.0, 2.0, 2.0), (-0.5, -0.5, -0.5)),
            ((0.25, 0.25, 0.25), (0.75, 0.5, 0.25))]
    starts, ends = np.array([h[0] for h in hand]) * cell, np.array([h[1] for h in hand]) * cell
    seg_traces = None
    for flags in ALL_FLAGS:
        _, hits, seg_traces = p.cast_segments(starts, ends, 100.0 * cell, flags, seg_traces, "hand-worked, flags %d" % flags)
        for k in range(len(hand)):
            st, ray_hits, _ = p.cast_rays(starts[k], ends[k:k + 1].astype(np.float32), 100.0 * cell, flags, None, "hand-worked ray %d, flags %d" % (k, flags))
            assert ray_hits.tobytes() == hits[k:k + 1].tobytes(), "the two forms agree on a ray both can express"
    # sensors and ends exactly on cell and chunk boundaries on both sides of zero: every combination of a few lattice values per axis
    axes = [np.array(sorted({0, 1, -1, n, -n, n + 1, -n - 1, 2 * n, -2 * n}), np.float64) for n in dims]
    lattice = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    blocked = 0
    for k in range(6):
        sensor = lattice[rng.integers(len(lattice))] * cell
        pts = (lattice[rng.permutation(len(lattice))[:250]] * cell).astype(np.float32)
        max_range, flags = (4.0, 9.0, 100.0)[k % 3] * cell, (0, 4, 1, 6, 3, 7)[k]
        st, _, _ = p.cast_rays(sensor, pts, max_range, flags, None, "lattice rays %d" % k)
        other = lattice[rng.permutation(len(lattice))[:250]] * cell
        st2, _, _ = p.cast_segments(other, pts.astype(np.float64), max_range, flags, None, "lattice segments %d" % k)
        blocked += (st == C.CAST_BLOCKED).sum() + (st2 == C.CAST_BLOCKED).sum()
    assert blocked > 300


@pytest.mark.parametrize("range_cells", [0.3, 7.0, 65536.0])
def test_ranges_from_a_fraction_of_a_cell_to_the_largest(pair, range_cells):
    origin, inverse = rigid((0.7, -0.2, 0.4, 0.1), (0.1, 0.2, -0.3))
    cell = 0.25
    p = pair(inverse=inverse, cell_size=cell, chunk_dims=(3, 2, 5), default=DEFAULTS[1])
    rng = np.random.default_rng(332)
    sensor, pts = random_frame(rng, origin, cell, 500, 20.0)
    starts, ends = random_segments(rng, origin, cell, 500, 8, 20.0)
    build_scene(p, rng, origin, cell, (3, 2, 5), 10, sensor[None])
    for flags in (0, 5, 6):
        st, _, _ = p.cast_rays(sensor, pts, range_cells * cell, flags, None, "rays")
        st2, _, _ = p.cast_segments(starts, ends, range_cells * cell, flags, None, "segments")
        for s in (st, st2):
            if range_cells < 15:
                assert (s == C.CAST_CLEAR_IN_RANGE).sum() > 30
            if range_cells > 20:
                assert (s == C.CAST_CLEAR_IN_RANGE).sum() == 0 and (s == C.CAST_BLOCKED).sum() > 100 and (s == C.CAST_CLEAR).sum() > 30
    if range_cells < 1.0:
        assert (st == C.CAST_CLEAR).sum() >= 1, "no ray shorter than the range: the case does not cover the short clear ray"


def test_skipped_rays_inside_a_batch(pair):
    p = pair(chunk_dims=(3, 2, 5), default=DEFAULTS[0])
    p.set_cells([(3.5, 0.5, 0.5), (0.5, 4.5, 0.5)], FILLED)
    edge = float(1 << 20)
    pts = np.array([(5.5, 0.5, 0.5), (np.nan, 0.5, 0.5), (0.5, 6.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (-4.5, -3.5, 2.5), (edge * 3, 0.5, 0.5),
                    (0.5, -edge * 2 - 0.5, 0.5), (0.5, 0.5, edge * 5), (3e38, 0.5, 0.5), (0.5, 1.5, 0.5), (edge * 3 - 0.5, 0.5, 0.5)], np.float32)
    st, hits, _ = p.cast_rays((0.5, 0.5, 0.5), pts, 10.0, 0)
    assert st.tolist() == [3, 0, 3, 0, 0, 1, 0, 0, 0, 0, 1, 3]
    assert all(hits[k].tobytes() == bytes(48) for k in np.flatnonzero(st == 0))
    starts = np.tile((0.5, 0.5, 0.5), (len(pts), 1))
    starts[[0, 2, 5]] = [(np.nan, 0.5, 0.5), (0.5, edge * 2, 0.5), (0.5, 0.5, -np.inf)]  # an invalid start skips its ray only
    st2, hits2, _ = p.cast_segments(starts, pts.astype(np.float64), 10.0, 0)
    assert st2.tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 3] and hits2[:10].tobytes() == bytes(480)
    # far from zero: a walk along the last valid chunk of the x axis
    far = np.array([(edge * 3 - 0.5, 0.5, 0.5)], np.float64)
    st3, hits3, _ = p.cast_segments(far, far - (40.0, 0, 0), 100.0, 4)
    assert st3.tolist() == [3] and hits3["cell"][0].tolist() == [3 * (1 << 20) - 1, 0, 0] and hits3["found"][0] == R.NOT_FOUND


def test_refusals_change_nothing(pair):
    p = pair(chunk_dims=(3, 2, 5), default=DEFAULTS[0])
    p.set_cells([(3.5, 0.5, 0.5)], FILLED)
    pts = np.array([(5.5, 0.5, 0.5)], np.float32)
    ok = (0.5, 0.5, 0.5)
    before = p.snapshot()
    calls = [lambda: p.gpu.cast_rays((np.nan, 0.5, 0.5), pts, 10.0), lambda: p.gpu.cast_rays((0.5, -np.inf, 0.5), pts, 10.0),
             lambda: p.gpu.cast_rays((float(1 << 20) * 3, 0.5, 0.5), pts, 10.0),
             lambda: p.gpu.cast_rays(ok, pts, 0.0), lambda: p.gpu.cast_rays(ok, pts, 65536.5), lambda: p.gpu.cast_rays(ok, pts, np.nan),
             lambda: p.gpu.cast_rays(ok, pts, 10.0, 8), lambda: p.gpu.cast_rays(ok, pts, 10.0, 1 << 31),
             lambda: p.gpu.cast_rays(ok, pts, 10.0, 0, statuses=False, hits=False),
             lambda: p.gpu.cast_segments([ok], pts, 0.0), lambda: p.gpu.cast_segments([ok], pts, 65536.5), lambda: p.gpu.cast_segments([ok], pts, np.nan),
             lambda: p.gpu.cast_segments([ok], pts, 10.0, 8), lambda: p.gpu.cast_segments([ok], pts, 10.0, 0, statuses=False, hits=False),
             lambda: p.gpu.cast_rays((np.nan, 0.5, 0.5), pts[:0], 10.0), lambda: p.gpu.cast_segments(pts[:0], pts[:0], 10.0, 8),
             lambda: p.gpu.cast_rays_device(ok, 0, 0, 10.0, 0, 0, 0), lambda: p.gpu.cast_segments_device(0, 0, 0, 0.0, 0, 1, 0)]
    for k, call in enumerate(calls):
        with pytest.raises(capi.SdfGpuError) as e:
            call()
        assert e.value.code == -1, "call %d: %s" % (k, e.value)
    for sensor, max_range, flags in [((np.nan, 0.5, 0.5), 10.0, 0), (ok, 0.0, 0), (ok, 65536.5, 0), (ok, np.nan, 0), (ok, 10.0, 8)]:
        with pytest.raises(C.Refused):
            C.cast_rays(p.ref, sensor, pts, max_range, flags)
    p.unchanged(before, False, "refusals")
    p.cast_rays(ok, pts, 65536.0, 7)


def test_no_ray_one_ray_and_one_output(pair):
    p = pair(chunk_dims=(3, 2, 5), default=DEFAULTS[0])
    p.set_cells([(3.5, 0.5, 0.5)], FILLED)
    ok = (0.5, 0.5, 0.5)
    st, hits = p.gpu.cast_rays(ok, np.zeros((0, 3), np.float32), 5.0)
    assert len(st) == 0 and len(hits) == 0
    st, hits = p.gpu.cast_segments(np.zeros((0, 3)), np.zeros((0, 3)), 5.0)
    assert len(st) == 0 and len(hits) == 0
    p.gpu.cast_rays_device(ok, 0, 0, 5.0, 0, 1, 0)                             # no ray: no buffer is touched
    p.gpu.cast_segments_device(0, 0, 0, 5.0, 0, 0, 8)
    st, hits, _ = p.cast_rays(ok, [(-6.5, 0.5, 0.5)], 50.0, 0)
    assert st.tolist() == [1] and hits["cell"][0].tolist() == [-7, 0, 0] and hits["step"][0] == 7
    st, hits, _ = p.cast_segments([ok], [(6.5, 0.5, 0.5)], 50.0, 0)
    assert st.tolist() == [3] and hits["cell"][0].tolist() == [3, 0, 0] and hits["record"][0] == FILLED and hits["t"][0] == 2.5 / 6
    pts = np.array([(6.5, 0.5, 0.5), (0.5, 6.5, 0.5), (np.nan, 0, 0)], np.float32)
    for kw in ({"hits": False}, {"statuses": False}):
        st, hits, _ = p.cast_rays(ok, pts, 4.0, 0, None, str(kw), **kw)
        assert (p.gpu.cast_rays(ok, pts, 4.0, 0, **kw)[0] is None) == ("statuses" in kw)
        st, hits, _ = p.cast_segments(np.tile(ok, (3, 1)), pts.astype(np.float64), 4.0, 0, None, str(kw), **kw)
        assert st.tolist() == [3, 2, 0]


# ---- what a cast means ----------------------------------------------------------------------------------------------------------------------
def test_a_cast_along_an_inserted_ray_is_blocked_at_its_end_cell(pair):
    p = pair(chunk_dims=(4, 4, 4), default=DEFAULTS[0])
    sensor, pts = (0.3, 0.6, 0.2), np.array([(9.7, -5.2, 3.4)], np.float32)
    st, counts = p.gpu.insert_rays(sensor, pts, 50.0, FREE, FILLED)
    RR.insert_rays(p.ref, sensor, pts, 50.0, FREE, FILLED)
    n_steps = counts["cells_carved"]
    assert st.tolist() == [capi.DSH_RAY_HIT] and n_steps == 9 + 6 + 3
    st, hits, _ = p.cast_rays(sensor, pts, 50.0, 0)
    assert st.tolist() == [C.CAST_BLOCKED] and hits["step"][0] == n_steps and hits["cell"][0].tolist() == [9, -6, 3] and hits["record"][0] == FILLED
    assert hits["found"][0] == R.FOUND_IN_CELL
    st, hits, _ = p.cast_rays(sensor, pts, 50.0, C.SKIP_LAST)
    assert st.tolist() == [C.CAST_CLEAR] and hits["step"][0] == n_steps, "the carved cells are free, the unknown around them is never visited"
    p.cast_segments(pts.astype(np.float64), [sensor], 50.0, C.SKIP_FIRST | C.UNKNOWN_IS_FILLED, None, "the way back")   # (another walk: the restatement judges it)


def test_the_first_set_bit_of_an_extracted_window_along_the_walk_is_the_blocker(pair):
    origin, inverse, cell = FRAMES["rotated-quarter"]
    dims = (3, 2, 5)
    p = pair(inverse=inverse, cell_size=cell, chunk_dims=dims, default=DEFAULTS[0])
    rng = np.random.default_rng(333)
    sensor, pts = random_frame(rng, origin, cell, 400, 14.0)
    build_scene(p, rng, origin, cell, dims, 8, sensor[None])
    lower, shape = (-20, -20, -20), (40, 40, 40)
    for flags in (0, C.UNKNOWN_IS_FILLED | C.SKIP_FIRST):
        st, hits = p.gpu.cast_rays(sensor, pts, 12.0 * cell, flags)
        _, words = p.gpu.extract_window(lower, shape, bool(flags & C.UNKNOWN_IS_FILLED), records=False, bits=True)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:np.prod(shape)].reshape(shape).astype(bool)
        gs, i0 = RR.grid_coordinates(p.ref, sensor)
        seen = 0
        for k, point in enumerate(pts.astype(np.float64)):
            ge, i1 = RR.grid_coordinates(p.ref, point)
            len2, first = RR.length2(gs, ge), None
            for j, (c, t) in enumerate(RR.steps(gs, ge, i0, i1)):
                if len2 > 144.0 and not (t * t) * len2 <= 144.0:
                    break
                if not (j == 0 and flags & C.SKIP_FIRST) and bits[tuple(np.subtract(c, lower))]:
                    first = (list(c), j)
                    break
            assert (st[k] == C.CAST_BLOCKED) == (first is not None), k
            if first is not None:
                assert (hits["cell"][k].tolist(), int(hits["step"][k])) == first, k
                seen += 1
        assert seen > 100


# ---- the device forms ---------------------------------------------------------------------------------------------------------------------------
def test_device_forms_on_buffers_at_natural_but_not_16_byte_alignment(pair):
    origin, inverse, cell = FRAMES["rotated-quarter"]
    dims = (4, 4, 4)
    p = pair(inverse=inverse, cell_size=cell, chunk_dims=dims, default=DEFAULTS[2])
    rng = np.random.default_rng(334)
    n = 777
    sensor, pts = random_frame(rng, origin, cell, n, 20.0)
    starts, ends = random_segments(rng, origin, cell, n, 8, 20.0)
    build_scene(p, rng, origin, cell, dims, 10, np.concatenate([sensor[None], starts[:4]]))
    stream = torch.cuda.current_stream().cuda_stream
    raw_pts = torch.zeros(n * 12 + 16, dtype=torch.uint8, device="cuda")
    raw_starts, raw_ends = (torch.zeros(n * 24 + 16, dtype=torch.uint8, device="cuda") for _ in range(2))
    raw_hits = torch.full((n * 48 + 16 + 48,), 0xEE, dtype=torch.uint8, device="cuda")
    raw_st = torch.full((n + 16 + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    assert raw_pts.data_ptr() % 16 == 0 and raw_hits.data_ptr() % 16 == 0 and raw_st.data_ptr() % 16 == 0 and raw_starts.data_ptr() % 16 == 0
    raw_pts[4:4 + n * 12] = torch.from_numpy(pts.view(np.uint8).reshape(-1)).cuda()
    raw_starts[8:8 + n * 24] = torch.from_numpy(starts.view(np.uint8).reshape(-1)).cuda()
    raw_ends[8:8 + n * 24] = torch.from_numpy(ends.view(np.uint8).reshape(-1)).cuda()
    max_range = 14.0 * cell
    for form in ("rays", "segments"):
        traces = C.trace_rays(p.ref, sensor, pts, max_range) if form == "rays" else C.trace_segments(p.ref, starts, ends, max_range)
        for flags in (0, 3, 4):
            raw_hits.fill_(0xEE)
            raw_st.fill_(0xEE)
            before = p.snapshot()
            if form == "rays":
                p.gpu.cast_rays_device(sensor, raw_pts.data_ptr() + 4, n, max_range, flags, raw_st.data_ptr() + 1, raw_hits.data_ptr() + 8, stream)
            else:
                p.gpu.cast_segments_device(raw_starts.data_ptr() + 8, raw_ends.data_ptr() + 8, n, max_range, flags, raw_st.data_ptr() + 1, raw_hits.data_ptr() + 8,
                                           stream)
            torch.cuda.synchronize()
            p.unchanged(before, False, "%s on the device, flags %d" % (form, flags))
            st, hits = raw_st.cpu().numpy(), raw_hits.cpu().numpy()
            assert (st[:1] == 0xEE).all() and (st[1 + n:] == 0xEE).all() and (hits[:8] == 0xEE).all() and (hits[8 + n * 48:] == 0xEE).all(), "bytes beside the outputs"
            want_st, _ = p.compare((st[1:1 + n], hits[8:8 + n * 48].copy().view(capi.DSH_CAST_HIT_DTYPE)), traces, flags, "%s on the device, flags %d" % (form, flags))
            assert (want_st == C.CAST_BLOCKED).sum() > 100
    # misaligned buffers are refused: points off 4 bytes, hits off 8, starts off 8
    for call in (lambda: p.gpu.cast_rays_device(sensor, raw_pts.data_ptr() + 2, n, max_range, 0, raw_st.data_ptr(), 0, stream),
                 lambda: p.gpu.cast_rays_device(sensor, raw_pts.data_ptr(), n, max_range, 0, 0, raw_hits.data_ptr() + 4, stream),
                 lambda: p.gpu.cast_segments_device(raw_starts.data_ptr() + 4, raw_ends.data_ptr(), n, max_range, 0, raw_st.data_ptr(), 0, stream),
                 lambda: p.gpu.cast_segments_device(raw_starts.data_ptr(), raw_ends.data_ptr() + 4, n, max_range, 0, raw_st.data_ptr(), 0, stream)):
        with pytest.raises(capi.SdfGpuError) as e:
            call()
        assert e.value.code == -1 and "aligned" in str(e.value)


# ---- red zones -------------------------------------------------------------------------------------------------------------------------------
def core_cases_on(ctx):
    made = []

    def make(**kw):
        made.append(CastPair(ctx, **kw))
        return made[-1]
    try:
        one_case(make, (3, 2, 5), "rotated-quarter", 200)
        one_case(make, (8, 8, 32), "identity", 200)
        test_tie_rays_face_rays_and_rays_between_cell_and_chunk_boundaries(make, 0.25)
        test_skipped_rays_inside_a_batch(make)
        test_refusals_change_nothing(make)
        test_no_ray_one_ray_and_one_output(make)
        test_a_cast_along_an_inserted_ray_is_blocked_at_its_end_cell(make)
        test_device_forms_on_buffers_at_natural_but_not_16_byte_alignment(make)
    finally:
        for p in made:
            p.close()


def test_the_core_cases_in_a_child_process_with_red_zones_from_the_environment():
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from sdf_tools_amd import capi\nimport test_gpu_dsh_cast as T\n"
            "ctx = capi.SdfGpu(0)\nT.core_cases_on(ctx)\nctx.redzone_check()\nctx.close()\nprint('core cases clean')\n") % (tests, os.path.dirname(tests))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SDFGPU_REDZONE="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "core cases clean" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
