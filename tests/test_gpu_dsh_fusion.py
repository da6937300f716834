"""GPU: a frame of sensor rays fused into the dynamic spatial hashed map as occupancy probabilities (sdfgpu_dsh_fuse_rays*,
include/sdfgpu.h "Sensor rays: fusion") against the restatement of its contract (tests/dsh_fusion_restated.py on a
tests/dsh_restated.py map): the full export, the statuses and the counts compared byte for byte, no cell excused."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dsh_restated as R
import dsh_rays_restated as RR
import dsh_fusion_restated as F
from sdf_tools_amd import capi
from test_gpu_dsh import Pair
from test_gpu_dsh_rays import FRAMES, random_frame, to_world

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 2, 5), (3, 3, 5), (4, 4, 4), (8, 8, 32), (32, 32, 32)]
DEFAULT = R.record(0.5, 0xABCD)                                              # unknown
MODEL = F.DEFAULT_MODEL
OTHER_MODEL = (0.9, 0.45, 0.2, 0.8)


def fused(prior, *measurements, model=MODEL, component=0xABCD):
    """the record of a cell that held occupancy `prior` after the measurements ('hit' / 'miss') in turn"""
    p = prior
    for m in measurements:
        p = F.fuse(p, model[0] if m == "hit" else model[1], model[2], model[3])
    return R.record(p, component)


class FusePair(Pair):
    """the map on the GPU and its restatement, driven together by fused frames"""

    def __init__(self, ctx, default=DEFAULT, **kw):
        Pair.__init__(self, ctx, default=default, **kw)

    def fuse_rays(self, sensor, points, max_range, model=None, what=""):
        st, counts = self.gpu.fuse_rays(sensor, points, max_range, model)
        want_st, want_counts = F.fuse_rays(self.ref, sensor, points, max_range, model)
        assert np.array_equal(st, want_st), what + ": ray statuses"
        assert counts == want_counts, what + ": counts"
        return st, counts

    def refused(self, sensor, points, max_range, model=None, code=-1):
        before = self.gpu.info()
        with pytest.raises(capi.SdfGpuError) as e:
            self.gpu.fuse_rays(sensor, points, max_range, model)
        assert e.value.code == code, str(e.value)
        after = self.check("refused")
        assert (after["bytes_held"], after["table_capacity"], after["capacity_chunks"]) == (before["bytes_held"], before["table_capacity"], before["capacity_chunks"])
        return str(e.value)


@pytest.fixture
def pair(gpu):
    made = []

    def make(**kw):
        made.append(FusePair(gpu, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


# ---- shapes and frames -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_random_frames_in_every_chunk_shape(pair, dims, frame):
    origin, inverse, cell = FRAMES[frame]
    p = pair(inverse=inverse, cell_size=cell, chunk_dims=dims)
    rng = np.random.default_rng(41)
    reach = 14 if dims == (1, 1, 1) else 30
    for k, (n_rays, max_cells, model) in enumerate([(600, reach * 0.7, None), (200, reach * 2.0, OTHER_MODEL), (150, reach * 0.5, None)]):
        sensor, pts = random_frame(rng, origin, cell, n_rays, reach)
        st, counts = p.fuse_rays(sensor, pts, max_cells * cell, model, what="frame %d" % k)
        assert counts["rays_hit"] > 25 and (k == 1 or counts["rays_truncated"] > 25) and counts["cells_carved"] > 4 * n_rays
        p.check("frame %d" % k)
    p.check_get(to_world(origin, rng.uniform(-35, 35, (300, 3)), cell))
    occ = R.occupancy(p.gpu.export()[1])
    assert len(np.unique(occ)) > 4, "cells seen once, twice and three times, hit and missed, must differ"


# ---- what a frame means ----------------------------------------------------------------------------------------------------------------------
def test_a_fan_of_rays_updates_the_cells_they_share_once(pair):
    p = pair(chunk_dims=(4, 4, 4))
    fan = np.array([(30.5, y + 0.5, z + 0.5) for y in range(-8, 9) for z in range(-8, 9)], np.float32)      # 289 rays from one cell
    st, counts = p.fuse_rays((0.5, 0.5, 0.5), fan, 100.0)
    assert (st == capi.DSH_RAY_HIT).all() and counts["cells_carved"] > 289 * 30
    rec, _ = p.gpu.get([(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (2.5, 0.5, 0.5), (30.5, 0.5, 0.5), (31.5, 0.5, 0.5)])
    assert rec.tolist() == [fused(0.5, "miss")] * 3 + [fused(0.5, "hit"), DEFAULT], "the sensor's cell lies on every ray and is updated once"
    p.check()
    p.fuse_rays((0.5, 0.5, 0.5), fan, 100.0)
    rec, _ = p.gpu.get([(0.5, 0.5, 0.5), (30.5, 0.5, 0.5)])
    assert rec.tolist() == [fused(0.5, "miss", "miss"), fused(0.5, "hit", "hit")]
    p.check("the same fan again")


def test_a_hit_beats_the_misses_and_two_hits_on_one_cell_count_once(pair):
    p = pair(chunk_dims=(4, 4, 4))
    line = np.array([(x + 0.5, 0.5, 0.5) for x in (2, 4, 4, 7, 11, 11, 11, 2)], np.float32)
    fan = np.array([(11.5, y + 0.5, 0.5) for y in range(-3, 4)], np.float32)
    st, counts = p.fuse_rays((0.5, 0.5, 0.5), np.concatenate([line, fan, line[::-1]]), 50.0)
    assert (st == capi.DSH_RAY_HIT).all() and counts["cells_carved"] == 2 * (2 + 4 + 4 + 7 + 11 * 3 + 2) + sum(11 + abs(y) for y in range(-3, 4))
    rec, _ = p.gpu.get([(x + 0.5, 0.5, 0.5) for x in range(13)])
    assert rec.tolist() == [fused(0.5, "hit") if x in (2, 4, 7, 11) else fused(0.5, "miss") if x < 11 else DEFAULT for x in range(13)]
    p.check()


def test_rays_along_z_both_ways_and_along_x_across_chunk_boundaries(pair):
    for dims in [(3, 3, 5), (4, 4, 16), (8, 8, 32)]:
        p = pair(chunk_dims=dims)
        nz = dims[2]
        ends = [(0.5, 0.5, 2.5 * nz + 0.5), (0.5, 0.5, -2.5 * nz - 0.5), (3 * dims[0] + 1.5, 0.5, 0.5), (-2 * dims[0] - 0.5, 0.5, 0.5), (1.5, 1.5, 3 * nz + 0.5),
                (0.5, 0.5, 1000.5)]
        st, counts = p.fuse_rays((0.5, 0.5, 0.5), np.array(ends, np.float32), 4.0 * nz)
        assert st.tolist() == [1, 1, 1, 1, 1, 2]
        rec, _ = p.gpu.get([(0.5, 0.5, 0.5), (0.5, 0.5, nz + 0.5), (0.5, 0.5, -nz - 0.5), (dims[0] + 0.5, 0.5, 0.5), (3 * dims[0] + 1.5, 0.5, 0.5), (0.5, 0.5, 4 * nz + 0.5),
                            (0.5, 0.5, 4 * nz + 1.5)])
        assert rec.tolist() == [fused(0.5, "miss")] * 4 + [fused(0.5, "hit"), fused(0.5, "miss"), DEFAULT]
        p.check("%r" % (dims,))


def test_truncated_and_skipped_rays_inside_a_frame(pair):
    p = pair(chunk_dims=(3, 3, 5))
    edge = float(1 << 20)
    pts = np.array([(5.5, 0.5, 0.5), (np.nan, 0.5, 0.5), (0.5, 6.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (-4.5, -3.5, 2.5), (edge * 3, 0.5, 0.5),
                    (0.5, -edge * 3 - 0.5, 0.5), (0.5, 0.5, edge * 5), (3e38, 0.5, 0.5), (0.5, 1.5, 0.5), (edge * 3 - 0.5, 0.5, 0.5), (0.5, 0.5, 40.5)], np.float32)
    st, counts = p.fuse_rays((0.5, 0.5, 0.5), pts, 10.0)
    assert st.tolist() == [1, 0, 1, 0, 0, 1, 0, 0, 0, 0, 1, 2, 2] and counts["rays_skipped"] == 7
    p.check("skips")
    rec, _ = p.gpu.get([(0.5, 0.5, 10.5), (0.5, 0.5, 11.5)])
    assert rec.tolist() == [fused(0.5, "miss"), DEFAULT], "a long ray updates the in-range prefix and hits nothing"


def test_rays_through_absent_chunk_filled_and_cell_filled_chunks_in_one_frame(pair):
    dims = (3, 2, 5)
    p = pair(chunk_dims=dims)
    n = np.array(dims, np.float64)
    nan_record = R.record_bits(0x7FC00001, 5)
    chunk_records = [R.record(1.0, 0x11111111), R.record(0.5, 0x22222222), nan_record, R.record(0.25, 0x33333333), R.record(1.0, 4), R.record(-0.0, 0x55555555)]
    rng = np.random.default_rng(44)
    loc = rng.uniform(-4, 10, (80, 3))
    priors = [R.record_bits(0x7FC00001, 7), R.record_bits(0xFFC12345, 8), R.record(0.0, 9), R.record(-0.0, 10), R.record(1.0, 11), R.record(0.05, 12), R.record(0.99, 13),
              R.record(np.inf, 14), R.record(-np.inf, 15), R.record(-3.0, 16), R.record(1e-40, 17), R.record(0.6, 0xFFFFFFFF)]
    p.set_cells(loc, np.array([priors[k % len(priors)] for k in range(len(loc))], np.uint64))
    p.set_chunks([(np.array(c) + 0.5) * n for c in [(1, 0, 0), (2, 1, 0), (-1, -1, -1), (0, 3, 0), (30, 30, 30), (0, 0, 1)]], np.array(chunk_records, np.uint64))
    states_before = {c: k for c, (k, _) in p.ref.chunks.items()}
    components_before = {c: int(w) >> 32 for c, (k, w) in p.ref.chunks.items() if k == "chunk"}
    sensor, pts = random_frame(rng, np.eye(4), 1.0, 500, 12.0)
    before = {c: w.copy() for c, (k, w) in p.ref.chunks.items() if k == "cells"}
    p.fuse_rays(sensor, pts, 9.0)
    became_cells = {states_before.get(c, "absent") for c, (k, _) in p.ref.chunks.items() if k == "cells"}
    assert became_cells == {"absent", "chunk", "cells"}, "the frame must cross chunks of all three states"
    assert p.ref.chunks[(30, 30, 30)][0] == "chunk", "a chunk-filled chunk no ray crosses stays chunk-filled"
    spread = [c for c, comp in components_before.items() if p.ref.chunks[c][0] == "cells"]
    assert len(spread) >= 3
    for c in spread:                                                          # the chunk record's component word survives in every cell
        assert (p.ref.chunks[c][1] >> np.uint64(32) == np.uint64(components_before[c])).all()
    kept = sum(int((p.ref.chunks[c][1] == w).sum()) for c, w in before.items())
    changed = sum(int((p.ref.chunks[c][1] != w).sum()) for c, w in before.items())
    assert kept > 20 and changed > 20, "touched cell-filled chunks hold cells the frame updated and cells it left alone"
    p.check()
    p.fuse_rays(sensor, pts, 9.0, OTHER_MODEL)
    p.check("again, another model")


def test_three_frames_from_different_sensors_leave_no_marks_behind(pair):
    p = pair(chunk_dims=(4, 4, 4))
    rng = np.random.default_rng(45)
    touched = []
    for k, (at, n_rays, reach) in enumerate([((0.5, 0.5, 0.5), 300, 18.0), ((6.5, -3.5, 2.5), 300, 18.0), ((0.5, 0.5, 0.5), 40, 5.0)]):
        d = rng.normal(size=(n_rays, 3))
        pts = (np.array(at) + d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.0, reach, (n_rays, 1))).astype(np.float32)
        _, carved, hits = RR.frame(p.ref, at, pts, 30.0)
        H, M = F.sets_of(carved, hits)
        touched.append({p.ref.split(c)[0] for c in H | M})
        p.fuse_rays(at, pts, 30.0, what="frame %d" % k)
        p.check("frame %d" % k)                                               # a stale mark would show as a second update
    assert touched[2] < touched[0] and touched[2] < (touched[0] | touched[1]), "the last frame touches a strict subset of the chunks"


def test_a_seen_obstacle_that_leaves_fades_at_the_frame_the_restatement_says(pair, gpu):
    p = pair(chunk_dims=(4, 4, 4))
    sensor = np.array((0.5, 8.5, 8.5))
    wall = np.array([(20.5, y + 0.5, z + 0.5) for y in range(3, 15) for z in range(3, 15)])

    def seen(box):
        """the frame's points: where each ray to the wall meets the plane x = 10.5 inside the box's face, else the wall"""
        at = sensor + (wall - sensor) * ((10.5 - sensor[0]) / (wall[0, 0] - sensor[0]))
        on_box = box & (at[:, 1] >= 6) & (at[:, 1] < 11) & (at[:, 2] >= 6) & (at[:, 2] < 11)
        return np.where(on_box[:, None], at, wall).astype(np.float32), on_box
    first, on_box = seen(True)
    old_place = np.unique(np.floor(first[on_box].astype(np.float64)), axis=0).astype(np.int64)
    # by hand: three hits leave odds (7/3)^3 = 12.7; each miss multiplies them by 2/3; they pass below 1 with the seventh miss
    occ, want_fade = np.float32(0.5), None
    for k in range(10):
        occ = F.fuse(occ, MODEL[0] if k < 3 else MODEL[1], MODEL[2], MODEL[3])
        if k >= 3 and want_fade is None and not occ > np.float32(0.5):
            want_fade = k
    assert want_fade == 9
    lower, shape = (0, 2, 2), (24, 14, 14)
    at = tuple((old_place - np.array(lower)).T)
    n_vox = int(np.prod(shape))
    faded = None
    for k in range(11):
        p.fuse_rays(sensor, seen(k < 3)[0], 40.0, what="frame %d" % k)
        want = p.ref.window(lower, shape)
        want_bits = R.pack_bits(R.classify(want, False))
        d_bits = torch.full(((n_vox + 31) // 32,), -1, dtype=torch.int32, device="cuda")
        d_sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        p.gpu.extract_window_device(lower, shape, False, 0, d_bits.data_ptr(), stream)
        gpu.build_bits_device(d_bits.data_ptr(), shape, d_sdf.data_ptr(), 1.0, False, stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_bits.cpu().numpy().view(np.uint32), want_bits), "window bits after frame %d" % k
        want_sdf, _ = gpu.build_cells(want.view(np.float32), shape, 8, 0, False, 1.0, False)
        assert np.array_equal(d_sdf.cpu().numpy().view(np.uint32), want_sdf.view(np.uint32)), "the SDF of the window differs from the SDF of the restatement's records"
        filled = R.classify(want, False)[at]
        if faded is None and k >= 3 and not filled.any():
            faded = k
        if faded is None:
            assert filled.all() and (want_sdf[at] < 0).all(), "frame %d: the obstacle's place is still an obstacle" % k
        else:
            assert not filled.any() and (want_sdf[at] > 0).all(), "frame %d: the obstacle's old place is outside every obstacle" % k
    assert faded == want_fade
    p.check()


# ---- growth and the byte limit -------------------------------------------------------------------------------------------------------------
def test_growth_from_the_smallest_table_and_a_one_chunk_pool_in_one_frame(pair):
    p = pair(chunk_dims=(3, 2, 5), initial_chunks=1)
    info = p.gpu.info()
    assert info["table_capacity"] == 16 and info["capacity_chunks"] == 1
    rng = np.random.default_rng(46)
    sensor, pts = random_frame(rng, np.eye(4), 1.0, 1000, 40.0)
    st, counts = p.fuse_rays(sensor, pts, 30.0)
    info = p.check("one frame")
    assert counts["new_chunks"] == info["cell_filled"] > 800 and info["table_capacity"] >= 2 * info["cell_filled"]
    assert info["scratch_bytes"] >= info["capacity_chunks"] * 30, "the mark plane counts in scratch_bytes: a byte per cell of the pool"
    p.fuse_rays(sensor + 50.0, pts + np.float32(50.0), 30.0)
    p.check("a second frame beside it")
    p.set_cells(rng.uniform(200, 260, (300, 3)), R.record(0.9, 1))            # a batch grows the pool; the next fused frame catches up with it
    p.fuse_rays(sensor + 230.0, pts[:300] + np.float32(230.0), 30.0)
    p.check("a third frame after a batch grew the pool")


def test_a_frame_that_does_not_fit_the_byte_limit_is_refused_and_changes_nothing(pair):
    dims, cpc = (4, 4, 4), 64
    limit = 32 * 12 + 2 * (24 + 8 * cpc)                                    # a table of 32 entries and a pool of 2 chunks
    p = pair(chunk_dims=dims, initial_chunks=2, byte_limit=limit)
    sensor = (0.5, 0.5, 0.5)
    fits = np.array([(7.5, 0.5, 0.5)], np.float32)                           # passes cells 0 .. 6, hits 7: chunks 0 and 1
    too_far = np.array([(8.5, 0.5, 0.5)], np.float32)                        # passes cells 0 .. 7 (chunks 0 and 1), hits 8: chunk 2
    held_by = lambda info: {k: v for k, v in info.items() if k != "scratch_bytes"}       # (scratch is not what the limit bounds)
    start = p.gpu.info()
    assert start["table_capacity"] == 16 and start["capacity_chunks"] == 2

    def device_form(points):
        d = torch.from_numpy(points).cuda()
        p.gpu.fuse_rays_device(sensor, d.data_ptr(), len(points), 9.0)
        torch.cuda.synchronize()
    # One such ray may enter 3 chunks: the table of 16 entries takes its keys, the pool refuses, the keys are rolled back.  Four of them
    # (duplicates) may enter 12: the frame's table of 32 entries is made before the pool refuses, and must be given back.
    def refused_both_ways(what, before):
        for points in (too_far, np.repeat(too_far, 4, axis=0)):
            for call in (lambda: p.gpu.fuse_rays(sensor, points, 9.0), lambda: device_form(points)):
                with pytest.raises(capi.SdfGpuError) as e:
                    call()
                assert e.value.code == -3 and "byte limit" in str(e.value)
                assert held_by(p.check("%s, %d rays" % (what, len(points)))) == held_by(before)
    refused_both_ways("refused on the empty map", start)
    p.fuse_rays(sensor, fits, 9.0)                                           # a good frame after the refusals: the marks are still zero
    held = p.check("two chunks")
    assert held["cell_filled"] == 2 and held["table_capacity"] == 16 and held["bytes_held"] <= limit
    refused_both_ways("refused beside two chunks", held)
    rec, st = p.gpu.get([(x + 0.5, 0.5, 0.5) for x in range(10)])
    assert rec.tolist() == [fused(0.5, "miss")] * 7 + [fused(0.5, "hit")] + [DEFAULT] * 2 and st.tolist() == [2] * 8 + [0] * 2
    # a frame whose table alone would pass the limit is refused before anything is enqueued
    with pytest.raises(capi.SdfGpuError) as e:
        p.gpu.fuse_rays(sensor, np.array([(x + 0.5, y + 0.5, 0.5) for x in range(8) for y in range(8)], np.float32), 9.0)
    assert e.value.code == -3 and "byte limit" in str(e.value)
    assert p.check("refused by the table")["bytes_held"] == held["bytes_held"]
    p.fuse_rays(sensor, fits, 9.0)                                           # every later frame is as if the refused ones had not happened
    p.fuse_rays(sensor, fits[:, [1, 0, 2]] * np.float32(0.5), 9.0)          # (0.25, 3.75, 0.25), chunk 0
    rec, _ = p.gpu.get([(0.5, 0.5, 0.5), (7.5, 0.5, 0.5)])
    assert rec.tolist() == [fused(0.5, "miss", "miss", "miss"), fused(0.5, "hit", "hit")]
    p.check("after the refusals")


def test_more_than_65535_touched_chunks_in_one_frame(pair):
    p = pair(chunk_dims=(1, 1, 1))
    rng = np.random.default_rng(47)
    d = rng.normal(size=(300, 3))
    pts = (0.5 + d / np.linalg.norm(d, axis=1)[:, None] * 400.0).astype(np.float32)
    st, counts = p.fuse_rays((0.5, 0.5, 0.5), pts, 256.0)
    assert (st == capi.DSH_RAY_TRUNCATED).all() and counts["new_chunks"] > 65535
    p.check()


# ---- the edges -------------------------------------------------------------------------------------------------------------------------------
def test_the_model_refusals_no_ray_and_one_ray(pair):
    p = pair(chunk_dims=(3, 2, 5))
    pts = np.array([(5.5, 0.5, 0.5)], np.float32)
    p.fuse_rays((0.5, 0.5, 0.5), pts, 10.0)
    for bad in [(0.7, 0.4, 0.97, 0.12), (0.0009999, 0.4, 0.12, 0.97), (0.7, 0.9990001, 0.12, 0.97), (0.7, 0.4, 0.0, 0.97), (0.7, 0.4, 0.12, 1.0),
                (np.nan, 0.4, 0.12, 0.97), (0.7, np.nan, 0.12, 0.97), (0.7, 0.4, np.nan, 0.97), (0.7, 0.4, 0.12, np.nan), (-0.7, 0.4, 0.12, 0.97), (0.7, 0.4, 0.12, np.inf)]:
        with pytest.raises(F.Refused):
            F.fuse_rays(p.ref, (0.5, 0.5, 0.5), pts, 10.0, bad)
        assert "sensor model" in p.refused((0.5, 0.5, 0.5), pts, 10.0, bad)
        p.refused((0.5, 0.5, 0.5), pts[:0], 10.0, bad)                        # refused with no ray too
    for sensor, max_range in [((np.nan, 0.5, 0.5), 10.0), ((float(3 << 20), 0.5, 0.5), 10.0), ((0.5, 0.5, 0.5), 0.0), ((0.5, 0.5, 0.5), 65536.5), ((0.5, 0.5, 0.5), np.nan)]:
        with pytest.raises(F.Refused):
            F.fuse_rays(p.ref, sensor, pts, max_range)
        p.refused(sensor, pts, max_range)
    for corner in [(0.001, 0.001, 0.001, 0.001), (0.999, 0.999, 0.999, 0.999), (0.001, 0.999, 0.001, 0.999), (0.999, 0.001, 0.001, 0.999), (0.4, 0.7, 0.5, 0.5)]:
        p.fuse_rays((0.5, 0.5, 0.5), pts, 10.0, corner, what="%r" % (corner,))
        p.check("%r" % (corner,))


def test_no_ray_and_one_ray(pair):
    p = pair(chunk_dims=(3, 2, 5))
    st, counts = p.fuse_rays((0.5, 0.5, 0.5), np.zeros((0, 3), np.float32), 5.0)
    assert len(st) == 0 and counts == dict.fromkeys(counts, 0)
    info = p.check("no ray")
    assert info["chunk_filled"] == info["cell_filled"] == 0
    assert p.gpu.fuse_rays_device((0.5, 0.5, 0.5), 0, 0, 5.0) == counts
    st, counts = p.fuse_rays((0.5, 0.5, 0.5), [(-6.5, 0.5, 0.5)], 50.0)
    assert st.tolist() == [1] and counts == {"rays_hit": 1, "rays_truncated": 0, "rays_skipped": 0, "cells_carved": 7, "new_chunks": 4}
    p.check("one ray")
    # the device form with statuses and counts, one ray
    d = torch.tensor([[0.5, 0.5, 9.5]], dtype=torch.float32, device="cuda")
    d_st = torch.full((1,), 77, dtype=torch.uint8, device="cuda")
    got = p.gpu.fuse_rays_device((0.5, 0.5, 0.5), d.data_ptr(), 1, 4.0, OTHER_MODEL, d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want_st, want = F.fuse_rays(p.ref, (0.5, 0.5, 0.5), d.cpu().numpy(), 4.0, OTHER_MODEL)
    assert got == want and d_st.cpu().numpy().tolist() == want_st.tolist() == [2]
    p.check("one long ray on the device")


def test_the_carve_is_unchanged_beside_fused_frames(pair):
    """sdfgpu_dsh_insert_rays on a map that also takes fused frames: the records it writes overwrite, the fused frames update them"""
    p = pair(chunk_dims=(4, 4, 4))
    rng = np.random.default_rng(48)
    sensor, pts = random_frame(rng, np.eye(4), 1.0, 300, 15.0)
    p.fuse_rays(sensor, pts, 12.0)
    st, counts = p.gpu.insert_rays(sensor, pts[:150], 12.0, R.record(0.0, 1), R.record(1.0, 2))
    want_st, want_counts = RR.insert_rays(p.ref, sensor, pts[:150], 12.0, R.record(0.0, 1), R.record(1.0, 2))
    assert np.array_equal(st, want_st) and counts == want_counts
    p.check("carved")
    p.fuse_rays(sensor, pts, 12.0)
    p.check("fused again")


# ---- red zones -------------------------------------------------------------------------------------------------------------------------------
def core_cases_on(ctx):
    made = []

    def make(**kw):
        made.append(FusePair(ctx, **kw))
        return made[-1]
    try:
        test_random_frames_in_every_chunk_shape(make, (3, 3, 5), "rotated-quarter")
        test_random_frames_in_every_chunk_shape(make, (8, 8, 32), "identity")
        test_a_fan_of_rays_updates_the_cells_they_share_once(make)
        test_a_hit_beats_the_misses_and_two_hits_on_one_cell_count_once(make)
        test_truncated_and_skipped_rays_inside_a_frame(make)
        test_rays_through_absent_chunk_filled_and_cell_filled_chunks_in_one_frame(make)
        test_three_frames_from_different_sensors_leave_no_marks_behind(make)
        test_growth_from_the_smallest_table_and_a_one_chunk_pool_in_one_frame(make)
        test_a_frame_that_does_not_fit_the_byte_limit_is_refused_and_changes_nothing(make)
        test_no_ray_and_one_ray(make)
    finally:
        for p in made:
            p.close()


def test_the_core_cases_in_a_child_process_with_red_zones_from_the_environment():
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from sdf_tools_amd import capi\nimport test_gpu_dsh_fusion as T\n"
            "ctx = capi.SdfGpu(0)\nT.core_cases_on(ctx)\nctx.redzone_check()\nctx.close()\nprint('core cases clean')\n") % (tests, os.path.dirname(tests))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SDFGPU_REDZONE="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "core cases clean" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
