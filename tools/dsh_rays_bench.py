#!/usr/bin/env python3
"""Timings of a frame of sensor rays carved into the dynamic spatial hashed map (sdfgpu_dsh_insert_rays_device):
one JSON line per row, also appended to profiles/dsh_rays_bench.jsonl with --out.  Device time between two events of the caller,
medians of `--reps` after `--warmup`.

The scene: the room scene (synth.room_mask_torch) in a 512^3 region of 16^3 chunks, the sensor at the region's centre, 200 k rays in
evenly spread directions.  A ray's return is the first filled voxel along it (marched here in torch); a ray that leaves the region has
no return inside the range and is given a point beyond it, so it carves up to max_range = half the region and hits nothing.
  warm    the frame into a map that already holds it (every chunk exists: the steady state of a map server), with the frame's
          cells_carved and mean walk length beside the time
  first   the same frame into an empty map (table and pool grow, every chunk is made), a fresh map per repetition
Beside them: sdfgpu_dsh_insert_points_device of the same points, a device fill of cells_carved * 8 bytes (the floor of the store
traffic), sdfgpu_dsh_extract_window_device (bits) of the 512^3 window and sdfgpu_build_bits_device on it.
The aim is reported as met or missed, never asserted: a warm frame costs less than the window extraction plus the build it feeds.
lane_step_share is computed from the rays' lengths, not measured: the share of the lane-steps of the walk kernels' waves (64 rays in
list order, each wave as long as its longest ray) in which a lane still has a cell to walk.
usage: dsh_rays_bench.py [--reps R] [--warmup W] [--out FILE] [--side N] [--rays N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdf_tools_amd import capi, synth  # noqa: E402

CELL = 0.01
UNKNOWN, FREE, FILLED = capi.dsh_record(0.5, 0), capi.dsh_record(0.0, 0), capi.dsh_record(1.0, 0)


def timed(call, reps, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def room_frame(mask, side, n_rays, range_cells):
    """(sensor xyz in metres, points float32 [n, 3] on the device, walk lengths in cells): the room seen from the region's centre"""
    k = torch.arange(n_rays, device="cuda", dtype=torch.float64) + 0.5
    z = 1.0 - 2.0 * k / n_rays                                               # a Fibonacci sphere: evenly spread directions
    r = torch.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    d = torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], 1)
    s = torch.full((3,), side / 2 + 0.5, device="cuda", dtype=torch.float64)   # in cells
    hit_t = torch.full((n_rays,), float("inf"), device="cuda", dtype=torch.float64)
    flat = mask.reshape(-1)
    for step in range(1, int(2 * side * 0.9)):                                # half-cell steps out to the region's corners
        t = 0.5 * step
        i = torch.floor(s + d * t).to(torch.int64)
        inside = ((i >= 0) & (i < side)).all(1)
        ic = i.clamp(0, side - 1)
        filled = inside & (flat[(ic[:, 0] * side + ic[:, 1]) * side + ic[:, 2]] != 0)
        hit_t = torch.where(filled & torch.isinf(hit_t), torch.full_like(hit_t, t), hit_t)
    reach = torch.where(torch.isinf(hit_t), torch.full_like(hit_t, range_cells * 1.25), hit_t)
    pts = ((s + d * reach[:, None]) * CELL).to(torch.float32).contiguous()
    walked = torch.minimum(reach, torch.full_like(reach, float(range_cells)))[:, None] * d.abs()
    return (s * CELL).cpu().numpy(), pts, walked.sum(1)                        # (the L1 length: about the number of cells of the walk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--rays", type=int, default=200000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    side, shape, n = a.side, (a.side,) * 3, a.rays
    range_cells = side // 2
    ctx = capi.SdfGpu(0)
    stream = torch.cuda.current_stream().cuda_stream
    mask = synth.room_mask_torch(shape)
    sensor, pts, lengths = room_frame(mask, side, n, range_cells)
    max_range = range_cells * CELL

    def frame_into(m):
        return m.insert_rays_device(sensor, pts.data_ptr(), n, max_range, FREE, FILLED, stream=stream)

    # ---- the first frame into an empty map, a fresh map each time
    first_ms = []
    for _ in range(max(3, a.reps // 4)):
        m = ctx.dsh_create(None, CELL, (16, 16, 16), UNKNOWN)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        first_counts = frame_into(m)
        e1.record()
        e1.synchronize()
        first_ms.append(e0.elapsed_time(e1))
        m.close()
    # ---- the warm frame
    m = ctx.dsh_create(None, CELL, (16, 16, 16), UNKNOWN)
    frame_into(m)
    counts = frame_into(m)
    assert counts["new_chunks"] == 0
    walked = counts["rays_hit"] + counts["rays_truncated"]
    waves = lengths.reshape(-1, 64) if n % 64 == 0 else lengths[:n // 64 * 64].reshape(-1, 64)
    row = {"row": "insert_rays", "rays": n, "side": side, "range_cells": range_cells, "rays_hit": counts["rays_hit"], "rays_truncated": counts["rays_truncated"],
           "cells_carved": counts["cells_carved"], "mean_walk_cells": counts["cells_carved"] / max(walked, 1), "chunks": m.info()["cell_filled"],
           "first_frame_new_chunks": first_counts["new_chunks"], "first_frame_ms": float(np.median(first_ms)),
           "lane_step_share": float(waves.sum() / (64.0 * waves.max(1).values.sum()))}
    row["warm_frame_ms"] = timed(lambda: frame_into(m), a.reps, a.warmup)
    row["insert_points_ms"] = timed(lambda: m.insert_points_device(pts.data_ptr(), n, FILLED, stream=stream), a.reps, a.warmup)
    floor = torch.empty(counts["cells_carved"], dtype=torch.int64, device="cuda")
    row["fill_carved_bytes_ms"] = timed(lambda: floor.fill_(FREE), a.reps, a.warmup)
    d_bits = torch.zeros(side ** 3 // 32, dtype=torch.int32, device="cuda")
    d_sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
    frame_into(m)                                                             # (the insert_points rows above filled every return again: same map)
    row["extract_window_ms"] = timed(lambda: m.extract_window_device((0, 0, 0), shape, False, 0, d_bits.data_ptr(), stream), a.reps, a.warmup)
    row["build_bits_ms"] = timed(lambda: ctx.build_bits_device(d_bits.data_ptr(), shape, d_sdf.data_ptr(), CELL, False, stream), a.reps, a.warmup)
    row["aim_warm_frame_below_extract_plus_build"] = "met" if row["warm_frame_ms"] < row["extract_window_ms"] + row["build_bits_ms"] else "missed"
    m.close()
    ctx.close()
    line = json.dumps(row)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
