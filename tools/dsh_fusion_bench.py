#!/usr/bin/env python3
"""Timings of a frame of sensor rays fused into the dynamic spatial hashed map (sdfgpu_dsh_fuse_rays_device): one
JSON line, also appended to profiles/dsh_fusion_bench.jsonl with --out.  Device time between two events of the caller, medians of
`--reps` after `--warmup`.

The scene is that of tools/dsh_rays_bench.py: the room seen from the centre of a 512^3 region of 16^3 chunks, 200 k rays, a range of
256 cells.  In one run:
  warm_fuse_ms     the fused frame into a map that already holds every chunk it touches (the steady state of a map server)
  first_fuse_ms    the same frame into an empty map (table, pool and mark plane grow), a fresh map per repetition
  warm_carve_ms    sdfgpu_dsh_insert_rays_device of the same rays into a map of its own that already holds them
  copy_touched_ms  a device-to-device copy of the touched chunks' record bytes: the floor of the pass the fusion adds
The aim is reported as met or missed, never asserted: a warm fused frame within 1.25 x the warm carve frame of the same run.
usage: dsh_fusion_bench.py [--reps R] [--warmup W] [--out FILE] [--side N] [--rays N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdf_tools_amd import capi, synth  # noqa: E402
from dsh_rays_bench import CELL, FILLED, FREE, UNKNOWN, room_frame, timed  # noqa: E402


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
    sensor, pts, _ = room_frame(mask, side, n, range_cells)
    max_range = range_cells * CELL

    def fuse_into(m):
        return m.fuse_rays_device(sensor, pts.data_ptr(), n, max_range, None, stream=stream)

    def carve_into(m):
        return m.insert_rays_device(sensor, pts.data_ptr(), n, max_range, FREE, FILLED, stream=stream)

    # ---- the first fused frame into an empty map, a fresh map each time
    first_ms = []
    for _ in range(max(3, a.reps // 4)):
        m = ctx.dsh_create(None, CELL, (16, 16, 16), UNKNOWN)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        first_counts = fuse_into(m)
        e1.record()
        e1.synchronize()
        first_ms.append(e0.elapsed_time(e1))
        m.close()
    # ---- the warm frames, each kind into a map of its own
    fused, carved = ctx.dsh_create(None, CELL, (16, 16, 16), UNKNOWN), ctx.dsh_create(None, CELL, (16, 16, 16), UNKNOWN)
    fuse_into(fused)
    counts = fuse_into(fused)
    carve_into(carved)
    assert counts["new_chunks"] == 0 and carve_into(carved) == counts
    info = fused.info()
    chunks = info["cell_filled"]
    row = {"row": "fuse_rays", "fuse_kernel": "marks staged in LDS, records swept in lane order", "rays": n, "side": side, "range_cells": range_cells, "rays_hit": counts["rays_hit"], "rays_truncated": counts["rays_truncated"],
           "cells_carved": counts["cells_carved"], "chunks": chunks, "touched_record_bytes": chunks * 4096 * 8, "mark_plane_bytes": info["capacity_chunks"] * 4096,
           "first_frame_new_chunks": first_counts["new_chunks"], "first_fuse_ms": float(np.median(first_ms))}
    # the two warm frames alternate, so that whatever else the machine does falls on both alike
    for _ in range(a.warmup):
        fuse_into(fused)
        carve_into(carved)
    torch.cuda.synchronize()
    ms = {"fuse": [], "carve": []}
    for _ in range(a.reps):
        for name, call in (("fuse", lambda: fuse_into(fused)), ("carve", lambda: carve_into(carved))):
            ms[name].append(timed(call, 1, 0))
    row["warm_fuse_ms"], row["warm_carve_ms"] = float(np.median(ms["fuse"])), float(np.median(ms["carve"]))
    row["warm_fuse_ms_min_max"], row["warm_carve_ms_min_max"] = [min(ms["fuse"]), max(ms["fuse"])], [min(ms["carve"]), max(ms["carve"])]
    src, dst = torch.empty(chunks * 4096, dtype=torch.int64, device="cuda"), torch.empty(chunks * 4096, dtype=torch.int64, device="cuda")
    row["copy_touched_ms"] = timed(lambda: dst.copy_(src), a.reps, a.warmup)
    row["fuse_over_carve"] = row["warm_fuse_ms"] / row["warm_carve_ms"]
    row["aim_warm_fuse_within_1.25x_warm_carve"] = "met" if row["fuse_over_carve"] <= 1.25 else "missed"
    fused.close()
    carved.close()
    ctx.close()
    line = json.dumps(row)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
