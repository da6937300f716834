#!/usr/bin/env python3
"""Timings of removal from the dynamic spatial hashed map (sdfgpu_dsh_retain_box, sdfgpu_dsh_remove_chunks_device, sdfgpu_dsh_shrink;
DESIGN.md section 32): one JSON line, appended to profiles/dsh_remove_bench.jsonl (--out).  Device time between two events of the
caller, medians of `--reps` after `--warmup`.

The scene is that of tools/dsh_rays_bench.py: the room seen from the centre of a 512^3 region of 16^3 chunks, 200 k rays, a range of
256 cells, fused into a map until it is warm.  In one run:
  slide_retain_ms   sdfgpu_dsh_retain_box with the region slid by one chunk layer along x (the layer x < 16 cells goes)
  slide_list_ms     sdfgpu_dsh_remove_chunks_device of the same chunks, one location each
  shrink_ms         sdfgpu_dsh_shrink(0) after the half x < 256 cells was removed
beside their baselines
  copy_removed_ms   a device-to-device copy of removed x (24 + 8 x 4096) bytes: the most the slide's moves can carry (there are at
                    most as many movers as removed chunks)
  copy_half_ms      the same for the chunks shrink keeps: what its two copies carry
  one_chunk_ms      a removal of ONE chunk by list: flags, count, read-back, scan, one move, the table's clear and k_dsh_rehash over
                    every kept head -- what a removal costs apart from its moves
  table_clear_ms    a device memset of the table's key bytes alone
  warm_fuse_ms      the warm fused frame of this run
Between repetitions the frame is fused again (untimed), which brings the removed chunks back.  The aim is reported as met or MISSED,
never asserted: sliding by one layer costs less than the warm fused frame it precedes.
usage: dsh_remove_bench.py [--reps R] [--warmup W] [--out FILE] [--side N] [--rays N]"""
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
from dsh_rays_bench import CELL, UNKNOWN, room_frame, timed  # noqa: E402

CHUNK = 16
CHUNK_BYTES = 24 + 8 * CHUNK ** 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--rays", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsh_remove_bench.jsonl"))
    a = ap.parse_args()
    side, shape, n = a.side, (a.side,) * 3, a.rays
    range_cells = side // 2
    ctx = capi.SdfGpu(0)
    stream = torch.cuda.current_stream().cuda_stream
    mask = synth.room_mask_torch(shape)
    sensor, pts, _ = room_frame(mask, side, n, range_cells)
    max_range = range_cells * CELL
    m = ctx.dsh_create(None, CELL, (CHUNK,) * 3, UNKNOWN)

    def fuse():
        return m.fuse_rays_device(sensor, pts.data_ptr(), n, max_range, None, stream=stream)

    def live():
        info = m.info()
        return info["chunk_filled"] + info["cell_filled"]
    fuse()
    assert fuse()["new_chunks"] == 0
    chunks = live()
    # the chunks of the layer x < 16 cells, by Get at one location each
    per_side = side // CHUNK + 2
    yz = (np.stack(np.meshgrid(np.arange(-1, per_side - 1), np.arange(-1, per_side - 1), indexing="ij"), -1).reshape(-1, 2) * CHUNK + 0.5) * CELL
    layer = np.concatenate([np.full((len(yz), 1), 0.5 * CELL), yz], 1)
    layer = layer[m.get(layer)[1] != 0]
    d_layer = torch.from_numpy(np.ascontiguousarray(layer)).cuda()
    far = side + 2 * CHUNK
    slid = ((CHUNK, -CHUNK, -CHUNK), (far, far + CHUNK, far + CHUNK))
    half = ((side // 2, -CHUNK, -CHUNK), (far, far + CHUNK, far + CHUNK))
    removed = {}

    def once(call, restore=fuse):
        """device time of one call between two events, the map restored (untimed) in front of it"""
        restore()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def slide_retain():
        removed["retain"] = m.retain_box(slid[0], slid[1], stream=stream)

    def slide_list():
        removed["list"] = m.remove_chunks_device(d_layer.data_ptr(), len(layer), stream=stream)

    def one_chunk():
        removed["one"] = m.remove_chunks_device(d_layer.data_ptr(), 1, stream=stream)

    def remove_half():
        fuse()
        removed["half"] = m.retain_box(half[0], half[1], stream=stream)
    ms = {k: [] for k in ("slide_retain_ms", "slide_list_ms", "one_chunk_ms", "warm_fuse_ms", "shrink_ms")}
    for rep in range(a.warmup + a.reps):
        got = {"slide_retain_ms": once(slide_retain), "slide_list_ms": once(slide_list), "one_chunk_ms": once(one_chunk),
               "warm_fuse_ms": once(lambda: fuse())}
        if rep % 3 == 0 or rep < a.warmup:                                      # (a shrink is followed by a frame that grows everything again)
            got["shrink_ms"] = once(lambda: m.shrink(0, stream=stream), restore=remove_half)
            fuse()
        if rep >= a.warmup:
            for k, v in got.items():
                ms[k].append(v)
    fuse()
    assert live() == chunks and removed["retain"] == removed["list"] == len(layer) and removed["one"] == 1
    info = m.info()
    row = {"row": "dsh_remove", "rays": n, "side": side, "range_cells": range_cells, "chunks": chunks, "table_capacity": info["table_capacity"],
           "slide_removed_chunks": removed["retain"], "half_removed_chunks": removed["half"], "reps": a.reps}
    for k, v in ms.items():
        row[k] = float(np.median(v))
        row[k + "_min_max"] = [min(v), max(v)]

    def copy_ms(n_chunks):
        words = max(1, n_chunks * CHUNK_BYTES // 8)
        src, dst = torch.empty(words, dtype=torch.int64, device="cuda"), torch.empty(words, dtype=torch.int64, device="cuda")
        return timed(lambda: dst.copy_(src), a.reps, a.warmup)
    row["copy_removed_ms"] = copy_ms(removed["retain"])
    row["copy_half_ms"] = copy_ms(chunks - removed["half"])
    keys = torch.empty(info["table_capacity"], dtype=torch.int64, device="cuda")
    row["table_clear_ms"] = timed(lambda: keys.fill_(-1), a.reps, a.warmup)
    row["slide_over_warm_fuse"] = row["slide_retain_ms"] / row["warm_fuse_ms"]
    row["slide_over_copy_removed"] = row["slide_retain_ms"] / row["copy_removed_ms"]
    row["aim_slide_below_warm_fuse"] = "met" if row["slide_retain_ms"] < row["warm_fuse_ms"] else "MISSED"
    m.close()
    ctx.close()
    line = json.dumps(row)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
