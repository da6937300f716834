#!/usr/bin/env python3
"""Timings of the frontier calls on the dynamic spatial hashed map (sdfgpu_dsh_frontier_window_device, sdfgpu_dsh_frontier_cells_device,
sdfgpu_component_stats_device): one JSON line, also appended to profiles/dsh_frontier_bench.jsonl with --out.
Device time between two events of the caller, medians of `--reps` after `--warmup`, all in one run, the rows alternating twice (the
two passes' medians are reported side by side as the spread).

The scene is that of tools/dsh_rays_bench.py: the room scene in a 512^3 region of 16^3 chunks seen from the region's centre, 200 k
rays in evenly spread directions, range half the region, fused into the map until the frame is warm.
  warm_fused_frame_ms        sdfgpu_dsh_fuse_rays_device of the frame into the map that already holds it
  window_6_ms, window_26_ms  the frontier bits of the whole 512^3 region under either rule
  extract_window_bits_ms     sdfgpu_dsh_extract_window_device of the same window, bits only
  copy_bits_ms               a device-to-device copy of the window's 16 MiB of bits
  cells_6_ms, cells_26_ms    the list over the whole map (a call that sizes the list included in neither: the capacity suffices)
  export_ms                  sdfgpu_dsh_export_device of the whole map
  clusters_window_ms, clusters_components_ms, clusters_stats_ms   the three calls of ExtractFrontierClusters on the 512^3 window,
                             26-rule; clusters_ms is their sum
The aims -- window_6_ms at most twice extract_window_bits_ms, clusters_ms below warm_fused_frame_ms -- are reported as met or
missed, never asserted.
usage: dsh_frontier_bench.py [--reps R] [--warmup W] [--out FILE] [--side N] [--rays N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from dsh_rays_bench import CELL, UNKNOWN, room_frame, timed  # noqa: E402
from sdf_tools_amd import capi, synth  # noqa: E402


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
    m = ctx.dsh_create(None, CELL, (16, 16, 16), UNKNOWN)
    for _ in range(2):
        m.fuse_rays_device(sensor, pts.data_ptr(), n, max_range, stream=stream)
    info = m.info()
    n_chunks, cpc = info["chunk_filled"] + info["cell_filled"], m.cells_per_chunk
    lower, n_vox = (0, 0, 0), side ** 3
    d_bits = torch.zeros((n_vox + 31) // 32, dtype=torch.int32, device="cuda")
    d_bits_copy = torch.zeros_like(d_bits)
    d_labels = torch.zeros(n_vox, dtype=torch.int32, device="cuda")
    totals = [m.frontier_cells_device(None, None, flags, 0, 0, stream) for flags in (0, capi.DSH_FRONTIER_26)]
    d_cells = torch.zeros((max(totals), 3), dtype=torch.int64, device="cuda")
    d_chunks = torch.zeros((n_chunks, 6), dtype=torch.int64, device="cuda")
    d_export = torch.zeros((info["cell_filled"], cpc), dtype=torch.int64, device="cuda")
    m.frontier_window_device(lower, shape, capi.DSH_FRONTIER_26, d_bits.data_ptr(), stream)
    labels = ctx.components_bits_device(d_bits.data_ptr(), shape, d_labels.data_ptr(), stream)
    clusters = ctx.component_stats_device(d_bits.data_ptr(), d_labels.data_ptr(), shape, labels, 0, 0, stream)
    d_stats = torch.zeros((max(clusters, 1), 8), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    window_set = [0, 0]
    for k, flags in enumerate((0, capi.DSH_FRONTIER_26)):
        m.frontier_window_device(lower, shape, flags, d_bits_copy.data_ptr(), stream)
        torch.cuda.synchronize()
        words = d_bits_copy[d_bits_copy != 0].cpu().numpy().view("uint32")
        window_set[k] = int(sum(bin(int(w)).count("1") for w in words))
    row = {"row": "frontier", "rays": n, "side": side, "range_cells": range_cells, "chunks": n_chunks, "cell_filled_chunks": info["cell_filled"],
           "frontier_cells_6": totals[0], "frontier_cells_26": totals[1], "window_set_bits_6": window_set[0], "window_set_bits_26": window_set[1],
           "labels": labels, "clusters_26": clusters}

    def window(flags):
        return lambda: m.frontier_window_device(lower, shape, flags, d_bits.data_ptr(), stream)

    def cells(flags):
        return lambda: m.frontier_cells_device(None, None, flags, d_cells.data_ptr(), len(d_cells), stream)
    calls = {
        "warm_fused_frame_ms": lambda: m.fuse_rays_device(sensor, pts.data_ptr(), n, max_range, stream=stream),
        "window_6_ms": window(0), "window_26_ms": window(capi.DSH_FRONTIER_26),
        "extract_window_bits_ms": lambda: m.extract_window_device(lower, shape, False, 0, d_bits_copy.data_ptr(), stream),
        "copy_bits_ms": lambda: d_bits_copy.copy_(d_bits),
        "cells_6_ms": cells(0), "cells_26_ms": cells(capi.DSH_FRONTIER_26),
        "export_ms": lambda: m.export_device(d_chunks.data_ptr(), n_chunks, d_export.data_ptr(), d_export.numel(), stream),
        "clusters_window_ms": window(capi.DSH_FRONTIER_26),
        "clusters_components_ms": lambda: ctx.components_bits_device(d_bits.data_ptr(), shape, d_labels.data_ptr(), stream),
        "clusters_stats_ms": lambda: ctx.component_stats_device(d_bits.data_ptr(), d_labels.data_ptr(), shape, labels, d_stats.data_ptr(), len(d_stats), stream)}
    # (the fused frame changes occupancies, not which cells are free or unknown once they are clamped: it runs last in each pass)
    order = [k for k in calls if k != "warm_fused_frame_ms"] + ["warm_fused_frame_ms"]
    passes = [{k: timed(calls[k], a.reps, a.warmup) for k in order} for _ in range(2)]
    for k in order:
        row[k] = min(p[k] for p in passes)
        row[k.replace("_ms", "_other_pass_ms")] = max(p[k] for p in passes)
    row["clusters_ms"] = row["clusters_window_ms"] + row["clusters_components_ms"] + row["clusters_stats_ms"]
    row["aim_window_6_within_twice_extract_window"] = "met" if row["window_6_ms"] <= 2.0 * row["extract_window_bits_ms"] else "missed"
    row["aim_clusters_below_warm_fused_frame"] = "met" if row["clusters_ms"] < row["warm_fused_frame_ms"] else "missed"
    m.close()
    ctx.close()
    line = json.dumps(row)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
