#!/usr/bin/env python3
"""Timings of sdfgpu_dsh_update_components on the dynamic spatial hashed map: one JSON line per scene, also
appended to profiles/dsh_components_bench.jsonl with --out.  Device time between two events of the caller around one call (the
call's two synchronisations and its read-backs included), `--reps` calls after `--warmup`, all in one run; the rows are taken in
two alternating passes, and each row reports the median, the smallest and the largest call of the pass with the lower median and the
other pass's median beside it.

The scenes are those of tools/dsh_bench.py, in a 512^3 region of 16^3 chunks:
  room    every filled voxel of the room scene (synth.room_mask_torch) as a cell set; absent chunks elsewhere
  cloud   twenty frames of 200 k points on a wavy wall, inserted as points
Rows per scene:
  update_ms, update_apart_ms     sdfgpu_dsh_update_components of the whole map under either rule
  extract_window_bits_ms         sdfgpu_dsh_extract_window_device of the 512^3 window over the same map, bits only
  dense_components_ms            sdfgpu_components_bits_device on those bits
  dense_pair_ms                  the sum of the two: what a caller had to do before the update existed
The aim -- update_ms at most dense_pair_ms on the room map -- is reported as met or missed, never asserted.  The shares of the single
kernels are not taken here: they come from a kernel trace of this script with few repetitions (rocprofv3 --kernel-trace --stats).
usage: dsh_components_bench.py [--reps R] [--warmup W] [--out FILE] [--side N] [--points N] [--scene room|cloud|both]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from dsh_bench import CELL, FILLED, frame  # noqa: E402
from sdf_tools_amd import capi, synth  # noqa: E402


def calls_ms(call, reps, warmup):
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
    return ms


def scene_row(ctx, name, m, side, reps, warmup):
    shape, n_vox = (side,) * 3, side ** 3
    stream = torch.cuda.current_stream().cuda_stream
    info = m.info()
    d_bits = torch.zeros((n_vox + 31) // 32, dtype=torch.int32, device="cuda")
    d_labels = torch.zeros(n_vox, dtype=torch.int32, device="cuda")
    m.extract_window_device((0, 0, 0), shape, False, 0, d_bits.data_ptr(), stream)
    row = {"row": "components (%s)" % name, "side": side, "chunks": info["chunk_filled"] + info["cell_filled"], "cell_filled_chunks": info["cell_filled"],
           "nodes": info["cell_filled"] * m.cells_per_chunk + info["chunk_filled"], "window_voxels": n_vox, "reps": reps,
           "components": m.update_components(0, stream), "components_apart": m.update_components(capi.DSH_COMPONENTS_UNKNOWN_APART, stream),
           "dense_labels": ctx.components_bits_device(d_bits.data_ptr(), shape, d_labels.data_ptr(), stream)}
    row["scratch_bytes"] = m.info()["scratch_bytes"]
    calls = {
        "update_ms": lambda: m.update_components(0, stream),
        "update_apart_ms": lambda: m.update_components(capi.DSH_COMPONENTS_UNKNOWN_APART, stream),
        "extract_window_bits_ms": lambda: m.extract_window_device((0, 0, 0), shape, False, 0, d_bits.data_ptr(), stream),
        "dense_components_ms": lambda: ctx.components_bits_device(d_bits.data_ptr(), shape, d_labels.data_ptr(), stream)}
    passes = [{k: calls_ms(calls[k], reps, warmup) for k in calls} for _ in range(2)]
    for k in calls:
        best, other = sorted(passes, key=lambda p: float(np.median(p[k])))
        row[k] = float(np.median(best[k]))
        row[k.replace("_ms", "_min_ms")], row[k.replace("_ms", "_max_ms")] = float(min(best[k])), float(max(best[k]))
        row[k.replace("_ms", "_other_pass_ms")] = float(np.median(other[k]))
    row["dense_pair_ms"] = row["extract_window_bits_ms"] + row["dense_components_ms"]
    row["update_over_dense_pair"] = row["update_ms"] / row["dense_pair_ms"]
    row["aim_update_no_slower_than_dense_pair"] = "met" if row["update_ms"] <= row["dense_pair_ms"] else "missed"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--scene", default="both", choices=["room", "cloud", "both"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    side, shape = a.side, (a.side,) * 3
    ctx = capi.SdfGpu(0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    if a.scene in ("room", "both"):
        room = ctx.dsh_create(None, CELL, (16, 16, 16), 0)
        loc = ((torch.nonzero(synth.room_mask_torch(shape)).to(torch.float64) + 0.5) * CELL).contiguous()
        step = 1 << 22
        for k in range(0, len(loc), step):
            part = loc[k:k + step].contiguous()
            room.set_cells_device(part.data_ptr(), len(part), one_value=FILLED, stream=stream)
        rows.append(scene_row(ctx, "room", room, side, a.reps, a.warmup))
        room.close()
    if a.scene in ("cloud", "both"):
        cloud = ctx.dsh_create(None, CELL, (16, 16, 16), 0)
        for s in range(20):
            f = frame(side, a.points, s)
            cloud.insert_points_device(f.data_ptr(), len(f), FILLED, stream=stream)
        rows.append(scene_row(ctx, "cloud", cloud, side, a.reps, a.warmup))
        cloud.close()
    ctx.close()
    for r in rows:
        line = json.dumps(r)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
