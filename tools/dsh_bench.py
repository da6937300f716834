#!/usr/bin/env python3
"""Timings of the dynamic spatial hashed map (sdfgpu_dsh_*): one JSON line per row, also appended to
profiles/dsh_bench.jsonl with --out.  A 512^3 window with 16^3 chunks; every row is measured beside a baseline of the parent commit on
the same data, in the same process.  Medians of `--reps` after `--warmup`, between two events of the caller:
  insert          sdfgpu_dsh_insert_points_device of a 200 k-point frame into a warm map (the frame's chunks exist: the steady state
                  of a map server), beside sdfgpu_voxelize_points_bits_device of the same points into the dense 512^3 bit field
  window (room)   sdfgpu_dsh_extract_window_device, bits only, from a map that holds the room scene (synth.room_mask_torch) as cells,
  window (cloud)  and from a map that holds twenty point-cloud frames; beside each a device-to-device copy of the bytes the call must
                  read and write (the live chunks' cells in the window + the bit field) and sdfgpu_build_bits_device on those bits
Two aims are reported as met or missed, never asserted: the extraction costs less than the build it feeds, and the insert costs less
than twice the dense voxelise.
usage: dsh_bench.py [--reps R] [--warmup W] [--out FILE] [--side N]"""
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
FILLED = capi.dsh_record(1.0, 0)


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


def frame(side, n_points, seed):
    """points on a wavy wall through the window, float32 [n, 3] on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    uv = torch.rand((n_points, 2), device="cuda", generator=g) * (side * CELL)
    depth = (0.5 + 0.2 * torch.sin(uv[:, 0] * 3.0 + seed) * torch.cos(uv[:, 1] * 2.0)) * (side * CELL)
    return torch.stack([uv[:, 0], depth, uv[:, 1]], 1).contiguous()


def window_rows(ctx, name, m, side, reps, warmup):
    shape, n = (side,) * 3, side ** 3
    stream = torch.cuda.current_stream().cuda_stream
    d_bits = torch.zeros(n // 32, dtype=torch.int32, device="cuda")
    d_sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
    info = m.info()
    read = info["cell_filled"] * m.cells_per_chunk * 8 + info["chunk_filled"] * 24
    src = torch.empty(read + n // 8, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    row = {"row": "window (%s)" % name, "side": side, "chunks": info["cell_filled"] + info["chunk_filled"], "bytes_read_and_written": read + n // 8}
    row["extract_ms"] = timed(lambda: m.extract_window_device((0, 0, 0), shape, False, 0, d_bits.data_ptr(), stream), reps, warmup)
    row["dtod_ms"] = timed(lambda: dst.copy_(src), reps, warmup)
    row["build_bits_ms"] = timed(lambda: ctx.build_bits_device(d_bits.data_ptr(), shape, d_sdf.data_ptr(), CELL, False, stream), reps, warmup)
    row["aim_extract_below_build"] = "met" if row["extract_ms"] < row["build_bits_ms"] else "missed"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    side, shape = a.side, (a.side,) * 3
    ctx = capi.SdfGpu(0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    # ---- the point-cloud map: twenty frames, then the insert of one of them again (warm) beside the dense voxelise
    cloud = ctx.dsh_create(None, CELL, (16, 16, 16), 0)
    frames = [frame(side, a.points, s) for s in range(20)]
    for f in frames:
        cloud.insert_points_device(f.data_ptr(), len(f), FILLED, stream=stream)
    d_bits = torch.zeros(side ** 3 // 32, dtype=torch.int32, device="cuda")
    origin = np.zeros(3)
    row = {"row": "insert", "points": a.points, "side": side, "chunks": cloud.info()["cell_filled"]}
    row["insert_ms"] = timed(lambda: cloud.insert_points_device(frames[7].data_ptr(), a.points, FILLED, stream=stream), a.reps, a.warmup)
    row["voxelize_bits_ms"] = timed(lambda: ctx.voxelize_points_bits_device(frames[7].data_ptr(), a.points, origin, CELL, shape, d_bits.data_ptr(), True, stream),
                                    a.reps, a.warmup)
    row["aim_insert_below_twice_voxelize"] = "met" if row["insert_ms"] < 2.0 * row["voxelize_bits_ms"] else "missed"
    rows.append(row)
    rows.append(window_rows(ctx, "cloud", cloud, side, a.reps, a.warmup))
    cloud.close()

    # ---- the room map: every filled voxel of the room scene as a cell set
    room = ctx.dsh_create(None, CELL, (16, 16, 16), 0)
    mask = synth.room_mask_torch(shape)
    idx = torch.nonzero(mask).to(torch.float64)
    loc = ((idx + 0.5) * CELL).contiguous()
    step = 1 << 22
    for k in range(0, len(loc), step):
        part = loc[k:k + step].contiguous()
        room.set_cells_device(part.data_ptr(), len(part), one_value=FILLED, stream=stream)
    rows.append(window_rows(ctx, "room", room, side, a.reps, a.warmup))
    room.close()
    ctx.close()

    for r in rows:
        line = json.dumps(r)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
