#!/usr/bin/env python3
"""Resample timings (sdfgpu_resample_cells_device / CollisionMapGrid::Resample): one JSON line per case, also appended to
profiles/resample_bench.jsonl with --out.  Device-resident 8- and 16-byte cells; 512^3 at new / old resolution 2, 4, 1.5 and 0.5
and 256^3 at 2; the occupancies come from the room scene (synth.room_mask_torch) and from Bernoulli(0.5)
(synth.bernoulli_mask_torch), the index word holds the linear index + 1.  Per line, medians of `--reps` after `--warmup`:
  winner_ms / gather_ms   memset + k_rs_winner and k_rs_gather, from the library's events (option "resample_timing"), with the
                          pre-reduced atomics (the default) and with one atomic per source cell ("plain_*")
  call_ms                 the whole device call between two events of the caller
  dtod_ms                 hipMemcpyDtoD of (source + result) bytes in the same process: what a plain copy of that volume costs
  class_ms                the host-to-host class call (pysdf_tools Resample: upload, kernels, download), 8- and 16-byte classes,
                          room scene, ratios >= 1
and once, as the host baseline, the restatement's loop (tests/resample_restated.cpp) on one core at 256^3 ("host_loop_ms").
There is no pass / fail threshold.
usage: resample_bench.py [--reps R] [--warmup W] [--only name,...] [--out FILE] [--no-class] [--no-host-loop]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdf_tools_amd import capi, synth  # noqa: E402

CELL = 0.05
CASES = [(512, 2.0), (512, 4.0), (512, 1.5), (512, 0.5), (256, 2.0)]


def _median(v):
    return float(np.median(v))


def _cells(n, cb, scene):
    """int32 [n, n, n, cb / 4] on the device: occupancy (1.0 filled, 0.0 free) | linear index + 1 | (object id | segment)"""
    shape = (n, n, n)
    mask = synth.room_mask_torch(shape) if scene == "room" else synth.bernoulli_mask_torch(shape, 0.5, 1)
    rec = torch.zeros(shape + (cb // 4,), dtype=torch.int32, device="cuda")
    rec[..., 0] = torch.where(mask != 0, torch.tensor(1.0, device="cuda"), torch.tensor(0.0, device="cuda")).view(torch.int32)
    lin = torch.arange(1, n ** 3 + 1, dtype=torch.int64, device="cuda").view(shape)
    rec[..., 1] = lin.to(torch.int32)
    if cb == 16:
        rec[..., 2] = (mask != 0).to(torch.int32) * 3
        rec[..., 3] = (lin % 1000).to(torch.int32)
    return rec


def device_case(ctx, n, ratio, cb, scene, reps, warmup):
    shape = (n, n, n)
    rshape = tuple(int(np.ceil(n * CELL / (CELL * ratio))) for _ in range(3))
    src = _cells(n, cb, scene)
    dst = torch.empty(rshape + (cb // 4,), dtype=torch.int32, device="cuda")
    fill = np.zeros(cb, np.uint8)
    stream = torch.cuda.current_stream().cuda_stream
    row = {"case": "%d^3 x %g" % (n, ratio), "n": n, "ratio": ratio, "cell_bytes": cb, "scene": scene, "result": list(rshape)}
    ctx.set_option("resample_timing", 1)
    for plain in (0, 1):
        ctx.set_option("resample_plain_atomics", plain)
        win, gat, call = [], [], []
        for it in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.resample_cells_device(src.data_ptr(), shape, CELL, np.eye(4), np.eye(4), 1.0 / (CELL * ratio), dst.data_ptr(), rshape, fill, cb,
                                      stream=stream)
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                w, g = ctx.debug_resample_times()
                win.append(w), gat.append(g), call.append(e0.elapsed_time(e1))
        pre = "plain_" if plain else ""
        row[pre + "winner_ms"], row[pre + "gather_ms"], row[pre + "call_ms"] = _median(win), _median(gat), _median(call)
    ctx.set_option("resample_plain_atomics", 0)
    ctx.set_option("resample_timing", 0)
    written = ctx.resample_cells_device(src.data_ptr(), shape, CELL, np.eye(4), np.eye(4), 1.0 / (CELL * ratio), dst.data_ptr(), rshape, fill, cb,
                                        count=True, stream=stream)
    row["cells_written"] = written
    # a plain device-to-device copy of the same volume
    a = torch.empty(src.numel() + dst.numel(), dtype=torch.int32, device="cuda")
    b = torch.empty_like(a)
    ms = []
    for it in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    row["dtod_ms"] = _median(ms)
    row["bytes"] = int(a.numel()) * 4
    return row, src


def class_ms(src, n, ratio, cb, reps):
    """host to host through the class: records from `src` (device tensor) into a grid, Resample, nothing else timed"""
    from sdf_tools_amd._bindings import load_pysdf_tools
    m = load_pysdf_tools()
    ident = m.Isometry3d(np.eye(4))
    if cb == 8:
        g = m.CollisionMapGrid(ident, "bench", CELL, n, n, n, m.COLLISION_CELL(0.0, 0))
    else:
        g = m.TaggedObjectCollisionMapGrid(ident, "bench", CELL, n, n, n, m.TAGGED_OBJECT_COLLISION_CELL(0.0, 0))
    g.SetRawCellsNumpy(src.cpu().numpy().view(np.uint8).reshape(n, n, n, cb))
    ms = []
    for it in range(reps + 1):
        t0 = time.perf_counter()
        r = g.Resample(CELL * ratio)
        if it:
            ms.append((time.perf_counter() - t0) * 1e3)
        del r
    return _median(ms)


def host_loop_ms(n=256, ratio=2.0, cb=8):
    import resample_restated as R
    cells = R.payload((n, n, n), cb)
    R.restated(R.payload((2, 2, 2), cb), CELL, np.eye(4), CELL * 2, R.oob_record(cb))      # (compiled before the clock starts)
    t0 = time.perf_counter()
    R.restated(cells, CELL, np.eye(4), CELL * ratio, R.oob_record(cb))
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-class", action="store_true")
    ap.add_argument("--no-host-loop", action="store_true")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    ctx = capi.SdfGpu(0)
    lines = []
    for n, ratio in CASES:
        for scene in ("room", "bernoulli"):
            for cb in (8, 16):
                name = "%d-%g-%s-%d" % (n, ratio, scene, cb)
                if only and name not in only:
                    continue
                row, src = device_case(ctx, n, ratio, cb, scene, args.reps, args.warmup)
                if not args.no_class and scene == "room" and ratio >= 1.0:          # (the 1024^3 result of x 0.5 is 8 - 17 GB of host memory)
                    row["class_ms"] = class_ms(src, n, ratio, cb, 3)
                del src
                torch.cuda.empty_cache()
                lines.append(row)
                print(json.dumps(row), flush=True)
    if not args.no_host_loop and not only:
        row = {"case": "host loop 256^3 x 2", "cell_bytes": 8, "host_loop_ms": host_loop_ms()}
        lines.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
