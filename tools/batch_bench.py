"""Batched build against the loop of single builds it replaces.

Device-resident, HIP events around REPS repetitions after a warm-up, inputs rotated over ROT buffers.  Per shape, batch size and
scene it records t_single (one sdfgpu_build_device), t_loop (B x sdfgpu_build_device back to back on one stream: what a caller
had before the batch entry points) and t_batch (one sdfgpu_build_batch_device), and for 16 objects in 64^3 the per-id
sdfgpu_build_tagged_cells loop against sdfgpu_build_tagged_objects, host to host.  One JSON line per case is appended to
profiles/batch_bench.jsonl.

    python tools/batch_bench.py [--reps 200] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdf_tools_amd import capi, synth  # noqa: E402

SHAPES = [(64, 64, 64), (40, 40, 40), (100, 100, 50), (25, 20, 15)]
BATCHES = [1, 8, 32, 128]
ROT = 3


def boxes_scene(shape, seed):
    """Boxes in free space: a structured scene with far-field voxels."""
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, np.uint8)
    for _ in range(6):
        lo = [int(rng.integers(0, max(1, s - 2))) for s in shape]
        hi = [min(s, l + int(rng.integers(1, max(2, s // 4)))) for s, l in zip(shape, lo)]
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    return m


def timed(fn, reps, warmup=20):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="64^3 and 25x20x15 only")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = capi.SdfGpu(0)
    stream = torch.cuda.current_stream().cuda_stream
    out_path = os.path.join(ROOT, "profiles", "batch_bench.jsonl")
    rows = []
    for shape in (SHAPES[::3] if args.quick else SHAPES):
        n = int(np.prod(shape))
        for scene in ("bernoulli0.5", "boxes"):
            for B in BATCHES:
                bufs = []
                for r in range(ROT):
                    ms = [synth.bernoulli_mask(shape, 0.5, 100 * r + b) if scene == "bernoulli0.5" else boxes_scene(shape, 100 * r + b) for b in range(B)]
                    bufs.append(torch.from_numpy(np.stack(ms)).cuda())
                out = torch.empty((B,) + shape, dtype=torch.float32, device="cuda")
                reps = max(20, args.reps // max(1, B // 8))

                def single(i):
                    ctx.build_device(bufs[i % ROT].data_ptr(), shape, out.data_ptr(), 0.01, False, stream)

                def loop(i):
                    base, o = bufs[i % ROT].data_ptr(), out.data_ptr()
                    for b in range(B):
                        ctx.build_device(base + b * n, shape, o + 4 * b * n, 0.01, False, stream)

                def batch(i):
                    ctx.build_batch_device(bufs[i % ROT].data_ptr(), B, shape, out.data_ptr(), 0.01, False, stream)

                ctx.set_option("policy_reset", 1)
                row = {"shape": list(shape), "scene": scene, "B": B, "reps": reps, "device": torch.cuda.get_device_name(0),
                       "t_single_ms": timed(single, args.reps), "t_loop_ms": timed(loop, reps), "t_batch_ms": timed(batch, reps)}
                row["loop_over_batch"] = row["t_loop_ms"] / row["t_batch_ms"]
                row["batch_over_single"] = row["t_batch_ms"] / row["t_single_ms"]
                rows.append(row)
                print(json.dumps(row), flush=True)
    # tagged: 16 objects in 64^3, host to host
    shape = (64, 64, 64)
    rng = np.random.default_rng(3)
    cells = np.zeros(shape, dtype=np.dtype([("occupancy", "<f4"), ("component", "<u4"), ("object_id", "<u4"), ("convex_segment", "<u4")]))
    cells["occupancy"] = (rng.random(shape) < 0.3).astype(np.float32)
    cells["object_id"] = rng.integers(1, 17, size=shape)
    ids = list(range(1, 17))

    def host_timed(fn, reps=20):
        fn()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t) / reps * 1e3

    def per_id():
        for k, i in enumerate(ids):
            ctx.build_tagged_cells(cells if k == 0 else None, shape, object_mode=2, object_ids=[i], resolution=0.01)

    row = {"shape": list(shape), "scene": "tagged16", "B": 16, "device": torch.cuda.get_device_name(0),
           "t_loop_ms": host_timed(per_id), "t_batch_ms": host_timed(lambda: ctx.build_tagged_objects(cells, shape, ids, resolution=0.01))}
    row["loop_over_batch"] = row["t_loop_ms"] / row["t_batch_ms"]
    rows.append(row)
    print(json.dumps(row), flush=True)
    with open(out_path, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
