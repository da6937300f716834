#!/usr/bin/env python3
"""Shape rasteriser timings (sdfgpu_rasterize_shapes_device): one JSON line per scene, also appended to profiles/raster_bench.jsonl
with --out.  Device-resident, 512^3 at resolution 0.01, bits only (the 16 MiB field sdfgpu_build_bits_device reads).  Scenes: the
room, the tutorial's solid boxes and the three solid spheres of sdf_tools_amd/synth.py expressed as shape lists (the same solids in
metres: a slab of the mask from cell a to cell b is the box [a res, b res]), and 65 536 octomap-like boxes of 1 - 3 voxels.
Per line, medians of `--reps` after `--warmup`, each between two events of the caller on one stream:
  raster_ms     the rasteriser call (memset of the status word + three kernels)
  memset_ms     a memset of the 16 MiB bit field: the bytes the call must write
  torch_ms      the same scene rasterised by synth.py's torch code on the device (byte mask; none for the octomap scene)
  build_ms      sdfgpu_build_bits_device on the rasteriser's bits: the build the rasteriser feeds
  filled        set bits of the result
The aim (no assertion): on the room, raster_ms < build_ms.
usage: raster_bench.py [--n N] [--reps R] [--warmup W] [--only name,...] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdf_tools_amd import capi, synth  # noqa: E402

RES = 0.01


def _box(n, lo, hi):
    """the mask slab [lo, hi) cells per axis as a box record (cells a .. b - 1 are met by the box [a res, b res] shrunk by a hair)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    pose = np.eye(4)
    pose[:3, 3] = (lo + hi) * 0.5 * RES
    return (capi.SHAPE_BOX, 1, (hi - lo) * RES - 1e-6, pose)


def room_shapes(n):
    f = lambda v: int(v * n)                                                   # noqa: E731
    t = max(f(0.02), 1)
    items = [_box(n, (0, 0, 0), (n, n, t)), _box(n, (0, 0, 0), (t, n, n)), _box(n, (0, 0, 0), (n, t, n)),
             _box(n, (f(0.3), f(0.3), f(0.35)), (f(0.7), f(0.6), f(0.38)))]
    for x, y in ((0.31, 0.31), (0.68, 0.31), (0.31, 0.58), (0.68, 0.58)):
        items.append(_box(n, (f(x), f(y), 0), (f(x) + t, f(y) + t, f(0.35))))
    items.append(_box(n, (f(0.8), f(0.1), f(0.5)), (f(0.98), f(0.9), f(0.55))))
    return capi.make_shapes(items)


def boxes_shapes(n):
    items = []
    for x0, x1, y0, y1, z0, z1 in ((0.5, 0.7, 0.5, 0.6, 0.0, 0.5), (0.5, 0.75, 0.2, 0.4, 0.25, 0.5)):
        items.append(_box(n, (int(x0 * n), int(y0 * n), int(z0 * n)), (int(x1 * n), int(y1 * n), int(z1 * n))))
    return capi.make_shapes(items)


def spheres_shapes(n):
    items = []
    for cx, cy, cz, r in ((0.3, 0.3, 0.3, 0.12), (0.7, 0.6, 0.4, 0.2), (0.5, 0.8, 0.8, 0.08)):
        pose = np.eye(4)
        pose[:3, 3] = (np.array([cx, cy, cz]) * n + 0.5) * RES
        items.append((capi.SHAPE_SPHERE, 1, (r * n * RES,), pose))
    return capi.make_shapes(items)


def octomap_shapes(n, count=capi.MAX_SHAPES, seed=5):
    rng = np.random.default_rng(seed)
    out = np.zeros(count, capi.SHAPE_DTYPE)
    out["type"], out["object_id"] = capi.SHAPE_BOX, 1
    out["dims"] = rng.integers(1, 4, (count, 1)) * RES
    pose = np.tile(np.eye(4).reshape(-1), (count, 1))
    # a surface-like cloud: boxes near a wavy sheet through the volume
    xy = rng.uniform(0.0, n * RES, (count, 2))
    z = (0.5 + 0.2 * np.sin(xy[:, 0] * 3.0) * np.cos(xy[:, 1] * 2.0)) * n * RES + rng.normal(0.0, 2 * RES, count)
    pose[:, 3], pose[:, 7], pose[:, 11] = xy[:, 0], xy[:, 1], z
    out["pose"] = pose
    return out


SCENES = {"room": (room_shapes, lambda s: synth.room_mask_torch(s)), "boxes": (boxes_shapes, lambda s: synth.tutorial_boxes_mask_torch(s)),
          "spheres": (spheres_shapes, lambda s: synth.solid_spheres_mask_torch(s)), "octomap": (octomap_shapes, None)}


def _timed(fn, reps, warmup):
    ms = []
    for it in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    n, shape = args.n, (args.n,) * 3
    ctx = capi.SdfGpu(0)
    stream = torch.cuda.current_stream().cuda_stream
    words = (n ** 3 + 31) // 32
    d_bits = torch.zeros(words, dtype=torch.int32, device="cuda")
    d_sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
    lines = []
    for name, (make, torch_mask) in SCENES.items():
        if only and name not in only:
            continue
        shapes = make(n)
        d_shapes = torch.from_numpy(shapes.view(np.uint8).reshape(-1).copy()).cuda()
        row = {"scene": name, "n": n, "shapes": int(len(shapes)), "bit_field_bytes": words * 4}
        assert ctx.rasterize_shapes_device(d_shapes.data_ptr(), len(shapes), np.eye(4), RES, shape, d_bits=d_bits.data_ptr(), check=True, stream=stream) == -1
        row["raster_ms"] = _timed(lambda: ctx.rasterize_shapes_device(d_shapes.data_ptr(), len(shapes), np.eye(4), RES, shape, d_bits=d_bits.data_ptr(),
                                                                      stream=stream), args.reps, args.warmup)
        v = d_bits.to(torch.int64) & 0xFFFFFFFF
        v = v - ((v >> 1) & 0x55555555)
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
        v = (v + (v >> 4)) & 0x0F0F0F0F
        row["filled"] = int((((v * 0x01010101) >> 24) & 0xFF).sum().item())
        del v
        scratch = torch.empty_like(d_bits)
        row["memset_ms"] = _timed(lambda: scratch.zero_(), args.reps, args.warmup)
        del scratch
        if torch_mask is not None:
            row["torch_ms"] = _timed(lambda: torch_mask(shape), args.reps, args.warmup)
            row["torch_filled"] = int(torch_mask(shape).sum().item())
        ctx.set_option("policy_reset", 1)
        row["build_ms"] = _timed(lambda: ctx.build_bits_device(d_bits.data_ptr(), shape, d_sdf.data_ptr(), RES, False, stream), args.reps, args.warmup)
        row["path"] = str(ctx.last_path())
        lines.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
