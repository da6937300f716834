#!/usr/bin/env python3
"""Projection out of collision (sdfgpu_project_points_device / DeviceSignedDistanceField::ProjectBatch) timings: one JSON line per
case, also appended to profiles/projection_bench.jsonl with --out.

Cases, on a device-resident field at --size^3 (default 512, res 0.01, identity frame, stepsize_multiplier 1/8):
  uniform     --points points uniform over the room scene (most are free and take no step), minimum_distance 0
  deep        --points points inside the obstacles of the solid-boxes scene (long walks), minimum_distance 0
  planner     --planner points within 2 cells of a surface of the room scene (|sdf| <= 2 res at the cell), minimum_distance 2 res
Per case:
  kernel_ms       sdfgpu_project_points_device between HIP events on the current stream; median of --reps after --warmup
  points_per_s, steps_per_s   from kernel_ms and the total of the steps the walks took
  steps_max, steps_p50, steps_p99   the step histogram; statuses: the count per SDFGPU_PROJECT_* status
  wave_steps_mean, lane_efficiency   the mean over 64-point waves of the wave's longest walk, and steps_mean over it
  host_ms         the counted host walk (SignedDistanceField::ProjectCounted4d through ProjectOutOfCollisionNumpyHost, one core,
                  host clock) of the same batch, measured on --host-sample points and scaled to the batch (host_scaled = true)
                  when the batch is larger; the host results of the sample are checked bit for bit against the device's
usage: projection_bench.py [--size N] [--points N] [--planner N] [--reps R] [--warmup W] [--host-sample N] [--only case,...] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdf_tools_amd import capi, synth  # noqa: E402
from sdf_tools_amd._bindings import load_pysdf_tools  # noqa: E402

CASES = ("uniform", "deep", "planner")


def points_for(case, mask, sdf, res, n, rng):
    size = np.array(mask.shape, np.float64) * res
    if case == "uniform":
        return rng.uniform(0.0, 1.0, (n, 3)) * size
    if case == "deep":
        cells = np.argwhere(mask != 0)
        pick = cells[rng.integers(0, len(cells), n)]
        return (pick + rng.uniform(0.0, 1.0, pick.shape)) * res
    near = np.argwhere(np.abs(sdf) <= 2.0 * res)
    pick = near[rng.integers(0, len(near), n)]
    return (pick + rng.uniform(0.0, 1.0, pick.shape)) * res


def run_case(case, args, ctx, m, res):
    n = args.size
    shape = (n, n, n)
    mt = (synth.tutorial_boxes_mask_torch(shape, "cuda", True) if case == "deep" else synth.room_mask_torch(shape, "cuda"))
    field = m.DeviceSignedDistanceField(m.Isometry3d(np.eye(4)), "world", res, n, n, n, math.inf)
    ptr = field.DevicePointer()
    stream = torch.cuda.current_stream().cuda_stream
    ctx.build_device(mt.data_ptr(), shape, ptr, res, False, stream)
    torch.cuda.synchronize()
    mask = mt.cpu().numpy()
    del mt
    host = field.Host()
    sdf = host.GetRawDataNumpy()
    rng = np.random.default_rng(CASES.index(case))
    npts = args.planner if case == "planner" else args.points
    md = 2.0 * res if case == "planner" else 0.0
    pts = points_for(case, mask, sdf, res, npts, rng)
    del sdf, mask
    eye = np.eye(4)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    d_out = torch.empty((npts, 3), dtype=torch.float64, device="cuda")
    d_st = torch.empty(npts, dtype=torch.uint8, device="cuda")
    d_sp = torch.empty(npts, dtype=torch.int32, device="cuda")

    def call():
        ctx.project_points_device(ptr, shape, res, d_pts.data_ptr(), npts, d_out.data_ptr(), eye, eye, md, 0.125, 0, False,
                                  d_st.data_ptr(), d_sp.data_ptr(), stream)

    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    kernel_ms = float(np.median(times))
    out, st, sp = d_out.cpu().numpy(), d_st.cpu().numpy(), d_sp.cpu().numpy()
    total_steps = int(sp.astype(np.int64).sum())
    # a wave of 64 consecutive points runs as long as its longest walk: steps_mean / wave_steps_mean is the share of lane-steps
    # doing work, the ceiling of what refilling finished lanes could recover
    pad = (-npts) % 64
    wave_steps = float(np.concatenate([sp, np.zeros(pad, sp.dtype)]).reshape(-1, 64).max(axis=1).mean())
    k = min(args.host_sample, npts)
    t0 = time.perf_counter()
    h_out, h_st, h_sp = host.ProjectOutOfCollisionNumpyHost(pts[:k], md, 0.125, 0, False)
    host_ms = (time.perf_counter() - t0) * 1e3 * (npts / k)
    same = bool(np.array_equal(h_out.view(np.uint64), out[:k].view(np.uint64)) and np.array_equal(h_st, st[:k]) and np.array_equal(h_sp, sp[:k]))
    row = {
        "case": case, "size": n, "points": npts, "minimum_distance": md, "stepsize_multiplier": 0.125, "reps": args.reps,
        "kernel_ms": round(kernel_ms, 4), "kernel_ms_min": round(float(np.min(times)), 4),
        "points_per_s": round(npts / (kernel_ms * 1e-3)), "steps_per_s": round(total_steps / (kernel_ms * 1e-3)),
        "steps_total": total_steps, "steps_max": int(sp.max()), "steps_p50": float(np.percentile(sp, 50)),
        "steps_p99": float(np.percentile(sp, 99)), "steps_mean": round(float(sp.mean()), 3),
        "wave_steps_mean": round(wave_steps, 3), "lane_efficiency": round(float(sp.mean()) / max(wave_steps, 1e-9), 3),
        "statuses": {str(s): int((st == s).sum()) for s in np.unique(st)},
        "host_ms": round(host_ms, 2), "host_sample": k, "host_scaled": k < npts, "speedup_vs_host": round(host_ms / kernel_ms, 1),
        "host_sample_bit_equal": same, "device": torch.cuda.get_device_name(0),
    }
    del host, field
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--planner", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=20000)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    m = load_pysdf_tools()
    ctx = capi.SdfGpu(0)
    rows = []
    for case in CASES:
        if args.only and case not in args.only.split(","):
            continue
        row = run_case(case, args, ctx, m, 0.01)
        print(json.dumps(row), flush=True)
        rows.append(row)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not all(r["host_sample_bit_equal"] for r in rows):
        sys.exit("device results differ from the host walk")


if __name__ == "__main__":
    main()
