#!/usr/bin/env python3
"""Interpolated-gradient (sdfgpu_query_gradients_device / DeviceSignedDistanceField::QueryGradientsBatch) timings: one JSON line per
case, also appended to --out (profiles/query_bench.jsonl).

Fields: device-resident at --size^3 (default 512, res 0.01, identity frame), the room and the solid-boxes scenes.
Point sets per field: "uniform", --points points uniform over the grid; "planner", --planner points within 2 cells of a surface
(|sdf| <= 2 res at the cell).
Cases per point set:
  query_points     the existing sdfgpu_query_points_device (distance + grid-aligned gradient, edge gradients on): the yardstick
  autodiff         SDFGPU_QUERY_AUTODIFF_GRADIENT (distance + exact gradient)
  smooth_res8      SDFGPU_QUERY_SMOOTH_GRADIENT, window res / 8 (the reference's own test)
  smooth_2res      SDFGPU_QUERY_SMOOTH_GRADIENT, window 2 res
  boundary         SDFGPU_QUERY_DISTANCE_TO_BOUNDARY
Per case:
  kernel_ms        between HIP events on the current stream; median of --reps after --warmup; points_per_s from it
  vs_query_points  kernel_ms / the yardstick's on the same points
  host_ms          QueryGradientsNumpyHost (SignedDistanceField::QueryGradient4d, one core, host clock) on --host-sample points,
                   scaled to the batch; the sample's host results are checked bit for bit against the device's
usage: query_bench.py [--size N] [--points N] [--planner N] [--reps R] [--warmup W] [--host-sample N] [--out FILE]"""
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

SCENES = ("room", "solid_boxes")
CASES = ("query_points", "autodiff", "smooth_res8", "smooth_2res", "boundary")


def timed(call, reps, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times))


def run_scene(scene, args, ctx, m, res):
    n = args.size
    shape = (n, n, n)
    mt = synth.tutorial_boxes_mask_torch(shape, "cuda", True) if scene == "solid_boxes" else synth.room_mask_torch(shape, "cuda")
    field = m.DeviceSignedDistanceField(m.Isometry3d(np.eye(4)), "world", res, n, n, n, math.inf)
    ptr = field.DevicePointer()
    stream = torch.cuda.current_stream().cuda_stream
    ctx.build_device(mt.data_ptr(), shape, ptr, res, False, stream)
    torch.cuda.synchronize()
    del mt
    host = field.Host()
    sdf = host.GetRawDataNumpy()
    rng = np.random.default_rng(SCENES.index(scene))
    near = np.argwhere(np.abs(sdf) <= 2.0 * res)
    sets = {"uniform": rng.uniform(0.0, 1.0, (args.points, 3)) * np.array(shape) * res}
    pick = near[rng.integers(0, len(near), args.planner)]
    sets["planner"] = (pick + rng.uniform(0.0, 1.0, pick.shape)) * res
    del sdf, near
    eye = np.eye(4)
    rows = []
    for set_name, pts in sets.items():
        npts = len(pts)
        d_pts = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
        d_val = torch.empty(npts, dtype=torch.float64, device="cuda")
        d_grad = torch.empty((npts, 3), dtype=torch.float64, device="cuda")
        d_st = torch.empty(npts, dtype=torch.uint8, device="cuda")
        base_ms = None
        for case in CASES:
            if case == "query_points":
                def call():
                    ctx.query_points_device(ptr, shape, res, d_pts.data_ptr(), npts, d_val.data_ptr(), d_grad.data_ptr(), d_st.data_ptr(),
                                            eye, np.eye(3), math.inf, True, stream)
                kind, window = None, 0.0
            else:
                kind, window = {"autodiff": (capi.QUERY_AUTODIFF_GRADIENT, 0.0), "smooth_res8": (capi.QUERY_SMOOTH_GRADIENT, res / 8),
                                "smooth_2res": (capi.QUERY_SMOOTH_GRADIENT, 2 * res),
                                "boundary": (capi.QUERY_DISTANCE_TO_BOUNDARY, 0.0)}[case]

                def call():
                    ctx.query_gradients_device(ptr, shape, res, d_pts.data_ptr(), npts, eye, kind, window, math.inf, d_val.data_ptr(),
                                               d_grad.data_ptr(), d_st.data_ptr(), stream)
            kernel_ms, kernel_min = timed(call, args.reps, args.warmup)
            row = {"scene": scene, "points_set": set_name, "case": case, "size": n, "points": npts, "window": window,
                   "reps": args.reps, "kernel_ms": round(kernel_ms, 4), "kernel_ms_min": round(kernel_min, 4),
                   "points_per_s": round(npts / (kernel_ms * 1e-3))}
            if case == "query_points":
                base_ms = kernel_ms
            else:
                row["vs_query_points"] = round(kernel_ms / base_ms, 2)
                val, grad, st = d_val.cpu().numpy(), d_grad.cpu().numpy(), d_st.cpu().numpy()
                k = min(args.host_sample, npts)
                t0 = time.perf_counter()
                hv, hg, hs = host.QueryGradientsNumpyHost(pts[:k], kind, window)
                host_ms = (time.perf_counter() - t0) * 1e3 * (npts / k)
                same = bool(np.array_equal(hv.view(np.uint64), val[:k].view(np.uint64)) and
                            np.array_equal(hg.view(np.uint64), grad[:k].view(np.uint64)) and np.array_equal(hs, st[:k]))
                row.update({"statuses": {str(s): int((st == s).sum()) for s in np.unique(st)}, "host_ms": round(host_ms, 2),
                            "host_sample": k, "host_scaled": k < npts, "speedup_vs_host": round(host_ms / kernel_ms, 1),
                            "host_sample_bit_equal": same})
            row["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del d_pts, d_val, d_grad, d_st
    del host, field
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--planner", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=20000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    m = load_pysdf_tools()
    ctx = capi.SdfGpu(0)
    rows = []
    for scene in SCENES:
        rows += run_scene(scene, args, ctx, m, 0.01)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not all(r.get("host_sample_bit_equal", True) for r in rows):
        sys.exit("device results differ from the host core")


if __name__ == "__main__":
    main()
