#!/usr/bin/env python3
"""Connected components (sdfgpu_components_bits_device / CollisionMapGrid::UpdateConnectedComponents) timings: one JSON line per
case.  Device-resident cases: bits and labels in HBM, HIP events around the call on the current stream (the call ends with the
read-back of K, so the events bracket the whole labelling), median of `--reps` after `--warmup`.  The host case times the in-place
CollisionMapGrid call at 512^3 with the wall clock (classify on the host, 1 bit / voxel up, labels down through the pinned
staging chunks into the 8-byte records).

Bytes per voxel are the model's, not a counter: 4 (k_cc_local label store) + 4 (k_cc_flatten load) + 4 + 4 (k_cc_relabel load +
store) + 2 x 1/8 (bits read by k_cc_local and k_cc_merge) + 4 x 1/32 x 4 (root flags and word ranks, written and read) = 16.75;
flatten's chain loads and the rewrites of non-root labels come on top.  frac_8TBs = model bytes / time / 8 TB/s.
usage: components_bench.py [--reps R] [--warmup W] [--only name,...]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdf_tools_amd import capi, synth  # noqa: E402

MODEL_BYTES_PER_VOXEL = 16.75


def bits_of(mask_cpu):
    return torch.from_numpy(capi.pack_bits_host(mask_cpu).view(np.int32)).cuda()


def device_case(ctx, name, shape, mask_cpu, reps, warmup):
    n = int(np.prod(shape))
    bits = bits_of(mask_cpu)
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    k = 0
    for _ in range(warmup):
        k = ctx.components_bits_device(bits.data_ptr(), shape, labels.data_ptr(), s)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        k = ctx.components_bits_device(bits.data_ptr(), shape, labels.data_ptr(), s)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    return {"case": name, "shape": list(shape), "path": "device", "components": int(k), "ms_median": round(med, 4),
            "ms_min": round(float(np.min(ms)), 4), "reps": reps, "bytes_per_voxel_model": MODEL_BYTES_PER_VOXEL,
            "frac_8TBs": round(n * MODEL_BYTES_PER_VOXEL / (med * 1e-3) / 8e12, 4)}


def host_case(name, n, reps, warmup):
    from sdf_tools_amd._bindings import load_pysdf_tools

    m = load_pysdf_tools()
    occ = synth.bernoulli_mask((n, n, n), 0.5, 7).astype(np.float32)
    g = m.CollisionMapGrid(m.Isometry3d([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]), "world", 0.01, n, n, n,
                           m.COLLISION_CELL(0.0))
    ms, k = [], 0
    for i in range(warmup + reps):
        g.SetOccupancyFromNumpy(occ)                            # (untimed: clears the stored components)
        t0 = time.perf_counter()
        k = g.UpdateConnectedComponents()
        t1 = time.perf_counter()
        if i >= warmup:
            ms.append((t1 - t0) * 1e3)
    med = float(np.median(ms))
    return {"case": name, "shape": [n, n, n], "path": "host in-place CollisionMapGrid", "components": int(k),
            "ms_median": round(med, 3), "ms_min": round(float(np.min(ms)), 3), "reps": reps,
            "pcie_bytes_per_voxel": 4.125, "note": "bits up (1/8 B), labels down (4 B) into 8-byte records"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    ctx = capi.SdfGpu(0)
    dev = torch.device("cuda", 0)
    cases = [
        ("bernoulli_0.5_256", (256,) * 3, lambda s: synth.bernoulli_mask(s, 0.5, 1)),
        ("bernoulli_0.5_512", (512,) * 3, lambda s: synth.bernoulli_mask(s, 0.5, 1)),
        ("bernoulli_0.3116_512", (512,) * 3, lambda s: synth.bernoulli_mask(s, 0.3116, 1)),
        ("room_512", (512,) * 3, lambda s: synth.room_mask_torch(s, dev).cpu().numpy()),
        ("solid_boxes_512", (512,) * 3, lambda s: synth.tutorial_boxes_mask_torch(s, dev, True).cpu().numpy()),
        ("bernoulli_0.5_1024", (1024,) * 3, lambda s: synth.bernoulli_mask(s, 0.5, 1)),
    ]
    for name, shape, mk in cases:
        if only and name not in only:
            continue
        r = device_case(ctx, name, shape, mk(shape), a.reps, a.warmup)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if not only or "host_collision_map_512" in only:
        print(json.dumps(host_case("host_collision_map_512", 512, max(3, a.reps // 2), 1)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
