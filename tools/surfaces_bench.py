#!/usr/bin/env python3
"""Component surfaces (sdfgpu_component_surfaces_device / CollisionMapGrid::ExtractComponentSurfaces) timings: one JSON line per
case, also appended to profiles/surfaces_bench.jsonl with --out.  The labels come from sdfgpu_components_bits_device on the same
scene and stay in HBM, and the indices land in a device buffer sized from a counts-only call; HIP events bracket the call on the
current stream (it reads back the total once and ends with the read-back of the counts, so the events cover the whole
computation); median of `--reps` after `--warmup`.  Three modes per scene: counts only, every component (select "all") and the
filled ones (select "filled").  Each case also times the components call on the same bits (components_ms) and reports the ratio;
the aim is counts + indices in at most 2x the components call ("aim_met").
usage: surfaces_bench.py [--n N] [--reps R] [--warmup W] [--only name,...] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdf_tools_amd import capi, synth  # noqa: E402


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def device_case(ctx, name, shape, mask_cpu, reps, warmup):
    n = int(np.prod(shape))
    bits = torch.from_numpy(capi.pack_bits_host(mask_cpu).view(np.int32)).cuda()
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    k = ctx.components_bits_device(bits.data_ptr(), shape, labels.data_ptr(), s)
    cc_med, _ = _time(lambda: ctx.components_bits_device(bits.data_ptr(), shape, labels.data_ptr(), s), reps, warmup)
    rows = []
    for mode in ("counts_only", "all", "filled"):
        d_sel = bits.data_ptr() if mode == "filled" else None
        _, total = ctx.component_surfaces_device(labels.data_ptr(), shape, k, d_sel, stream=s, counts_only=True)
        if mode == "counts_only":
            def fn():
                return ctx.component_surfaces_device(labels.data_ptr(), shape, k, d_sel, stream=s, counts_only=True)
        else:
            idx = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")

            def fn():
                return ctx.component_surfaces_device(labels.data_ptr(), shape, k, d_sel, d_indices=idx.data_ptr(), capacity=total, stream=s)
        med, mn = _time(fn, reps, warmup)
        row = {"case": name, "shape": list(shape), "path": "device", "mode": mode, "components": int(k), "surface_voxels": int(total),
               "ms_median": round(med, 4), "ms_min": round(mn, 4), "reps": reps, "components_ms": round(cc_med, 4),
               "ratio_to_components": round(med / cc_med, 2)}
        if mode != "counts_only":
            row["aim_met"] = bool(med <= 2.0 * cc_med)
        rows.append(row)
        idx = None
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    out = open(a.out, "a") if a.out else None
    ctx = capi.SdfGpu(0)
    dev = torch.device("cuda", 0)
    scenes = [
        ("bernoulli_0.5", lambda s: synth.bernoulli_mask(s, 0.5, 1)),
        ("bernoulli_0.3116", lambda s: synth.bernoulli_mask(s, 0.3116, 1)),
        ("room", lambda s: synth.room_mask_torch(s, dev).cpu().numpy()),
        ("solid_boxes", lambda s: synth.tutorial_boxes_mask_torch(s, dev, True).cpu().numpy()),
    ]
    for scene, mk in scenes:
        name = "%s_%d" % (scene, a.n)
        if only and name not in only:
            continue
        shape = (a.n,) * 3
        for r in device_case(ctx, name, shape, mk(shape), a.reps, a.warmup):
            print(json.dumps(r), flush=True)
            if out:
                out.write(json.dumps(r) + "\n")
                out.flush()
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
