#!/usr/bin/env python3
"""Component topology (sdfgpu_component_topology_device / CollisionMapGrid::ComputeComponentTopology) timings: one JSON line per
case, also appended to profiles/topology_bench.jsonl with --out.  Device-resident cases: the labels come from
sdfgpu_components_bits_device on the same scene and stay in HBM; HIP events bracket the topology call on the current stream (the
call reads back the node count once and ends with the read-back of the counters, so the events cover the whole computation);
median of `--reps` after `--warmup`.  Each case also times the components call on the same bits (components_ms) and reports the
ratio.  Two selections: every component (select "all") and the filled ones (ignore_empty_components, select "filled").  The host
case times the in-place CollisionMapGrid call at 512^3 with the wall clock (labels and classes gathered from the 8-byte records on
the host, up through the pinned staging chunks), components already valid.  --restated N also times the single-core C++
restatement (tests/topology_restated.cpp) at N^3 for comparison.
usage: topology_bench.py [--reps R] [--warmup W] [--only name,...] [--restated N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

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
    for select in ("all", "filled"):
        d_sel = bits.data_ptr() if select == "filled" else None
        counts = ctx.component_topology_device(labels.data_ptr(), shape, k, d_sel, s)
        med, mn = _time(lambda: ctx.component_topology_device(labels.data_ptr(), shape, k, d_sel, s), reps, warmup)
        rows.append({"case": name, "shape": list(shape), "path": "device", "select": select, "components": int(k),
                     "surface_vertex_nodes": int(counts[:, 0].sum()), "surfaces": int(counts[:, 4].sum()),
                     "ms_median": round(med, 4), "ms_min": round(mn, 4), "reps": reps, "components_ms": round(cc_med, 4),
                     "ratio_to_components": round(med / cc_med, 2)})
    return rows


def host_case(name, n, reps, warmup):
    from sdf_tools_amd._bindings import load_pysdf_tools

    m = load_pysdf_tools()
    occ = synth.bernoulli_mask((n, n, n), 0.5, 7).astype(np.float32)
    g = m.CollisionMapGrid(m.Isometry3d([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]), "world", 0.01, n, n, n,
                           m.COLLISION_CELL(0.0))
    g.SetOccupancyFromNumpy(occ)
    g.UpdateConnectedComponents()
    ms, res = [], {}
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        res = g.ComputeComponentTopology(True, True, False)       # (components valid: the update early-outs)
        t1 = time.perf_counter()
        if i >= warmup:
            ms.append((t1 - t0) * 1e3)
    return {"case": name, "shape": [n, n, n], "path": "host in-place CollisionMapGrid", "select": "filled", "components_in_map": len(res),
            "ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "reps": reps,
            "note": "labels (4 B) and classes (1/8 B) up per voxel from the 8-byte records, counters down"}


def restated_case(name, shape, mask_cpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_components_cpu import restated_labels
    from test_topology_cpu import restated_counts

    labels, k = restated_labels(mask_cpu)
    t0 = time.perf_counter()
    restated_counts(labels, max_label=k)
    return {"case": name, "shape": list(shape), "path": "restatement, one host core", "select": "all",
            "ms": round((time.perf_counter() - t0) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--restated", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    out = open(a.out, "a") if a.out else None

    def emit(r):
        print(json.dumps(r), flush=True)
        if out:
            out.write(json.dumps(r) + "\n")
            out.flush()

    ctx = capi.SdfGpu(0)
    dev = torch.device("cuda", 0)
    scenes = [
        ("bernoulli_0.5", lambda s: synth.bernoulli_mask(s, 0.5, 1)),
        ("bernoulli_0.3116", lambda s: synth.bernoulli_mask(s, 0.3116, 1)),
        ("room", lambda s: synth.room_mask_torch(s, dev).cpu().numpy()),
        ("solid_boxes", lambda s: synth.tutorial_boxes_mask_torch(s, dev, True).cpu().numpy()),
    ]
    for n in (256, 512):
        for scene, mk in scenes:
            name = "%s_%d" % (scene, n)
            if only and name not in only:
                continue
            shape = (n, n, n)
            for r in device_case(ctx, name, shape, mk(shape), a.reps, a.warmup):
                emit(r)
            torch.cuda.empty_cache()
    if not only or "host_collision_map_512" in only:
        emit(host_case("host_collision_map_512", 512, max(3, a.reps // 2), 1))
    if a.restated:
        for scene, mk in scenes:
            shape = (a.restated,) * 3
            emit(restated_case("%s_%d" % (scene, a.restated), shape, mk(shape)))
    ctx.close()


if __name__ == "__main__":
    main()
