#!/usr/bin/env python3
"""Local extrema and convex segments (sdfgpu_local_extrema_device, sdfgpu_convex_segments_cells / TaggedObjectCollisionMapGrid::
UpdateConvexSegments) timings: one JSON line per case, also appended to profiles/convex_segments_bench.jsonl with --out.

Per scene and size:
  extrema_ms       sdfgpu_local_extrema_device on a device-resident field (HIP events on the current stream around the call,
                   which reads back one count per doubling round); median of --reps after --warmup, with the doubling rounds,
                   cycles, longest cycle and longest basin-minimum -> cycle walk of the last call
  sdf_ms, components_ms   the SDF build (sdfgpu_build_device, virtual border) and the components (sdfgpu_components_bits_device)
                   of the same scene, device-resident: the yardstick of the aim (extrema + segments < 2 x their sum)
  host_ms          the whole in-place call on 16-byte tagged records (wall clock): upload, SDF build, extrema, segments, labels
                   scattered back (add_virtual_border = true, threshold 1.75 cells)
Scenes: room, solid_boxes, the reference's convex-segments scene tiled to size (the mask gives the occupancy; filled cells are
objects 1 / 2 / 0 by x thirds), and noise (the extrema of a uniform random field; the cells of a Bernoulli 0.5 mask).  The
segment kernels' own times come from a rocprofv3 --kernel-trace --stats run of this script (profiles/convex_kernel_stats.md).
--restated N times the single-core C++ restatement (tests/convex_segments_restated.cpp) at N^3 instead (no GPU needed).
usage: convex_segments_bench.py [--reps R] [--warmup W] [--sizes 256,512] [--only scene,...] [--no-host] [--restated N] [--out FILE]"""
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

SCENES = ("room", "solid_boxes", "convex_scene", "noise")


def mask_of(scene, n):
    shape = (n, n, n)
    if scene == "room":
        return synth.room_mask_torch(shape, "cpu").numpy()
    if scene == "solid_boxes":
        return synth.tutorial_boxes_mask_torch(shape, "cpu", True).numpy()
    if scene == "convex_scene":
        import scenes

        m, _ = scenes.convex_segments_scene()
        reps = [-(-n // s) for s in m.shape]
        return np.ascontiguousarray(np.tile(m, reps)[:n, :n, :n])
    return synth.bernoulli_mask(shape, 0.5, 3)


def cells_of(mask):
    c = np.zeros(mask.shape + (4,), np.uint32)
    c[..., 0] = np.where(mask != 0, np.float32(1.0), np.float32(0.0)).view(np.uint32)
    nx = mask.shape[0]
    obj = c[..., 2]
    obj[: nx // 3][mask[: nx // 3] != 0] = 1
    obj[nx // 3: 2 * nx // 3][mask[nx // 3: 2 * nx // 3] != 0] = 2
    return c


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


def gpu_case(ctx, scene, n, reps, warmup, host):
    shape = (n, n, n)
    res = 1.0
    mask = mask_of(scene, n)
    s = torch.cuda.current_stream().cuda_stream
    d_mask = torch.from_numpy(mask.astype(np.uint8)).cuda()
    d_sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
    sdf_ms, _ = _time(lambda: ctx.build_device(d_mask.data_ptr(), shape, d_sdf.data_ptr(), res, True, s), reps, warmup)
    bits = torch.from_numpy(capi.pack_bits_host(mask).view(np.int32)).cuda()
    labels = torch.empty(n * n * n, dtype=torch.int32, device="cuda")
    cc_ms, _ = _time(lambda: ctx.components_bits_device(bits.data_ptr(), shape, labels.data_ptr(), s), reps, warmup)
    if scene == "noise":
        d_sdf = torch.from_numpy(np.random.default_rng(1).random(shape, dtype=np.float32)).cuda()
    d_ext = torch.empty(shape, dtype=torch.int32, device="cuda")
    ext_ms, ext_min = _time(lambda: ctx.local_extrema_device(d_sdf.data_ptr(), shape, res, d_ext.data_ptr(), stream=s), reps, warmup)
    info = ctx.convex_last_info()
    row = {"case": "%s_%d" % (scene, n), "shape": list(shape), "extrema_ms": round(ext_ms, 4), "extrema_ms_min": round(ext_min, 4),
           "sdf_ms": round(sdf_ms, 4), "components_ms": round(cc_ms, 4), "reps": reps}
    row.update(info)
    row["extremum_off"] = int((d_ext == -1).sum().item())
    del d_mask, d_sdf, bits, labels, d_ext
    torch.cuda.empty_cache()
    if host:
        cells = cells_of(mask)
        ms, k = [], 0
        for i in range(1 + max(2, reps // 4)):
            work = cells.copy()
            t0 = time.perf_counter()
            k = ctx.convex_segments_cells(work, shape, res, 1.75 * res, True)
            t1 = time.perf_counter()
            if i >= 1:
                ms.append((t1 - t0) * 1e3)
        row.update({"host_ms": round(float(np.median(ms)), 2), "host_ms_min": round(float(np.min(ms)), 2), "segments": k,
                    "host_rounds": ctx.convex_last_info()["rounds"]})
    return row


def restated_case(scene, n):
    from test_convex_segments_cpu import restated_extrema, restated_segments
    from oracle import oracle as O

    mask = mask_of(scene, n)
    if scene == "noise":
        sdf = np.random.default_rng(1).random(mask.shape, dtype=np.float32)
    else:
        sdf, _ = O.reference_sdf(mask, 1.0, True)
    t0 = time.perf_counter()
    ext = restated_extrema(sdf, 1.0)
    t1 = time.perf_counter()
    cells = cells_of(mask)
    _, k = restated_segments(cells[..., 0].view(np.float32), cells[..., 2], ext, 1.75)
    t2 = time.perf_counter()
    return {"case": "%s_%d" % (scene, n), "shape": [n, n, n], "path": "restatement, one host core",
            "extrema_ms": round((t1 - t0) * 1e3, 1), "segments_ms": round((t2 - t1) * 1e3, 1), "segments": k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--only", default="")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--restated", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    only = [s for s in a.only.split(",") if s] or list(SCENES)
    out = open(a.out, "a") if a.out else None

    def emit(r):
        print(json.dumps(r), flush=True)
        if out:
            out.write(json.dumps(r) + "\n")
            out.flush()

    if a.restated:
        for scene in only:
            emit(restated_case(scene, a.restated))
        return
    ctx = capi.SdfGpu(0)
    for n in (int(v) for v in a.sizes.split(",")):
        for scene in only:
            emit(gpu_case(ctx, scene, n, a.reps, a.warmup, not a.no_host))
    ctx.close()


if __name__ == "__main__":
    main()
