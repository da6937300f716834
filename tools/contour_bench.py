#!/usr/bin/env python3
"""Contour select (sdfgpu_display_select_contour_device) timings: one JSON line per case, also appended to
profiles/contour_bench.jsonl with --out.  Device-resident 16-byte tagged records (occupancy at 0, object id at 8) at --n^3:
  solid_boxes    the tutorial's boxes, filled cells tagged with their connected component (distinct ids), free cells id 0
  room           the room scene, tagged the same way
  bernoulli_0.5  i.i.d. filled cells, ids drawn from a pool of 16
Per scene, HIP events around each call on the current stream (every call synchronises it), median of --reps after --warmup:
  contour_count / contour_scan / contour_grouped   reach 3: the total only (k_dp_contour and the status read-back), indices in scan
                                                    order, indices and keys grouped by id
  surface_count / surface_scan                      the yardstick on the SAME records: display_select_cells_device(OCCUPANCY, FILLED,
                                                    surface_only), the 26-neighbour rule of k_dp_select
Beside each: copy_ms, a device-to-device copy that moves the bytes the call must read and write at the least (the records once, the
results once), ratio_to_copy, and for the contour rows ratio_to_surface = contour ms / surface ms of the same result form.
composed_128: at 128^3 with 16 objects, host forms -- build_tagged_objects plus the reference's literal threshold in numpy against
display_select_contour, wall clock, the results compared.
usage: contour_bench.py [--n N] [--reps R] [--warmup W] [--only name,...] [--out FILE]"""
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


def _copy_ms(nbytes, reps, warmup):
    half = max(int(nbytes) // 2, 4)
    a = torch.empty(half, dtype=torch.uint8, device="cuda")
    b = torch.empty(half, dtype=torch.uint8, device="cuda")
    return _time(lambda: b.copy_(a), reps, warmup)[0]


def tagged_records(ctx, shape, mask_cpu, ids=None):
    """int32 [n, 4] on the device: occupancy bits, 0, object id, 0.  ids=None: the connected component of the filled cells"""
    n = int(np.prod(shape))
    s = torch.cuda.current_stream().cuda_stream
    cells = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    filled = torch.from_numpy(mask_cpu.reshape(-1) != 0).cuda()
    cells[:, 0] = torch.where(filled, 0x3F800000, 0).to(torch.int32)
    if ids is None:
        bits = torch.from_numpy(capi.pack_bits_host(mask_cpu).view(np.int32)).cuda()
        labels = torch.empty(n, dtype=torch.int32, device="cuda")
        ctx.components_bits_device(bits.data_ptr(), shape, labels.data_ptr(), s)
        torch.cuda.synchronize()
        cells[:, 2] = torch.where(filled, labels + 1, 0)
    else:
        cells[:, 2] = torch.from_numpy(np.ascontiguousarray(ids, np.uint32).reshape(-1).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return cells


def scene_rows(ctx, name, shape, cells, reps, warmup):
    n = int(np.prod(shape))
    s = torch.cuda.current_stream().cuda_stream
    objects = int(torch.unique(cells[:, 2]).numel())
    rows = []

    def contour(**kw):
        return ctx.display_select_contour_device(cells.data_ptr(), shape, 3, 16, 0, 8, stream=s, **kw)

    def surface(**kw):
        return ctx.display_select_cells_device(cells.data_ptr(), shape, capi.DISPLAY_OCCUPANCY, 16, 0, 8, class_mask=1, surface_only=True, stream=s, **kw)

    totals = {"contour": contour()[0], "surface": surface()[0]}
    idx = torch.empty(max(max(totals.values()), 1), dtype=torch.int32, device="cuda")
    keys = torch.empty_like(idx)
    gk = torch.empty(objects + 1, dtype=torch.int32, device="cuda")
    go = torch.empty(objects + 2, dtype=torch.int32, device="cuda")
    calls = [("surface_count", "surface", surface, 0), ("contour_count", "contour", contour, 0),
             ("surface_scan", "surface", lambda: surface(d_indices=idx.data_ptr(), capacity=totals["surface"]), 4),
             ("contour_scan", "contour", lambda: contour(d_indices=idx.data_ptr(), capacity=totals["contour"]), 4),
             ("contour_grouped", "contour", lambda: contour(grouped=True, d_indices=idx.data_ptr(), d_keys=keys.data_ptr(), capacity=totals["contour"],
                                                            d_group_keys=gk.data_ptr(), d_group_offsets=go.data_ptr(), group_capacity=objects + 1), 8)]
    timed = {}
    for case, kind, fn, per_element in calls:
        med, mn = _time(fn, reps, warmup)
        timed[case] = med
        moved = n * 16 + totals[kind] * per_element
        copy = _copy_ms(moved, reps, warmup)
        r = {"case": name, "shape": list(shape), "call": case, "objects": objects, "elements": int(totals[kind]), "ms_median": round(med, 4),
             "ms_min": round(mn, 4), "reps": reps, "bytes_moved": int(moved), "copy_ms": round(copy, 4), "ratio_to_copy": round(med / copy, 2)}
        yard = {"contour_count": "surface_count", "contour_scan": "surface_scan"}.get(case)
        if yard:
            r["ratio_to_surface"] = round(med / timed[yard], 3)
        rows.append(r)
    return rows


def composed_row(ctx, reps):
    """128^3, 16 solid boxes with ids 1 .. 16: the reference's route through per-object SDFs against the contour select, host forms"""
    shape, res = (128, 128, 128), 0.05
    ids = np.zeros(shape, np.uint32)
    for b in range(16):
        x, y = 32 * (b // 4), 32 * (b % 4)
        ids[x + 4:x + 28, y + 4:y + 28, 16:112] = b + 1
    rec = np.zeros(shape + (4,), np.uint32)
    rec[..., 0] = (ids != 0).astype(np.float32).view(np.uint32)
    rec[..., 2] = ids
    reach = capi.display_contour_reach(res)

    def composed():
        fields, _ = ctx.build_tagged_objects(rec, shape, list(range(1, 17)), unknown_is_filled=True, resolution=res, add_virtual_border=False)
        bdy = np.float32(-1.9 * res)
        drawn = np.zeros(shape, bool)
        for o, d in zip(range(1, 17), fields):
            drawn |= (ids == o) & (d < 0.0) & (d > bdy)
        return np.flatnonzero(drawn.reshape(-1)).astype(np.uint32)

    def direct():
        return ctx.display_select_contour(rec, shape, reach)[0]

    want, got = composed(), direct()
    assert np.array_equal(want, got)
    out = {}
    for name, fn in (("composed", composed), ("contour", direct)):
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = float(np.median(ms))
    return {"case": "composed_128", "shape": list(shape), "call": "host forms, wall clock", "objects": 16, "elements": int(len(got)), "reps": reps,
            "composed_ms_median": round(out["composed"], 2), "contour_ms_median": round(out["contour"], 2),
            "speedup": round(out["composed"] / out["contour"], 1)}


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
    shape = (a.n,) * 3

    def emit(r):
        print(json.dumps(r), flush=True)
        if out:
            out.write(json.dumps(r) + "\n")
            out.flush()

    scenes = [("solid_boxes", lambda: (synth.tutorial_boxes_mask_torch(shape, dev, True).cpu().numpy(), None)),
              ("room", lambda: (synth.room_mask_torch(shape, dev).cpu().numpy(), None)),
              ("bernoulli_0.5", lambda: (synth.bernoulli_mask(shape, 0.5, 1), np.random.default_rng(2).integers(1, 17, size=shape, dtype=np.uint32)))]
    for scene, mk in scenes:
        name = "%s_%d" % (scene, a.n)
        if only and name not in only:
            continue
        mask, ids = mk()
        cells = tagged_records(ctx, shape, np.ascontiguousarray(mask, np.uint8), ids)
        for r in scene_rows(ctx, name, shape, cells, a.reps, a.warmup):
            emit(r)
        del cells
        torch.cuda.empty_cache()
    if not only or "composed_128" in only:
        emit(composed_row(ctx, a.reps))
    ctx.close()


if __name__ == "__main__":
    main()
