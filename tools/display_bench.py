#!/usr/bin/env python3
"""Display export (sdfgpu_display_*_device) timings: one JSON line per case, also appended to
profiles/display_bench.jsonl with --out.  Everything is device-resident: 8-byte cell records (occupancy from the scene's mask, the
component labels of sdfgpu_components_bits_device), the scene's SDF, and result buffers sized from a count-only call.  HIP events
bracket each call on the current stream (the select and colour-map calls synchronise it themselves); median of --reps after --warmup.
Per scene:
  select_filled        OCCUPANCY, FILLED, scan order, indices only             (ExportForDisplay with one visible colour)
  select_surfaces      OCCUPANCY, all classes, surface_only, grouped by class  (ExportSurfacesForSeparateDisplay)
  select_components    KEY_FIELD on the component, FILLED only, grouped        (ExportConnectedComponentsForDisplay of the filled cells)
  select_sdf           d <= 0                                                   (ExportForDisplayCollisionOnly)
  expand               points and table colours of select_surfaces' result
  sdf_colors           the colour map of the whole field                        (SignedDistanceField::ExportForDisplay)
Beside each: copy_ms, a device-to-device copy that moves the bytes the call must read and write at the least (its input once,
its results once: a copy of half their sum reads and writes that many), ratio_to_copy, and host_ms, the same result from numpy on
the host, timed once (not for the surface rule: the 26-neighbour test in numpy at 512^3 takes minutes).
usage: display_bench.py [--n N] [--reps R] [--warmup W] [--only name,...] [--no-host] [--out FILE]"""
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


def _host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def scene_rows(ctx, name, shape, mask_cpu, reps, warmup, host):
    n = int(np.prod(shape))
    s = torch.cuda.current_stream().cuda_stream
    bits = torch.from_numpy(capi.pack_bits_host(mask_cpu).view(np.int32)).cuda()
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.components_bits_device(bits.data_ptr(), shape, labels.data_ptr(), s)
    cells = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    cells[:, 0] = torch.from_numpy(mask_cpu.reshape(-1).astype(np.float32).view(np.int32)).cuda()
    cells[:, 1] = labels
    del bits
    labels_cpu = labels.cpu().numpy().view(np.uint32)
    del labels
    d_mask = torch.from_numpy(mask_cpu.reshape(-1)).cuda()
    sdf = torch.empty(n, dtype=torch.float32, device="cuda")
    ctx.build_device(d_mask.data_ptr(), shape, sdf.data_ptr(), 0.01, stream=s)
    torch.cuda.synchronize()
    del d_mask
    sdf_cpu = sdf.cpu().numpy()
    rows = []

    def row(case, med, mn, moved, elements, host_ms=None):
        copy = _copy_ms(moved, reps, warmup)
        rows.append({"case": name, "shape": list(shape), "call": case, "elements": int(elements), "ms_median": round(med, 4), "ms_min": round(mn, 4),
                     "reps": reps, "bytes_moved": int(moved), "copy_ms": round(copy, 4), "ratio_to_copy": round(med / copy, 2),
                     "host_ms": None if host_ms is None else round(host_ms, 1)})

    selects = [("select_filled", capi.DISPLAY_OCCUPANCY, dict(class_mask=1), False),
               ("select_surfaces", capi.DISPLAY_OCCUPANCY, dict(class_mask=7, surface_only=True), True),
               ("select_components", capi.DISPLAY_KEY_FIELD, dict(class_mask=1), True)]
    surf = None
    for case, rule, opts, grouped in selects:
        total, _ = ctx.display_select_cells_device(cells.data_ptr(), shape, rule, 8, 0, 4, stream=s, **opts)
        idx = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
        keys = torch.empty(max(total, 1), dtype=torch.int32, device="cuda") if grouped else None
        gcap = 8 if rule == capi.DISPLAY_OCCUPANCY else int(labels_cpu.max()) + 1
        gk = torch.empty(gcap, dtype=torch.int32, device="cuda") if grouped else None
        go = torch.empty(gcap + 1, dtype=torch.int32, device="cuda") if grouped else None

        def fn():
            return ctx.display_select_cells_device(cells.data_ptr(), shape, rule, 8, 0, 4, grouped=grouped, d_indices=idx.data_ptr(),
                                                   d_keys=keys.data_ptr() if grouped else None, capacity=total,
                                                   d_group_keys=gk.data_ptr() if grouped else None,
                                                   d_group_offsets=go.data_ptr() if grouped else None, group_capacity=gcap, stream=s, **opts)
        med, mn = _time(fn, reps, warmup)
        host_ms = None
        if host and case == "select_filled":
            host_ms = _host_ms(lambda: np.flatnonzero(mask_cpu.reshape(-1) > 0.5).astype(np.uint32))
        if host and case == "select_components":
            def host_fn():
                i = np.flatnonzero(mask_cpu.reshape(-1) > 0.5).astype(np.uint32)
                return i[np.argsort(labels_cpu[i], kind="stable")]
            host_ms = _host_ms(host_fn)
        row(case, med, mn, n * 8 + total * (8 if grouped else 4), total, host_ms)
        if case == "select_surfaces":
            surf = (idx, keys, total)
    idx, keys, total = surf
    pts = torch.empty(max(total, 1) * 3, dtype=torch.float64, device="cuda")
    col = torch.empty(max(total, 1) * 4, dtype=torch.float32, device="cuda")
    table = torch.rand(12, dtype=torch.float32, device="cuda")

    def expand():
        ctx.display_expand_device(idx.data_ptr(), total, shape, 0.01, d_points=pts.data_ptr(), d_colors=col.data_ptr(), d_keys=keys.data_ptr(),
                                  d_color_table=table.data_ptr(), table_entries=3, stream=s)
    med, mn = _time(expand, reps, warmup)
    host_ms = None
    if host:
        i_cpu, k_cpu, t_cpu = idx.cpu().numpy().view(np.uint32)[:total].astype(np.int64), keys.cpu().numpy()[:total], table.cpu().numpy().reshape(3, 4)

        def host_expand():
            xyz = np.stack([i_cpu // (shape[1] * shape[2]), (i_cpu // shape[2]) % shape[1], i_cpu % shape[2]], axis=1).astype(np.float64)
            return 0.01 * (xyz + 0.5), t_cpu[k_cpu]
        host_ms = _host_ms(host_expand)
    row("expand", med, mn, total * (8 + 24 + 16), total, host_ms)
    del pts, col, surf

    total = ctx.display_select_sdf_device(sdf.data_ptr(), shape, stream=s)
    idx = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
    med, mn = _time(lambda: ctx.display_select_sdf_device(sdf.data_ptr(), shape, idx.data_ptr(), total, stream=s), reps, warmup)
    row("select_sdf", med, mn, n * 4 + total * 4, total, _host_ms(lambda: np.flatnonzero(sdf_cpu <= 0).astype(np.uint32)) if host else None)
    del idx
    colors = torch.empty(n * 4, dtype=torch.float32, device="cuda")
    med, mn = _time(lambda: ctx.display_sdf_colors_device(sdf.data_ptr(), shape, 0.5, colors.data_ptr(), stream=s), reps, warmup)
    host_ms = None
    if host:
        def host_colors():
            d = sdf_cpu.astype(np.float64)
            out = np.zeros((n, 4), np.float32)
            pos, neg = sdf_cpu > 0, sdf_cpu < 0
            out[pos, 1] = np.abs(d[pos] / max(0.0, d.max())) * 0.8 + 0.2
            out[neg, 0] = np.abs(d[neg] / min(0.0, d.min())) * 0.8 + 0.2
            out[~(pos | neg), 2] = 1.0
            out[:, 3] = 0.5
            return out
        host_ms = _host_ms(host_colors)
    row("sdf_colors", med, mn, n * 4 * 2 + n * 16, n, host_ms)       # (the field is read twice: extrema, then colours)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    out = open(a.out, "a") if a.out else None
    ctx = capi.SdfGpu(0)
    dev = torch.device("cuda", 0)
    scenes = [                                                      # (tools/surfaces_bench.py)
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
        for r in scene_rows(ctx, name, shape, np.ascontiguousarray(mk(shape), np.uint8), a.reps, a.warmup, not a.no_host):
            print(json.dumps(r), flush=True)
            if out:
                out.write(json.dumps(r) + "\n")
                out.flush()
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
