#!/usr/bin/env python3
"""Differential fuzzing of Resample on a GPU box: random shapes of at most 48 cells per axis (singleton axes included), ratios new /
old resolution in [0.3, 6], random unit quaternions and translations as origins, random cell sizes, all three record sizes, random
payloads and fill records; sdfgpu_resample_cells (host form) and sdfgpu_resample_cells_device (exact-size device buffers from
sdfgpu_device_malloc, the source at a random 4-byte offset) on ONE red-zoned handle, every byte of every result and the count of
written cells against the restatement (tests/resample_restated.cpp).

  python tools/fuzz_resample.py [seconds] [seed]

The last line is "fuzz OK: <scenes> scenes ..."; a mismatch prints the scene and exits 1."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import resample_restated as R  # noqa: E402
from sdf_tools_amd import capi  # noqa: E402

RESULT_CAP = 1 << 21          # result cells per scene


def draw_scene(rng):
    shape = [int(rng.integers(1, 49)) for _ in range(3)]
    for a in range(3):
        if rng.random() < 0.1:
            shape[a] = 1
    ratio = float(np.exp(rng.uniform(np.log(0.3), np.log(6.0)))) if rng.random() < 0.7 else float(rng.choice([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 1.0 / 3.0]))
    while np.prod([np.ceil(s / ratio) for s in shape]) > RESULT_CAP:
        shape[int(np.argmax(shape))] //= 2
    shape = tuple(max(1, s) for s in shape)
    cell = float(rng.choice([0.05, 0.25, 1.0, 0.013, float(rng.uniform(0.01, 2.0))]))
    origin = R.quaternion_origin(rng.normal(size=4), rng.uniform(-3.0, 3.0, 3)) if rng.random() < 0.8 else np.eye(4)
    cb = int(rng.choice([4, 8, 16]))
    cells = rng.integers(0, 256, shape + (cb,), dtype=np.uint8)
    cells.view(np.uint32)[..., -1 if cb == 4 else 1] = np.arange(1, int(np.prod(shape)) + 1, dtype=np.uint32).reshape(shape)
    fill = rng.integers(0, 256, cb, dtype=np.uint8)
    return shape, cell, cell * ratio, origin, cb, cells, fill


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    rng = np.random.default_rng(seed)
    R.restated(R.payload((2, 2, 2), 4), 1.0, np.eye(4), 2.0, R.oob_record(4))          # (compiles the restatement before the clock starts)
    ctx = capi.SdfGpu(0)
    ctx.set_option("redzone", 1)
    counts = {"scenes": 0, "host": 0, "device": 0, 4: 0, 8: 0, 16: 0, "coarser": 0, "finer": 0}
    t0 = time.time()
    while time.time() - t0 < budget:
        shape, cell, new_res, origin, cb, cells, fill = draw_scene(rng)
        want = R.restated(cells, cell, origin, new_res, fill)
        what = "seed %d scene %d shape %s cell %r new_resolution %r %d-byte origin %s" % (
            seed, counts["scenes"], "x".join(map(str, shape)), cell, new_res, cb, origin.tolist())
        try:
            got, written = ctx.resample_cells(cells, shape, cell, origin, want.inverse, want.inv_cell, want.shape, fill, cb)
            forms = [("host", got, written)]
            offset = 4 * int(rng.integers(0, 4))
            d_src, d_dst = ctx.device_malloc(cells.nbytes + offset), ctx.device_malloc(want.cells.nbytes)
            try:
                staged = np.zeros(cells.nbytes + offset, np.uint8)
                staged[offset:] = cells.reshape(-1)
                ctx.copy_from_host(d_src, staged)
                written = ctx.resample_cells_device(d_src + offset, shape, cell, origin, want.inverse, want.inv_cell, d_dst, want.shape, fill, cb,
                                                    count=True)
                got = ctx.copy_to_host(np.empty(want.cells.shape, np.uint8), d_dst)
                forms.append(("device", got, written))
            finally:
                ctx.device_free(d_src)
                ctx.device_free(d_dst)
        except capi.SdfGpuError as e:
            print("MISMATCH %s: %s" % (what, e), flush=True)
            sys.exit(1)
        for form, got, written in forms:
            if not np.array_equal(got, want.cells) or written != want.written:
                bad = np.argwhere((got != want.cells).any(axis=-1))
                print("MISMATCH %s: %s form: %d result cells differ (first %s), written %d against %d" % (
                    what, form, len(bad), bad[0].tolist() if len(bad) else None, written, want.written), flush=True)
                sys.exit(1)
            counts[form] += 1
        counts["scenes"] += 1
        counts[cb] += 1
        counts["coarser" if new_res > cell else "finer"] += 1
    ctx.redzone_check()
    ctx.close()
    print("fuzz OK: %d scenes in %.0f s (seed %d), red zones on, 0 mismatches; host %d, device %d; record sizes %s; coarser %d, finer or equal %d" % (
        counts["scenes"], time.time() - t0, seed, counts["host"], counts["device"], {k: counts[k] for k in (4, 8, 16)}, counts["coarser"],
        counts["finer"]))


if __name__ == "__main__":
    main()
