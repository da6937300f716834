#!/usr/bin/env python3
"""Solid mesh fill timings (sdfgpu_rasterize_solid_meshes_device): one JSON line per scene, also appended to
profiles/mesh_solid_bench.jsonl with --out.  The protocol of tools/mesh_raster_bench.py: device-resident, 512^3 at resolution 0.01,
bits only, medians of `--reps` after `--warmup`, each between two events of the caller on one stream.  Scenes, in one run:
  icosphere   81 920 triangles, one closed mesh: solid_ms against the surface call on the same mesh (surface_ms) and against
              sdfgpu_build_bits_device on the solid result (build_ms)
  room        the room of tools/raster_bench.py as nine closed 12-triangle meshes: solid_ms against the same room as nine box
              primitives through sdfgpu_rasterize_shapes_device (shapes_ms)
Per line also: filled (set bits of the solid result), surface_filled / shapes_filled, and whether the aim is met.
The aims (no assertion): icosphere solid_ms - surface_ms <= build_ms; room solid_ms <= shapes_ms.
usage: mesh_solid_bench.py [--n N] [--reps R] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mesh_raster_bench as MB  # noqa: E402
import raster_bench  # noqa: E402
from sdf_tools_amd import capi  # noqa: E402

RES = raster_bench.RES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n, shape = args.n, (args.n,) * 3
    ctx = capi.SdfGpu(0)
    stream = torch.cuda.current_stream().cuda_stream
    words = (n ** 3 + 31) // 32
    d_bits = torch.zeros(words, dtype=torch.int32, device="cuda")
    d_sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
    timed = raster_bench._timed
    lines = []
    for name, make in (("icosphere", MB.icosphere_meshes), ("room", MB.room_meshes)):
        meshes, vertices, triangles = make(n)
        assert capi.check_closed_meshes(meshes, vertices, triangles) is None
        d = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() for a in (meshes, vertices, triangles)]
        row = {"scene": name, "n": n, "meshes": int(len(meshes)), "triangles": int(len(triangles)), "bit_field_bytes": words * 4}

        def call(solid, check=False):
            f = ctx.rasterize_solid_meshes_device if solid else ctx.rasterize_meshes_device
            return f(d[0].data_ptr(), len(meshes), d[1].data_ptr(), len(vertices), d[2].data_ptr(), len(triangles), np.eye(4), RES, shape,
                     d_bits=d_bits.data_ptr(), check=check, stream=stream)
        if name == "room":
            shapes = raster_bench.room_shapes(n)
            d_shapes = torch.from_numpy(shapes.view(np.uint8).reshape(-1).copy()).cuda()
            row["shapes_ms"] = timed(lambda: ctx.rasterize_shapes_device(d_shapes.data_ptr(), len(shapes), np.eye(4), RES, shape, d_bits=d_bits.data_ptr(),
                                                                         stream=stream), args.reps, args.warmup)
            row["shapes_filled"] = MB._popcount(d_bits)
        assert call(False, check=True) == -1
        row["surface_ms"] = timed(lambda: call(False), args.reps, args.warmup)
        row["surface_filled"] = MB._popcount(d_bits)
        assert call(True, check=True) == -1
        row["solid_ms"] = timed(lambda: call(True), args.reps, args.warmup)
        row["filled"] = MB._popcount(d_bits)
        if name == "icosphere":
            ctx.set_option("policy_reset", 1)
            row["build_ms"] = timed(lambda: ctx.build_bits_device(d_bits.data_ptr(), shape, d_sdf.data_ptr(), RES, False, stream), args.reps, args.warmup)
            row["path"] = str(ctx.last_path())
            row["aim"] = "solid_ms - surface_ms <= build_ms"
            row["aim_met"] = bool(row["solid_ms"] - row["surface_ms"] <= row["build_ms"])
        else:
            row["aim"] = "solid_ms <= shapes_ms"
            row["aim_met"] = bool(row["solid_ms"] <= row["shapes_ms"])
        lines.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
