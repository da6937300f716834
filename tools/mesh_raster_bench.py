#!/usr/bin/env python3
"""Mesh rasteriser timings (sdfgpu_rasterize_meshes_device) and the plane's: one JSON line per scene, also appended to
profiles/mesh_raster_bench.jsonl with --out.  The protocol of tools/raster_bench.py: device-resident, 512^3 at resolution 0.01, bits
only, medians of `--reps` after `--warmup`, each between two events of the caller on one stream.  Scenes:
  room        the room of tools/raster_bench.py, every box as 12 triangles (9 x 12); beside it the same room as boxes through the
              shape rasteriser (shapes_ms)
  icosphere   81 920 triangles (an icosahedron subdivided six times), radius 0.35 of the grid
  heightfield 1024 x 1024 cells, 2 097 152 triangles, a wavy sheet through the volume
  sliver      one thin triangle across the grid's diagonal
  floor       two triangles over a whole z layer
  plane       one plane in a generic pose, through the shape rasteriser
Per line:
  raster_ms   the rasteriser call (memsets + five kernels; for the plane: the shape rasteriser's call)
  memset_ms   a memset of the 16 MiB bit field
  build_ms    sdfgpu_build_bits_device on the resulting bits
  filled      set bits of the result
The aims (no assertion): room raster_ms <= shapes_ms; icosphere raster_ms < build_ms.
usage: mesh_raster_bench.py [--n N] [--reps R] [--warmup W] [--only name,...] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import raster_bench  # noqa: E402
from sdf_tools_amd import capi  # noqa: E402

RES = raster_bench.RES
BOX_T = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)], np.uint32)


def room_meshes(n):
    items = []
    for rec in raster_bench.room_shapes(n):
        d = np.asarray(rec["dims"]) * 0.5
        v = np.array([((k & 1) * 2 - 1, ((k >> 1) & 1) * 2 - 1, ((k >> 2) & 1) * 2 - 1) for k in range(8)], np.float64) * d
        items.append((1, v, BOX_T, np.asarray(rec["pose"]).reshape(4, 4)))
    return capi.make_meshes(items)


def icosphere(levels):
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [np.array(p, np.float64) / np.sqrt(1.0 + g * g) for p in ((-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g),
                                                                   (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1))]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in t:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = out
    return np.array(v), np.array(t, np.uint32)


def icosphere_meshes(n):
    v, t = icosphere(6)
    pose = np.eye(4)
    pose[:3, 3] = np.array([0.5, 0.5, 0.5]) * n * RES + 0.0013
    return capi.make_meshes([(1, v * 0.35 * n * RES, t, pose)])


def heightfield_meshes(n, cells=1024):
    size = n * RES
    x, y = np.meshgrid(np.linspace(0.0, size, cells + 1), np.linspace(0.0, size, cells + 1), indexing="ij")
    z = (0.5 + 0.2 * np.sin(x * 3.0) * np.cos(y * 2.0)) * size
    v = np.stack([x, y, z], -1).reshape(-1, 3)
    i = (np.arange(cells)[:, None] * (cells + 1) + np.arange(cells)[None, :]).reshape(-1)
    t = np.concatenate([np.stack([i, i + cells + 1, i + cells + 2], 1), np.stack([i, i + cells + 2, i + 1], 1)]).astype(np.uint32)
    return capi.make_meshes([(1, v, t, np.eye(4))])


def sliver_meshes(n):
    size = n * RES
    v = np.array([(0.0, 0.0, 0.0), (size, size, size), (size + 0.3 * RES, size - 0.2 * RES, size)])
    return capi.make_meshes([(1, v, [(0, 1, 2)], np.eye(4))])


def floor_meshes(n):
    size, z = n * RES, (n // 3 + 0.37) * RES
    v = np.array([(0, 0, z), (size, 0, z), (size, size, z), (0, size, z)], np.float64)
    return capi.make_meshes([(1, v, [(0, 1, 2), (0, 2, 3)], np.eye(4))])


def generic_plane(n):
    q = np.array([0.71, 0.33, -0.52, 0.27])
    q /= np.linalg.norm(q)
    w, x, y, z = q
    pose = np.eye(4)
    pose[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    pose[:3, 3] = np.array([0.47, 0.553, 0.41]) * n * RES
    return capi.make_shapes([(capi.SHAPE_PLANE, 1, (0.3, -1.1, 0.7), pose)])


MESH_SCENES = {"room": room_meshes, "icosphere": icosphere_meshes, "heightfield": heightfield_meshes, "sliver": sliver_meshes, "floor": floor_meshes}


def _popcount(d_bits):
    v = d_bits.to(torch.int64) & 0xFFFFFFFF
    v = v - ((v >> 1) & 0x55555555)
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
    v = (v + (v >> 4)) & 0x0F0F0F0F
    return int((((v * 0x01010101) >> 24) & 0xFF).sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    n, shape = args.n, (args.n,) * 3
    ctx = capi.SdfGpu(0)
    stream = torch.cuda.current_stream().cuda_stream
    words = (n ** 3 + 31) // 32
    d_bits = torch.zeros(words, dtype=torch.int32, device="cuda")
    d_sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
    timed = raster_bench._timed
    lines = []

    def finish(row):
        row["filled"] = _popcount(d_bits)
        scratch = torch.empty_like(d_bits)
        row["memset_ms"] = timed(lambda: scratch.zero_(), args.reps, args.warmup)
        del scratch
        ctx.set_option("policy_reset", 1)
        row["build_ms"] = timed(lambda: ctx.build_bits_device(d_bits.data_ptr(), shape, d_sdf.data_ptr(), RES, False, stream), args.reps, args.warmup)
        row["path"] = str(ctx.last_path())
        lines.append(row)
        print(json.dumps(row), flush=True)

    for name, make in MESH_SCENES.items():
        if only and name not in only:
            continue
        meshes, vertices, triangles = make(n)
        d = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() for a in (meshes, vertices, triangles)]
        row = {"scene": name, "n": n, "meshes": int(len(meshes)), "triangles": int(len(triangles)), "bit_field_bytes": words * 4}

        def call(check=False):
            return ctx.rasterize_meshes_device(d[0].data_ptr(), len(meshes), d[1].data_ptr(), len(vertices), d[2].data_ptr(), len(triangles), np.eye(4), RES,
                                               shape, d_bits=d_bits.data_ptr(), check=check, stream=stream)
        if name == "room":                                                     # the same room as boxes, first: the bits that stay are the meshes'
            shapes = raster_bench.room_shapes(n)
            d_shapes = torch.from_numpy(shapes.view(np.uint8).reshape(-1).copy()).cuda()
            row["shapes_ms"] = timed(lambda: ctx.rasterize_shapes_device(d_shapes.data_ptr(), len(shapes), np.eye(4), RES, shape, d_bits=d_bits.data_ptr(),
                                                                         stream=stream), args.reps, args.warmup)
            row["shapes_filled"] = _popcount(d_bits)
        assert call(check=True) == -1
        row["raster_ms"] = timed(call, args.reps, args.warmup)
        finish(row)
    if not only or "plane" in only:
        shapes = generic_plane(n)
        d_shapes = torch.from_numpy(shapes.view(np.uint8).reshape(-1).copy()).cuda()
        row = {"scene": "plane", "n": n, "shapes": 1, "bit_field_bytes": words * 4}
        assert ctx.rasterize_shapes_device(d_shapes.data_ptr(), 1, np.eye(4), RES, shape, d_bits=d_bits.data_ptr(), check=True, stream=stream) == -1
        row["raster_ms"] = timed(lambda: ctx.rasterize_shapes_device(d_shapes.data_ptr(), 1, np.eye(4), RES, shape, d_bits=d_bits.data_ptr(), stream=stream),
                                 args.reps, args.warmup)
        finish(row)
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
