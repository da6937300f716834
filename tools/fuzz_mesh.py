#!/usr/bin/env python3
"""Differential fuzz of the mesh rasteriser and the plane: random meshes (random soups, icosahedra, long slivers, degenerate
triangles), poses, grids, origins and resolutions on ONE red-zoned handle, through the host form and the device form (with and
without accumulation onto a random field), every bit, byte and id against the numpy restatement (tests/mesh_raster_restated.py).
usage: fuzz_mesh.py [seconds] [seed]     prints "fuzz OK: N scenes ... 0 mismatches; ..." and exits 0, or the first mismatch and 1"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mesh_cases as MC  # noqa: E402
import mesh_raster_restated as R  # noqa: E402
import resample_restated  # noqa: E402
from sdf_tools_amd import capi  # noqa: E402


def scene(rng):
    grid = tuple(int(v) for v in rng.integers(1, 40, 3))
    res = float(rng.choice([0.05, 0.03, 0.125, 0.2, 0.0173]))
    origin = resample_restated.quaternion_origin(rng.normal(size=4), rng.uniform(-2.0, 2.0, 3)) if rng.random() < 0.7 else np.eye(4)
    ext = np.asarray(grid, np.float64) * res
    items = []
    for _ in range(int(rng.integers(0, 6))):
        kind = rng.integers(0, 5)
        if kind == 0:
            v, t = MC.icosahedron(float(rng.uniform(0.3, 6.0)) * res)
        elif kind == 1:
            v, t = MC.box_triangles(rng.uniform(0.2, 8.0, 3) * res)
        elif kind == 2:                                                        # a sliver through the grid
            a = rng.uniform(-0.6, 0.6, 3) * ext
            v, t = np.array([a, -a, -a + rng.normal(size=3) * 0.3 * res]), np.array([[0, 1, 2]])
        elif kind == 3:                                                        # degenerate: repeated indices
            v = rng.normal(size=(3, 3)) * 3.0 * res
            t = np.array([[0, 1, 1], [2, 2, 2], [0, 1, 2]])
        else:
            nv = int(rng.integers(3, 30))
            v = rng.normal(size=(nv, 3)) * rng.uniform(0.3, 5.0) * res
            t = rng.integers(0, nv, (int(rng.integers(0, 70)), 3))
        pose = origin @ MC._local(rng.normal(size=4), rng.uniform(-0.1, 1.1, 3) * ext)
        items.append((int(rng.integers(1, 12)), v, t, pose))
    return capi.make_meshes(items) + (origin, res, grid)


def upload(a):
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = torch.zeros(raw.size + 256, dtype=torch.uint8, device="cuda")
    if raw.size:
        d[:raw.size] = torch.from_numpy(raw.copy()).cuda()
    return d


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 30.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = np.random.default_rng(seed)
    ctx = capi.SdfGpu(0)
    ctx.set_option("redzone", 1)
    stream = torch.cuda.current_stream().cuda_stream
    t0, scenes, accumulated, planes, filled, triangles_seen = time.time(), 0, 0, 0, 0, 0
    while time.time() - t0 < seconds or scenes < 50:
        meshes, vertices, triangles, origin, res, grid = scene(rng)
        n = int(np.prod(grid))
        mask, ids, bits = R.restated(meshes, vertices, triangles, origin, res, grid)
        got = ctx.rasterize_meshes(meshes, vertices, triangles, origin, res, grid, bits=True, mask=True, object_ids=True)
        onto = None
        if rng.random() < 0.5:
            rmask = (rng.random(grid) < 0.2).astype(np.uint8)
            rids = np.where(rmask, rng.integers(1, 12, grid), 0).astype(np.uint32)
            onto = (rmask, rids)
            accumulated += 1
        wmask, wids, wbits = R.restated(meshes, vertices, triangles, origin, res, grid, onto=onto) if onto else (mask, ids, bits)
        d_in = [upload(a) for a in (meshes, vertices, triangles)]
        d_out = [upload(a) for a in ((R.pack_bits(onto[0]), onto[0], onto[1]) if onto else (np.zeros_like(bits), np.zeros_like(mask), np.zeros_like(ids)))]
        bad = ctx.rasterize_meshes_device(d_in[0].data_ptr(), len(meshes), d_in[1].data_ptr(), len(vertices), d_in[2].data_ptr(), len(triangles), origin,
                                          res, grid, d_out[0].data_ptr(), d_out[1].data_ptr(), d_out[2].data_ptr(), accumulate=onto is not None, check=True,
                                          stream=stream)
        torch.cuda.synchronize()
        dev = [d_out[0].cpu().numpy()[:bits.size * 4].view(np.uint32), d_out[1].cpu().numpy()[:n].reshape(grid),
               d_out[2].cpu().numpy()[:n * 4].view(np.uint32).reshape(grid)]
        pairs = [("host bits", got["bits"], bits), ("host mask", got["mask"], mask), ("host ids", got["object_ids"], ids),
                 ("device bits", dev[0], wbits), ("device mask", dev[1], wmask), ("device ids", dev[2], wids)]
        if rng.random() < 0.3:                                                 # a plane beside a box through the shape rasteriser
            shapes = capi.make_shapes([(capi.SHAPE_BOX, 2, rng.uniform(0.5, 5.0, 3) * res, origin @ MC._local(rng.normal(size=4), rng.uniform(0, 1, 3) * np.asarray(grid) * res)),
                                       (capi.SHAPE_PLANE, 1, rng.normal(size=3), origin @ MC._local(rng.normal(size=4), rng.uniform(-0.1, 1.1, 3) * np.asarray(grid) * res))])
            pm, pi, pb = R.restated_shapes(shapes, origin, res, grid)
            pg = ctx.rasterize_shapes(shapes, origin, res, grid, bits=True, mask=True, object_ids=True)
            pairs += [("plane bits", pg["bits"], pb), ("plane mask", pg["mask"], pm), ("plane ids", pg["object_ids"], pi)]
            planes += 1
        for what, a, b in pairs:
            if bad != -1 or not np.array_equal(a, b):
                print("MISMATCH in scene %d (seed %d): %s: %d cells differ; grid %s res %r, %d meshes, %d triangles, accumulate %s, bad %s"
                      % (scenes, seed, what, int((np.asarray(a) != np.asarray(b)).sum()), grid, res, len(meshes), len(triangles), onto is not None, bad))
                return 1
        ctx.redzone_check()
        scenes += 1
        filled += int(mask.sum())
        triangles_seen += len(triangles)
    ctx.close()
    print("fuzz OK: %d scenes in %.1f s, 0 mismatches; %d accumulated, %d with a plane; %d triangles, %d filled cells;"
          % (scenes, time.time() - t0, accumulated, planes, triangles_seen, filled))
    return 0


if __name__ == "__main__":
    sys.exit(main())
