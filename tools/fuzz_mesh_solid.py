#!/usr/bin/env python3
"""Differential fuzz of the solid mesh fill: random closed meshes (tests/mesh_solid_cases.random_closed_meshes: randomly posed
icosahedra, tori and boxes, randomly subdivided, with random flips, some as soups), grids, origins and resolutions on ONE red-zoned
handle, through the device form with and without accumulation onto a random field, and through the host form, every bit, byte and
id against the numpy restatement (tests/mesh_solid_restated.py).  run(generator=...) takes the scenes from the caller instead
(tests/test_gpu_fuzz_mesh_solid.py: mesh_solid_cases.random_tall_scene).
usage: fuzz_mesh_solid.py [seconds] [seed]     prints "fuzz OK: N scenes ..." and exits 0, or raises at the first mismatch"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mesh_raster_restated as R  # noqa: E402
import mesh_solid_cases as SC  # noqa: E402
import mesh_solid_restated as S  # noqa: E402
import resample_restated  # noqa: E402
from sdf_tools_amd import capi  # noqa: E402


def scene(rng):
    grid = tuple(int(v) for v in rng.integers(1, 28, 3))
    if rng.random() < 0.15:
        grid = grid[:2] + (int(rng.integers(60, 140)),)
    res = float(rng.choice([0.05, 0.03, 0.125, 0.2, 0.0173]))
    origin = resample_restated.quaternion_origin(rng.normal(size=4), rng.uniform(-2.0, 2.0, 3)) if rng.random() < 0.7 else np.eye(4)
    return capi.make_meshes(SC.random_closed_meshes(rng, origin, res, grid, most=5)) + (origin, res, grid)


def upload(a):
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = torch.zeros(raw.size + 256, dtype=torch.uint8, device="cuda")
    if raw.size:
        d[:raw.size] = torch.from_numpy(raw.copy()).cuda()
    return d


def run(seconds, seed, least=50, generator=None):
    """(scenes, filled cells, cells filled by parity alone); raises AssertionError at the first mismatch.  generator: an iterable of
    scenes (mesh_solid_cases tuples) to run through instead of `seconds` of scene(rng); seed then only draws the fields accumulated onto"""
    rng = np.random.default_rng(seed)
    ctx = capi.SdfGpu(0)
    ctx.set_option("redzone", 1)
    stream = torch.cuda.current_stream().cuda_stream
    t0, scenes, filled, inside = time.time(), 0, 0, 0
    given = iter(generator) if generator is not None else None
    try:
        while given is not None or time.time() - t0 < seconds or scenes < least:
            if given is not None:
                try:
                    meshes, vertices, triangles, origin, res, grid = next(given)
                except StopIteration:
                    break
            else:
                meshes, vertices, triangles, origin, res, grid = scene(rng)
            n = int(np.prod(grid))
            onto = None
            if rng.random() < 0.5:
                rmask = (rng.random(grid) < 0.2).astype(np.uint8)
                onto = (rmask, np.where(rmask, rng.integers(1, 12, grid), 0).astype(np.uint32))
            mask, ids, bits = S.restated(meshes, vertices, triangles, origin, res, grid, onto=onto)
            d_in = [upload(a) for a in (meshes, vertices, triangles)]
            d_out = [upload(a) for a in ((R.pack_bits(onto[0]), onto[0], onto[1]) if onto else (np.zeros_like(bits), np.zeros_like(mask), np.zeros_like(ids)))]
            bad = ctx.rasterize_solid_meshes_device(d_in[0].data_ptr(), len(meshes), d_in[1].data_ptr(), len(vertices), d_in[2].data_ptr(), len(triangles),
                                                    origin, res, grid, d_out[0].data_ptr(), d_out[1].data_ptr(), d_out[2].data_ptr(),
                                                    accumulate=onto is not None, check=True, stream=stream)
            torch.cuda.synchronize()
            pairs = [("device bits", d_out[0].cpu().numpy()[:bits.size * 4].view(np.uint32), bits), ("device mask", d_out[1].cpu().numpy()[:n].reshape(grid), mask),
                     ("device ids", d_out[2].cpu().numpy()[:n * 4].view(np.uint32).reshape(grid), ids)]
            if onto is None and scenes % 4 == 0:
                got = ctx.rasterize_solid_meshes(meshes, vertices, triangles, origin, res, grid, bits=True, mask=True, object_ids=True)
                pairs += [("host bits", got["bits"], bits), ("host mask", got["mask"], mask), ("host ids", got["object_ids"], ids)]
            for what, a, b in pairs:
                assert bad == -1 and np.array_equal(a, b), "MISMATCH in scene %d (seed %d): %s: %d cells differ; grid %s res %r, %d meshes, %d triangles, accumulate %s, bad %s" % (
                    scenes, seed, what, int((np.asarray(a) != np.asarray(b)).sum()), grid, res, len(meshes), len(triangles), onto is not None, bad)
            ctx.redzone_check()
            scenes += 1
            filled += int(mask.sum())
            if onto is None:
                inside += int(mask.sum()) - int(R.restated(meshes, vertices, triangles, origin, res, grid)[0].sum())
    finally:
        ctx.close()
    return scenes, filled, inside


if __name__ == "__main__":
    result = run(float(sys.argv[1]) if len(sys.argv) > 1 else 30.0, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    print("fuzz OK: %d scenes, 0 mismatches; %d filled cells, %d by parity alone" % result)
