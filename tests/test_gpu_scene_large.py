"""GPU: the shape rasteriser past 2^31 voxels.  1290 x 1290 x 1291 = 2 148 353 100 voxels, bits only (0.27 GB): three shapes, one
of them on the last x plane, whose voxels have linear indices above 2^31.  Inside each shape's index window the bits equal the
restatement (tests/scene_raster_restated.py, evaluated at those indices alone); the popcount of the whole field, taken on the
device, equals the windows' total, so nothing is set anywhere else."""
import numpy as np
import pytest
import torch

import resample_restated
import scene_raster_restated as R
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

GRID = (1290, 1290, 1291)
RES = 0.01


def _popcount(words):
    """total set bits of an int32 tensor, in chunks (torch has no popcount: the usual three folding steps)"""
    total = 0
    for chunk in words.split(1 << 24):
        v = chunk.to(torch.int64) & 0xFFFFFFFF
        v = v - ((v >> 1) & 0x55555555)
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
        v = (v + (v >> 4)) & 0x0F0F0F0F
        total += int(((v * 0x01010101) >> 24 & 0xFF).sum().item())
    return total


def test_three_shapes_on_a_grid_past_2_31_voxels(gpu):
    n = GRID[0] * GRID[1] * GRID[2]
    assert n > 2 ** 31
    origin = np.eye(4)
    origin[:3, 3] = (0.3, -0.2, 0.1)
    ext = np.asarray(GRID) * RES

    def pose(q, at):
        return origin @ resample_restated.quaternion_origin(q, at)

    items = [(capi.SHAPE_SPHERE, 5, (7.3 * RES,), pose((1.0, 0.0, 0.0, 0.0), (9.1 * RES, 8.2 * RES, 10.4 * RES))),
             (capi.SHAPE_BOX, 6, (9.0 * RES, 14.0 * RES, 6.0 * RES), pose((0.71, 0.33, -0.52, 0.27), ext * np.array([0.5, 0.43, 0.61]))),
             # on the last x planes: x >= 1289 has linear indices >= 1289 * 1290 * 1291 = 2 146 687 710, and 2^31 falls inside plane 1289
             (capi.SHAPE_CYLINDER, 7, (40.0 * RES, 5.5 * RES), pose((0.8, 0.1, 0.55, -0.2), (ext[0] - 3.0 * RES, ext[1] * 0.9, ext[2] * 0.8)))]
    shapes = capi.make_shapes(items)
    words = (n + 31) // 32
    d_bits = torch.full((words,), -1, dtype=torch.int32, device="cuda")
    raw = torch.from_numpy(shapes.view(np.uint8).reshape(-1).copy()).cuda()
    bad = gpu.rasterize_shapes_device(raw.data_ptr(), len(shapes), origin, RES, GRID, d_bits=d_bits.data_ptr(), check=True,
                                      stream=torch.cuda.current_stream().cuda_stream)
    assert bad == -1
    expected_total, beyond = 0, 0
    for rec in shapes:
        t = (np.asarray(rec["pose"]).reshape(4, 4)[:3, 3] - origin[:3, 3]) / RES          # the shape's centre in voxels
        reach = float(np.abs(rec["dims"]).sum()) / RES + 3.0
        lo = np.maximum(np.floor(t - reach).astype(np.int64), 0)
        hi = np.minimum(np.ceil(t + reach).astype(np.int64), np.asarray(GRID) - 1)
        x, y, z = np.meshgrid(*[np.arange(a, b + 1, dtype=np.int64) for a, b in zip(lo, hi)], indexing="ij")
        linear = ((x * GRID[1] + y) * GRID[2] + z).reshape(-1)
        want, _ = R.hits_at(shapes, R.centres_of(origin, RES, GRID, linear), RES)
        idx = torch.from_numpy(linear).cuda()
        got = ((d_bits[idx >> 5].to(torch.int64) >> (idx & 31)) & 1).cpu().numpy().astype(bool)
        assert np.array_equal(got, want), ("object %d" % rec["object_id"], int((got != want).sum()), len(want))
        assert want.any()
        expected_total += int(want.sum())
        beyond += int((want & (linear >= 2 ** 31)).sum())
    assert beyond > 100, "no filled voxel past 2^31: the case shows nothing"
    assert _popcount(d_bits) == expected_total
