"""GPU: the mesh rasteriser past 2^31 voxels.  1290 x 1290 x 1291 = 2 148 353 100 voxels, bits only (0.27 GB): three small meshes,
one of them on the last x plane, whose voxels have linear indices above 2^31.  Inside each mesh's index window the bits equal the
restatement (tests/mesh_raster_restated.py, evaluated at those indices alone); the popcount of the whole field, taken on the
device, equals the windows' total, so nothing is set anywhere else."""
import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_raster_restated as R
import resample_restated
from sdf_tools_amd import capi
from test_gpu_scene_large import GRID, RES, _popcount

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cached_device_memory():
    """what this module's torch buffers took from the device goes back when the module is done (a 0.27 GB field among them)"""
    yield
    torch.cuda.empty_cache()


def test_three_meshes_on_a_grid_past_2_31_voxels(gpu):
    n = GRID[0] * GRID[1] * GRID[2]
    assert n > 2 ** 31
    origin = np.eye(4)
    origin[:3, 3] = (0.3, -0.2, 0.1)
    ext = np.asarray(GRID) * RES

    def pose(q, at):
        return origin @ resample_restated.quaternion_origin(q, at)

    at = [np.array([9.1, 8.2, 10.4]) * RES, ext * np.array([0.5, 0.43, 0.61]),
          # on the last x planes: x >= 1289 has linear indices >= 1289 * 1290 * 1291 = 2 146 687 710, and 2^31 falls inside plane 1289
          np.array([ext[0] - 4.0 * RES, ext[1] * 0.9, ext[2] * 0.8])]
    items = [(5, *MC.icosahedron(7.3 * RES), pose((1.0, 0.0, 0.0, 0.0), at[0])),
             (6, *MC.box_triangles((9.0 * RES, 14.0 * RES, 6.0 * RES)), pose((0.71, 0.33, -0.52, 0.27), at[1])),
             # (a box whose x face lies inside the voxels of plane 1289)
             (7, *MC.box_triangles((7.0 * RES, 16.0 * RES, 14.0 * RES)), pose((1.0, 0.0, 0.0, 0.0), at[2]))]
    meshes, vertices, triangles = capi.make_meshes(items)
    words = (n + 31) // 32
    d_bits = torch.full((words,), -1, dtype=torch.int32, device="cuda")
    d = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() for a in (meshes, vertices, triangles)]
    bad = gpu.rasterize_meshes_device(d[0].data_ptr(), len(meshes), d[1].data_ptr(), len(vertices), d[2].data_ptr(), len(triangles), origin, RES, GRID,
                                      d_bits=d_bits.data_ptr(), check=True, stream=torch.cuda.current_stream().cuda_stream)
    assert bad == -1
    expected_total, beyond = 0, 0
    for centre in at:
        t = centre / RES                                                                   # the mesh's centre in voxels
        lo = np.maximum(np.floor(t - 20.0).astype(np.int64), 0)
        hi = np.minimum(np.ceil(t + 20.0).astype(np.int64), np.asarray(GRID) - 1)
        x, y, z = np.meshgrid(*[np.arange(a, b + 1, dtype=np.int64) for a, b in zip(lo, hi)], indexing="ij")
        linear = ((x * GRID[1] + y) * GRID[2] + z).reshape(-1)
        want, _ = R.hits_at_linear(meshes, vertices, triangles, origin, RES, GRID, linear)
        idx = torch.from_numpy(linear).cuda()
        got = ((d_bits[idx >> 5].to(torch.int64) >> (idx & 31)) & 1).cpu().numpy().astype(bool)
        assert np.array_equal(got, want), (centre, int((got != want).sum()), len(want))
        assert want.any()
        expected_total += int(want.sum())
        beyond += int((want & (linear >= 2 ** 31)).sum())
    assert beyond > 100, "no filled voxel past 2^31: the case shows nothing"
    assert _popcount(d_bits) == expected_total
