"""GPU: the solid fill of closed meshes past 2^31 voxels.  1290 x 1290 x 1291 = 2 148 353 100 voxels, bits (0.27 GB) and mask (2.1 GB) in
one call; the ids are left out (8.6 GB: the id loop of the merge is the surface pass's, tested past 2^31 in its own right, and its
index v is the mask's).  The toggle field of this grid is another 0.27 GB of the handle's.  Three solid meshes: an icosahedron near the
grid's origin corner, a box in a generic pose mid-grid, and a grid-aligned box that pokes out of the +x face, so that plane 1289 --
where the linear index passes 2^31 -- holds cells that are inside by parity and met by no probe.

Around each mesh, over the WHOLE columns of a +-20 voxel window in x and y, bits and mask equal the restatement: the surface
(mesh_raster_restated.hits_at_linear inside the window) ORed with the parity (mesh_solid_restated.inside_at_columns, full z).  The
popcount of the whole bit field and the sum of the whole mask, taken on the device, equal the windows' total: nothing is set anywhere
else.  Then a small grid on the same handle equals a fresh handle's result: the large toggle field was left all zero."""
import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_raster_restated as R
import mesh_solid_cases as SC
import mesh_solid_restated as S
import resample_restated
from sdf_tools_amd import capi
from test_gpu_mesh_solid import _device, _equal
from test_gpu_scene_large import GRID, RES, _popcount

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cached_device_memory():
    """what this module's torch buffers took from the device goes back when the module is done (2.4 GB of outputs among them)"""
    yield
    torch.cuda.empty_cache()


def test_three_solid_meshes_on_a_grid_past_2_31_voxels(gpu):
    n = GRID[0] * GRID[1] * GRID[2]
    assert n > 2 ** 31
    origin = np.eye(4)
    origin[:3, 3] = (0.3, -0.2, 0.1)
    ext = np.asarray(GRID) * RES

    def pose(q, at):
        return origin @ resample_restated.quaternion_origin(q, at)

    # x >= 1289 has linear indices >= 1289 * 1290 * 1291 = 2 146 687 710, and 2^31 falls inside plane 1289 at y = 616
    at = [np.array([9.1, 8.2, 10.4]) * RES, ext * np.array([0.5, 0.43, 0.61]), np.array([ext[0] - 1.6 * RES, ext[1] * 0.9, ext[2] * 0.8])]
    items = [(5, *MC.icosahedron(7.3 * RES), pose((0.71, 0.33, -0.52, 0.27), at[0])),
             (6, *MC.box_triangles((9.0 * RES, 14.0 * RES, 6.0 * RES)), pose((0.71, 0.33, -0.52, 0.27), at[1])),
             (7, *MC.box_triangles((9.6 * RES, 16.0 * RES, 14.0 * RES)), pose((1.0, 0.0, 0.0, 0.0), at[2]))]      # x from 1283.6 out of the grid
    meshes, vertices, triangles = capi.make_meshes(items)
    d_bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device="cuda")
    d_mask = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    d = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() for a in (meshes, vertices, triangles)]
    bad = gpu.rasterize_solid_meshes_device(d[0].data_ptr(), len(meshes), d[1].data_ptr(), len(vertices), d[2].data_ptr(), len(triangles), origin, RES, GRID,
                                            d_bits.data_ptr(), d_mask.data_ptr(), 0, check=True, stream=torch.cuda.current_stream().cuda_stream)
    assert bad == -1
    expected_total = parity_only_beyond = 0
    for m, centre in zip(meshes, at):
        t = centre / RES                                                                   # the mesh's centre in voxels
        lo = np.maximum(np.floor(t - 20.0).astype(np.int64), 0)
        hi = np.minimum(np.ceil(t + 20.0).astype(np.int64), np.asarray(GRID) - 1)
        xs, ys = (np.arange(a, b + 1, dtype=np.int64) for a, b in zip(lo[:2], hi[:2]))
        x, y, z = np.meshgrid(xs, ys, np.arange(GRID[2], dtype=np.int64), indexing="ij")
        linear = (x * GRID[1] + y) * GRID[2] + z                                           # the windows' whole columns
        window = (slice(None), slice(None), slice(int(lo[2]), int(hi[2]) + 1))
        hits = np.zeros(linear.shape, bool)
        hits[window] = R.hits_at_linear(meshes, vertices, triangles, origin, RES, GRID, linear[window].reshape(-1))[0].reshape(linear[window].shape)
        inside = S.inside_at_columns(R.world_triangles([m], vertices, triangles)[1], origin, RES, GRID, xs, ys)
        assert hits.any() and inside.any()
        outside = inside.copy()
        outside[window] = False
        assert not outside.any(), "the parity leaves the window's z range: the window is too small"
        want = hits | inside
        idx = torch.from_numpy(linear.reshape(-1)).cuda()
        got_bits = ((d_bits[idx >> 5].to(torch.int64) >> (idx & 31)) & 1).cpu().numpy().astype(bool).reshape(want.shape)
        got_mask = d_mask[idx].cpu().numpy().reshape(want.shape)
        _equal("bits about %s" % (t,), got_bits, want)
        _equal("mask about %s" % (t,), got_mask, want.astype(np.uint8))
        expected_total += int(want.sum())
        parity_only_beyond += int((inside & ~hits & (linear >= 2 ** 31)).sum())
    print("%d filled, %d of them past 2^31 by parity alone" % (expected_total, parity_only_beyond))
    assert parity_only_beyond >= 100, "no cell past 2^31 that only the parity fills: the case shows nothing"
    assert _popcount(d_bits) == expected_total
    assert sum(int(chunk.sum(dtype=torch.int64).item()) for chunk in d_mask.split(1 << 28)) == expected_total and int(d_mask.max().item()) == 1
    del d_bits, d_mask
    # a small grid on the same handle: what the large call left in its toggle field would show here
    scene = SC.stack_scene((12, 6, 96))
    ctx = capi.SdfGpu(0)
    try:
        fresh = _device(ctx, *scene)
    finally:
        ctx.close()
    got = _device(gpu, *scene)
    for k, what in enumerate(("bits", "mask", "ids")):
        _equal("the small grid afterwards: " + what, got[k], fresh[k])
    _equal("the small grid afterwards against the restatement", got[0], S.restated(*scene)[2])
