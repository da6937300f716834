"""GPU: component surfaces on a grid just past 2^31 voxels (1290 x 1290 x 1291 = 2 148 353 100), the test that catches 32-bit
index arithmetic.  The labels are built on the device (no host copy): label 2 is a box whose last voxels lie beyond linear
index 2^31, label 3 the single voxel at the last index, label 1 the rest.  Expectation, in closed form: the six grid faces, the
box's own shell and the free voxels that share a face with the box.  Counts are compared with integer arithmetic, the indices
with the same closed form evaluated by torch on the device in x chunks."""
import math

import numpy as np
import pytest

from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

SHAPE = (1290, 1290, 1291)
BOX = (1280, 1290, 600, 700, 300, 400)                              # x0, x1, y0, y1, z0, z1, half open; x1 = nx: it reaches the x face


@pytest.fixture(scope="module")
def big():
    """A context of its own for the largest grid: its scratch goes when the module ends."""
    import torch
    ctx = capi.SdfGpu(0)
    yield ctx
    ctx.close()
    torch.cuda.empty_cache()


def _expected_counts():
    nx, ny, nz = SHAPE
    x0, x1, y0, y1, z0, z1 = BOX
    dx, dy, dz = x1 - x0, y1 - y0, z1 - z0
    faces = nx * ny * nz - (nx - 2) * (ny - 2) * (nz - 2)
    box = dx * dy * dz - (dx - 2) * (dy - 2) * (dz - 2)             # (the layer at x = nx - 1 is on the grid face: reported either way)
    # free voxels sharing a face with the box that are not on a grid face: the slab below x0, and the y and z slabs without
    # their x = nx - 1 row; the slab above x1 is outside the grid
    neighbours = dy * dz + 2 * (dx - 1) * dz + 2 * (dx - 1) * dy
    free = faces - dy * dz - 1 + neighbours                         # (faces hold the box's x = nx - 1 layer and the last voxel)
    return [0, free, box, 1]


def _reported_chunk(xa, xb, device):
    """bool [xb - xa, ny, nz]: the closed form of the reported voxels, from coordinates alone"""
    import torch
    nx, ny, nz = SHAPE
    x0, x1, y0, y1, z0, z1 = BOX
    X = torch.arange(xa, xb, device=device).view(-1, 1, 1)
    Y = torch.arange(ny, device=device).view(1, -1, 1)
    Z = torch.arange(nz, device=device).view(1, 1, -1)

    def rng(c, lo, hi):
        return (c >= lo) & (c < hi)
    face = (X == 0) | (X == nx - 1) | (Y == 0) | (Y == ny - 1) | (Z == 0) | (Z == nz - 1)
    bx, by, bz = rng(X, x0, x1), rng(Y, y0, y1), rng(Z, z0, z1)
    box = bx & by & bz
    inner = rng(X, x0 + 1, x1 - 1) & rng(Y, y0 + 1, y1 - 1) & rng(Z, z0 + 1, z1 - 1)
    near = (rng(X, x0 - 1, x1 + 1) & by & bz) | (bx & rng(Y, y0 - 1, y1 + 1) & bz) | (bx & by & rng(Z, z0 - 1, z1 + 1))
    return face | (near & ~inner), box


def test_three_labels_past_2_31_voxels(big):
    import torch
    nx, ny, nz = SHAPE
    n = math.prod(SHAPE)
    assert 2 ** 31 < n < 2 ** 32
    x0, x1, y0, y1, z0, z1 = BOX
    assert ((x1 - 1) * ny + (y1 - 1)) * nz + (z1 - 1) > 2 ** 31 > (x0 * ny + y0) * nz + z0       # the box straddles index 2^31
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.empty_cache()
    need = 4 * n + n // 8 + (3 << 30)                               # labels, the surface bits, chunks and the sort's buffers
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %.1f GB of free device memory, %.1f GB are free" % (need / 1e9, free / 1e9))
    labels = torch.ones(SHAPE, dtype=torch.int32, device=dev)
    labels[x0:x1, y0:y1, z0:z1] = 2
    labels[nx - 1, ny - 1, nz - 1] = 3
    want = _expected_counts()
    total = sum(want)

    counts, t = big.component_surfaces_device(labels.data_ptr(), SHAPE, 3, stream=stream, counts_only=True)
    print("\n[surfaces-large] counts", counts.tolist(), "want", want)
    assert counts.tolist() == want and t == total
    idx = torch.full((total + 16,), -1, dtype=torch.int32, device=dev)
    counts, t = big.component_surfaces_device(labels.data_ptr(), SHAPE, 3, d_indices=idx.data_ptr(), capacity=total, stream=stream)
    assert counts.tolist() == want and t == total
    assert bool((idx[total:] == -1).all()), "stored past the capacity"
    got = idx[:total].to(torch.int64) & 0xFFFFFFFF
    assert int(got[-1]) == n - 1 and int(got.max()) == n - 1       # the last voxel: an index past 2^31, kept as uint32

    pos = {1: 0, 2: want[1], 3: want[1] + want[2]}
    chunk = 30
    for xa in range(0, nx, chunk):
        xb = min(nx, xa + chunk)
        rep, _ = _reported_chunk(xa, xb, dev)
        lab = labels[xa:xb]
        for c in (1, 2, 3):
            e = (rep & (lab == c)).reshape(-1).nonzero().reshape(-1) + xa * ny * nz
            k = int(e.numel())
            if k == 0:
                continue
            g = got[pos[c]:pos[c] + k]
            if g.numel() != k or not bool(torch.equal(g, e)):
                bad = (g != e).nonzero()[:3].reshape(-1).tolist() if g.numel() == k else []
                raise AssertionError("label %d, x planes %d..%d: indices differ (group positions %s)" % (c, xa, xb, bad))
            pos[c] += k
    assert pos == {1: want[1], 2: want[1] + want[2], 3: total}
    del labels, idx, got
    torch.cuda.empty_cache()
