"""Batches of same-shape grids (include/sdfgpu.h "Batches of same-shape grids"): sdfgpu_build_batch*, sdfgpu_build_tagged_objects,
sdfgpu_gradient_batch_device and utils_3d.compute_sdf_and_gradient_batch.

The yardstick is oracle.exact_sdf (the restatement that does not depend on the code under test), every voxel of every grid
compared as uint32; the single build is the second comparison.  All scenes are seeded."""
import numpy as np
import pytest

from oracle import oracle as O
from sdf_tools_amd import capi, synth

pytestmark = pytest.mark.gpu

RES = (1.0, 0.05, 0.01, 0.25)
INF = float("inf")

# (shape, batch sizes, fast path expected)
SHAPES = [
    ((64, 64, 64), (1, 2, 7, 32), True),
    ((40, 40, 40), (1, 2, 7, 32), True),
    ((100, 100, 50), (1, 2, 7, 32), True),
    ((25, 20, 15), (1, 2, 7, 32), True),
    ((20, 40, 1), (1, 2, 7, 32), True),
    ((1, 33, 70), (1, 2, 7, 32), True),
    ((128, 128, 128), (2,), True),
    ((37, 5, 129), (1, 2, 7, 32), False),
]


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _scene(shape, b, seed):
    """Grid b of a batch: Bernoulli noise whose density walks through dense, mid and far-field scenes."""
    p = (0.5, 0.05, 0.002, 0.9, 0.2)[b % 5]
    return synth.bernoulli_mask(shape, p, seed * 1000 + b)


def _check_batch(gpu, masks, res, vb, fast, single=True):
    got, ext = gpu.build_batch(masks, res, vb)
    assert gpu.last_batch_info()[0] == fast
    assert got.shape == masks.shape and got.dtype == np.float32 and len(ext) == masks.shape[0]
    for b in range(masks.shape[0]):
        r = float(res[b]) if np.ndim(res) else float(res)
        want, want_ext, _ = O.exact_sdf(masks[b], r, vb)
        assert _bits_equal(got[b], want), ("oracle", masks.shape, b, vb, int((got[b].view(np.uint32) != want.view(np.uint32)).sum()))
        assert ext[b] == tuple(float(v) for v in want_ext), ("extrema", masks.shape, b, vb, ext[b], want_ext)
        if single:
            one, one_ext = gpu.build(masks[b], r, vb)
            assert _bits_equal(got[b], one) and ext[b] == one_ext, ("single build", masks.shape, b, vb)
    return got, ext


@pytest.mark.parametrize("shape,batches,fast", SHAPES, ids=["x".join(map(str, s[0])) for s in SHAPES])
def test_batch_equals_oracle_and_single_build(gpu, shape, batches, fast):
    for B in batches:
        masks = np.stack([_scene(shape, b, B) for b in range(B)])
        res = np.array([RES[(b + B) % 4] for b in range(B)])
        for vb in (False, True):
            _check_batch(gpu, masks, res, vb, fast)
    # one resolution for the whole batch (resolutions == NULL)
    masks = np.stack([_scene(shape, b, 99) for b in range(2)])
    _check_batch(gpu, masks, 0.05, False, fast)
    info = gpu.last_batch_info()
    assert info == ((True, 2) if fast else (False, -1))


def _isolation_batch(shape, order):
    nx = shape[0]
    g = [np.zeros(shape, np.uint8), np.ones(shape, np.uint8), np.zeros(shape, np.uint8), np.zeros(shape, np.uint8),
         synth.bernoulli_mask(shape, 0.5, 4), synth.bernoulli_mask(shape, 0.001, 5)]
    g[2][0, shape[1] // 2, shape[2] // 3] = 1
    g[3][nx - 1, shape[1] // 3, shape[2] // 2] = 1
    return np.stack([g[i] for i in order]), order


@pytest.mark.parametrize("shape", [(64, 64, 64), (25, 20, 15), (40, 40, 40)])
def test_grids_of_a_batch_do_not_see_each_other(gpu, shape):
    """A neighbour's planes must never enter a grid's x pass (or a neighbour's rows its y pass where several planes share a
    workgroup): all free beside all filled beside single voxels on the x faces."""
    for order in ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]):
        masks, order = _isolation_batch(shape, order)
        res = np.array([RES[i % 4] for i in range(6)])
        got, ext = _check_batch(gpu, masks, res, False, True)
        free, full = order.index(0), order.index(1)
        assert np.all(got[free] == INF) and ext[free] == (INF, INF)          # all free / all filled
        assert np.all(got[full] == -INF) and ext[full] == (-INF, -INF)
        _check_batch(gpu, masks, res, True, True)


def test_far_field_content_in_the_fast_path(gpu):
    """One filled voxel in a corner of 64^3 (D up to 3 * 63^2) and its complement: the sentinel and the largest D of the shape."""
    m = np.zeros((64, 64, 64), np.uint8)
    m[0, 0, 0] = 1
    masks = np.stack([m, 1 - m, m[::-1, ::-1, ::-1].copy()])
    for vb in (False, True):
        got, ext = _check_batch(gpu, masks, np.array([1.0, 0.01, 0.25]), vb, True)
    got, ext = gpu.build_batch(masks, 1.0, False)
    assert got[0, 63, 63, 63] == np.float32(np.sqrt(3 * 63 * 63)) and ext[0][0] == np.sqrt(3.0 * 63 * 63)


def _tagged_cells(shape, seed):
    rng = np.random.default_rng(seed)
    cells = np.zeros(shape, dtype=np.dtype([("occupancy", "<f4"), ("component", "<u4"), ("object_id", "<u4"), ("convex_segment", "<u4")]))
    cells["occupancy"] = rng.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), size=shape, p=[0.55, 0.1, 0.35])
    cells["object_id"] = rng.choice(np.array([0, 1, 2, 3, 5, 8, 13, 40], dtype=np.uint32), size=shape)
    cells["component"] = rng.integers(0, 2**32, size=shape, dtype=np.uint64).astype(np.uint32)
    return cells


def test_tagged_objects_one_field_per_id(gpu):
    shape = (48, 40, 36)
    cells = _tagged_cells(shape, 21)
    ids = [13, 2, 40, 7, 1, 2, 8, 5, 3]            # unsorted, 7 is absent from the grid, 2 comes twice
    assert len(ids) == 9 and 7 not in cells["object_id"]
    for unknown in (False, True):
        for vb in (False, True):
            got, ext = gpu.build_tagged_objects(cells, shape, ids, unknown_is_filled=unknown, resolution=0.25, add_virtual_border=vb)
            assert gpu.last_batch_info() == (True, 2)
            occ = (cells["occupancy"] > 0.5) | (unknown & (cells["occupancy"] == 0.5))
            for b, i in enumerate(ids):
                want, want_ext, _ = O.exact_sdf((occ & (cells["object_id"] == i)).astype(np.uint8), 0.25, vb)
                assert _bits_equal(got[b], want) and ext[b] == tuple(float(v) for v in want_ext), (i, unknown, vb)
                one, one_ext = gpu.build_tagged_cells(cells, shape, object_mode=2, object_ids=[i], unknown_is_filled=unknown,
                                                      resolution=0.25, add_virtual_border=vb)
                assert _bits_equal(got[b], one) and ext[b] == one_ext, (i, unknown, vb)
            if not vb:
                assert np.all(got[ids.index(7)] == INF)
            # cells = NULL: the records of the previous tagged call
            again, ext2 = gpu.build_tagged_objects(None, shape, ids, unknown_is_filled=unknown, resolution=0.25, add_virtual_border=vb)
            assert _bits_equal(again, got) and ext2 == ext
    # a shape outside the fast path takes one classify + single build per id: same fields
    shape2 = (6, 5, 130)
    cells2 = _tagged_cells(shape2, 22)
    got, ext = gpu.build_tagged_objects(cells2, shape2, [5, 1, 99], resolution=0.5)
    assert gpu.last_batch_info() == (False, -1)
    for b, i in enumerate([5, 1, 99]):
        want, want_ext, _ = O.exact_sdf(((cells2["occupancy"] > 0.5) & (cells2["object_id"] == i)).astype(np.uint8), 0.5, False)
        assert _bits_equal(got[b], want) and ext[b] == tuple(float(v) for v in want_ext)


@pytest.mark.parametrize("shape", [(64, 64, 64), (25, 20, 15), (20, 40, 1), (37, 5, 129)])
def test_gradient_batch_equals_gradient_per_grid(gpu, shape):
    import torch
    B = 5
    masks = np.stack([synth.bernoulli_mask(shape, (0.5, 0.05, 0.3)[b % 3], 70 + b) for b in range(B)])
    res = np.array([RES[b % 4] for b in range(B)])
    sdf, _ = gpu.build_batch(masks, res, False)
    d_sdf = torch.from_numpy(sdf).cuda()
    s = torch.cuda.current_stream().cuda_stream
    for f64, dt, it in ((True, torch.float64, np.uint64), (False, torch.float32, np.uint32)):
        for edge in (True, False):
            for per_grid in (True, False):
                r = res if per_grid else 0.05
                out = torch.full(tuple(sdf.shape) + (3,), 7.0, dtype=dt, device="cuda")
                gpu.gradient_batch_device(d_sdf.data_ptr(), B, shape, out.data_ptr(), r, edge, f64, s)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                for b in range(B):
                    one = torch.full(tuple(shape) + (3,), 9.0, dtype=dt, device="cuda")
                    gpu.gradient_device(d_sdf[b].data_ptr(), shape, one.data_ptr(), float(res[b]) if per_grid else 0.05, edge, f64, s)
                    torch.cuda.synchronize()
                    assert np.array_equal(got[b].view(it), one.cpu().numpy().view(it)), (shape, f64, edge, per_grid, b)


def test_utils_3d_batch_equals_a_loop_over_the_single_helper():
    from sdf_tools_amd import utils_3d
    rng = np.random.default_rng(5)
    B = 4
    env = (rng.random((B, 24, 30, 18)) < 0.2).astype(np.float32)          # [B, y, x, z]
    res = [0.05, 0.1, 0.02, 1.0]
    origin = rng.normal(size=(B, 3))
    sdf, grad = utils_3d.compute_sdf_and_gradient_batch(env, res, origin, B)
    assert sdf.shape == (B, 24, 30, 18) and sdf.dtype == np.float32
    assert grad.shape == (B, 24, 30, 18, 3) and grad.dtype == np.float32
    for b in range(B):
        s1, g1 = utils_3d.compute_sdf_and_gradient(env[b], res[b], origin[b])
        assert _bits_equal(sdf[b], s1), b
        assert _bits_equal(grad[b], g1), b


def test_single_builds_and_batches_share_a_handle():
    """single -> batch -> single of another shape on one handle: all three right, and sdfgpu_get_extrema keeps answering for the
    last SINGLE build; bad arguments are refused and leave the handle usable."""
    import torch
    g = capi.SdfGpu(0)
    try:
        m1 = synth.bernoulli_mask((32, 48, 64), 0.3, 1)
        s1, e1 = g.build(m1, 0.5)
        assert _bits_equal(s1, O.exact_sdf(m1, 0.5)[0])
        for shape in ((40, 40, 40), (37, 5, 129)):             # fast path, then one single build per grid
            masks = np.stack([synth.bernoulli_mask(shape, 0.1, 2 + b) for b in range(3)])
            _check_batch(g, masks, np.array([0.01, 1.0, 0.25]), True, shape == (40, 40, 40), single=False)
            assert g.get_extrema() == e1                           # the last single build's
            assert g.get_extrema_batch(3) == [tuple(float(v) for v in O.exact_sdf(masks[b], r, True)[1]) for b, r in enumerate((0.01, 1.0, 0.25))]
        m3 = synth.bernoulli_mask((20, 64, 96), 0.02, 9)
        s3, e3 = g.build(m3, 0.25, True)
        want3, want3_ext, _ = O.exact_sdf(m3, 0.25, True)
        assert _bits_equal(s3, want3) and e3 == tuple(float(v) for v in want3_ext)
        # device-resident batch on a PyTorch stream
        masks = np.stack([synth.bernoulli_mask((25, 20, 15), 0.2, 30 + b) for b in range(7)])
        d_m = torch.from_numpy(masks).cuda()
        d_o = torch.empty(masks.shape, dtype=torch.float32, device="cuda")
        res = np.array([RES[b % 4] for b in range(7)])
        g.build_batch_device(d_m.data_ptr(), 7, (25, 20, 15), d_o.data_ptr(), res, False, torch.cuda.current_stream().cuda_stream)
        res[:] = -1.0                                              # (read before the call returned)
        ext = g.get_extrema_batch(7)
        back = d_o.cpu().numpy()
        for b in range(7):
            want, want_ext, _ = O.exact_sdf(masks[b], RES[b % 4])
            assert _bits_equal(back[b], want) and ext[b] == tuple(float(v) for v in want_ext)
        # refused calls
        ok = np.zeros((2, 8, 8, 8), np.uint8)
        for bad in (lambda: g.build_batch(np.zeros((0, 8, 8, 8), np.uint8)),
                    lambda: g.build_batch(ok, 0.0),
                    lambda: g.build_batch(ok, np.array([1.0, float("nan")])),
                    lambda: g.build_batch(ok, np.array([1.0, -2.0])),
                    lambda: g.build_batch_device(0, 2, (8, 8, 8), d_o.data_ptr()),
                    lambda: g.build_batch_device(d_m.data_ptr(), 2, (8, 0, 8), d_o.data_ptr()),
                    lambda: g.get_extrema_batch(3),
                    lambda: g.build_tagged_objects(np.zeros((8, 8, 8, 4), np.uint32), (8, 8, 8), [1], cell_stride=16, object_id_offset=7),
                    lambda: g.build_tagged_objects(np.zeros((8, 8, 8, 4), np.uint32), (8, 8, 8), []),
                    lambda: g.gradient_batch_device(0, 2, (8, 8, 8), d_o.data_ptr())):
            with pytest.raises(capi.SdfGpuError) as ei:
                bad()
            assert ei.value.code == -1
            got, ext = g.build_batch(masks[:2], 1.0)
            assert _bits_equal(got[0], O.exact_sdf(masks[0], 1.0)[0]) and _bits_equal(got[1], O.exact_sdf(masks[1], 1.0)[0])
    finally:
        g.close()


def test_pysdf_tools_object_sdfs_and_batch_extraction(gpu):
    """MakeObjectSDFs / MakeAllObjectSDFs and ExtractSignedDistanceFieldBatch through the bindings: the same fields as the C ABI,
    under the same keys, OOB value +inf."""
    from sdf_tools_amd._bindings import load_pysdf_tools
    m = load_pysdf_tools()
    shape = (12, 10, 9)
    cells = _tagged_cells(shape, 31)
    grid = m.TaggedObjectCollisionMapGrid(m.Isometry3d([[1.0, 0, 0, 0.5], [0, 1.0, 0, -1.0], [0, 0, 1.0, 2.0], [0, 0, 0, 1.0]]), "world", 0.25,
                                          *shape, m.TAGGED_OBJECT_COLLISION_CELL(0.0, 0))
    for x in range(shape[0]):
        for y in range(shape[1]):
            for z in range(shape[2]):
                grid.SetValue(x, y, z, m.TAGGED_OBJECT_COLLISION_CELL(float(cells["occupancy"][x, y, z]), int(cells["object_id"][x, y, z])))
    ids = [13, 2, 40, 7, 1, 2, 8, 5, 3]
    for unknown in (False, True):
        for vb in (False, True):
            want, _ = gpu.build_tagged_objects(cells, shape, ids, unknown_is_filled=unknown, resolution=0.25, add_virtual_border=vb)
            got = grid.MakeObjectSDFs(ids, unknown, vb)
            assert sorted(got) == sorted(set(ids))
            for b, i in enumerate(ids):
                assert _bits_equal(got[i].GetRawDataNumpy().astype(np.float32), want[b]), (i, unknown, vb)
                assert got[i].GetValueByIndex(-1, 0, 0) == (INF, False) and got[i].GetResolution() == 0.25
            every = grid.MakeAllObjectSDFs(unknown, vb)
            present = sorted(int(v) for v in np.unique(cells["object_id"]) if v > 0)
            assert sorted(every) == present
            for i in present:
                occ = (cells["occupancy"] > 0.5) | (unknown & (cells["occupancy"] == 0.5))
                assert _bits_equal(every[i].GetRawDataNumpy().astype(np.float32), O.exact_sdf((occ & (cells["object_id"] == i)).astype(np.uint8), 0.25, vb)[0])
    assert grid.MakeObjectSDFs([], False, False) == {}
    # a batch of CollisionMapGrids, each with its own resolution and origin
    rng = np.random.default_rng(8)
    maps, occs = [], []
    for b, res in enumerate((0.05, 1.0, 0.25)):
        g = m.CollisionMapGrid(m.Isometry3d([[1.0, 0, 0, b], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]]), "f%d" % b, res, 20, 16, 12,
                               m.COLLISION_CELL(0.0))
        occ = rng.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), size=(20, 16, 12), p=[0.7, 0.1, 0.2])
        g.SetOccupancyFromNumpy(occ)
        maps.append(g)
        occs.append(occ)
    for unknown in (False, True):
        for vb in (False, True):
            out = m.ExtractSignedDistanceFieldBatch(maps, -3.0, unknown, vb)
            assert len(out) == 3
            for b, (sdf, ext) in enumerate(out):
                one, one_ext = maps[b].ExtractSignedDistanceField(-3.0, unknown, vb)
                assert _bits_equal(sdf.GetRawDataNumpy().astype(np.float32), one.GetRawDataNumpy().astype(np.float32)) and ext == one_ext
                assert sdf.GetFrame() == "f%d" % b and sdf.GetResolution() == maps[b].GetResolution() and sdf.GetValueByIndex(-1, 0, 0) == (-3.0, False)
                mask = ((occs[b] > 0.5) | (unknown & (occs[b] == 0.5))).astype(np.uint8)
                want, want_ext, _ = O.exact_sdf(mask, maps[b].GetResolution(), vb)
                assert _bits_equal(sdf.GetRawDataNumpy().astype(np.float32), want) and ext == tuple(float(v) for v in want_ext)
    other = m.CollisionMapGrid(m.Isometry3d([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]]), "w", 0.1, 20, 16, 13, m.COLLISION_CELL(0.0))
    with pytest.raises(ValueError):
        m.ExtractSignedDistanceFieldBatch(maps + [other], 0.0, False, False)
