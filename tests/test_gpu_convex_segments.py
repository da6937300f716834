"""Local extrema and convex segments on the MI355X (sdfgpu_local_extrema*, sdfgpu_convex_segments_cells, SignedDistanceField::
ComputeLocalExtremaMap, TaggedObjectCollisionMapGrid::UpdateConvexSegments): extremum triples, labels and K bit-equal to the C++
restatement of the reference (tests/convex_segments_restated.cpp), through every entry point."""
import ctypes
import math

import numpy as np
import pytest
import torch

import scenes
from sdf_tools_amd import capi, synth
from sdf_tools_amd._bindings import load_pysdf_tools
from test_convex_segments_cpu import restated_extrema, restated_segments, rot_z

pytestmark = pytest.mark.gpu

ODD_SHAPES = [(1, 1, 1), (1, 1, 77), (33, 2, 1), (25, 20, 15), (7, 65, 33)]


def _device_extrema(ctx, sdf, res, q):
    f = torch.from_numpy(np.ascontiguousarray(sdf, np.float32)).cuda()
    out = torch.empty(f.shape, dtype=torch.int32, device="cuda")
    ctx.local_extrema_device(f.data_ptr(), f.shape, res, out.data_ptr(), q, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _check_extrema(ctx, sdf, res, q=(1.0, 0.0, 0.0, 0.0)):
    """host and device forms against the restatement, bit for bit (NaN never occurs: a triple is a location or +inf)"""
    ref = restated_extrema(sdf, res, q)
    idx = ctx.local_extrema(sdf, res, q)
    got = capi.extremum_locations(idx, sdf.shape, res)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), "sdfgpu_local_extrema"
    assert np.array_equal(_device_extrema(ctx, sdf, res, q), idx), "sdfgpu_local_extrema_device"
    return idx


def _cells(occ, obj, component=7, segment=0xDEADBEEF):
    c = np.zeros(occ.shape + (4,), np.uint32)
    c[..., 0] = np.asarray(occ, np.float32).view(np.uint32)
    c[..., 1] = component
    c[..., 2] = obj
    c[..., 3] = segment
    return c


def _tagged_sdf(ctx, cells, res, border):
    shape = cells.shape[:3]
    if border:
        return ctx.build_tagged_cells(cells, shape, 0, (), True, res, True)[0]
    fr = ctx.build_tagged_cells(cells, shape, 0, (), True, res, False)[0]
    nm = ctx.build_tagged_cells(cells, shape, 1, (), True, res, False)[0]
    return np.where(fr >= 0.0, fr, np.where(nm <= -0.0, nm, np.float32(0.0))).astype(np.float32)


def _check_segments(ctx, occ, obj, res, threshold, border, q=(1.0, 0.0, 0.0, 0.0)):
    cells = _cells(occ, obj)
    sdf = _tagged_sdf(ctx, cells, res, border)
    ext = restated_extrema(sdf, res, q)
    ref, k_ref = restated_segments(occ, obj, ext, threshold)
    got = cells.copy()
    k = ctx.convex_segments_cells(got, occ.shape, res, threshold, border, q)
    assert k == k_ref
    assert np.array_equal(got[..., 3], ref), "labels"
    assert np.array_equal(got[..., :3], cells[..., :3]), "occupancy, component and object id are untouched"
    return ref, k


def _scene_cells(mask, seed=0):
    """occupancy from a mask, objects: filled cells split into named objects 1..3 by x thirds, one third left object 0"""
    occ = np.where(mask != 0, 1.0, 0.0).astype(np.float32)
    obj = np.zeros(mask.shape, np.uint32)
    nx = mask.shape[0]
    obj[: nx // 3][mask[: nx // 3] != 0] = 1
    obj[nx // 3: 2 * nx // 3][mask[nx // 3: 2 * nx // 3] != 0] = 2 + seed % 2
    return occ, obj


# ---- extrema --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ODD_SHAPES)
def test_extrema_odd_shapes_uniform_noise(gpu, shape):
    rng = np.random.default_rng(sum(shape))
    _check_extrema(gpu, (rng.random(shape) * 2 - 1).astype(np.float32), 0.5)


@pytest.mark.parametrize("shape", [(64, 64, 64), (40, 33, 45)])
def test_extrema_uniform_noise_has_cycles_of_many_lengths(gpu, shape):
    rng = np.random.default_rng(11)
    _check_extrema(gpu, rng.random(shape).astype(np.float32), 1.0)
    info = gpu.convex_last_info()
    assert info["cycles"] > 0 and info["longest_cycle"] >= 2
    assert 1 <= info["rounds"] <= math.ceil(math.log2(np.prod(shape))) + 1


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_extrema_bernoulli_sdfs(gpu, p):
    m = synth.bernoulli_mask((48, 40, 36), p, 5)
    sdf, _ = gpu.build(m, 0.1)
    _check_extrema(gpu, sdf, 0.1)


@pytest.mark.parametrize("deg", [30.0, -115.0])
def test_extrema_rotated_frames(gpu, deg):
    m, res = scenes.tutorial_scene()
    sdf, _ = gpu.build(m, res, True)
    q = rot_z(deg)
    idx = _check_extrema(gpu, sdf, res, q)
    assert not np.array_equal(idx, gpu.local_extrema(sdf, res))


def test_extrema_field_without_filled_voxels(gpu):
    f = np.full((9, 10, 11), np.inf, np.float32)
    idx = _check_extrema(gpu, f, 1.0)
    assert np.array_equal(idx.reshape(-1), np.arange(f.size, dtype=np.uint32))


def test_extrema_room_256(gpu):
    m = synth.room_mask_torch((256, 256, 256), "cpu").numpy()
    sdf, _ = gpu.build(m, 0.02)
    _check_extrema(gpu, sdf, 0.02)


# ---- segments -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [True, False])
def test_convex_segments_scene(gpu, border):
    m, res = scenes.convex_segments_scene()
    occ, obj = _scene_cells(m)
    _, k = _check_segments(gpu, occ, obj, res, 1.75, border)
    assert k > 1


@pytest.mark.parametrize("border", [True, False])
def test_tutorial_scene_segments(gpu, border):
    m, res = scenes.tutorial_scene()
    occ, obj = _scene_cells(m, 1)
    _check_segments(gpu, occ, obj, res, 1.75 * res, border)


@pytest.mark.parametrize("shape", ODD_SHAPES)
def test_segments_odd_shapes_bernoulli(gpu, shape):
    m = synth.bernoulli_mask(shape, 0.3, 9)
    occ, obj = _scene_cells(m)
    occ[::3, ::2] = np.where(occ[::3, ::2] == 0, np.float32(np.nan), occ[::3, ::2])     # unknown cells: NaN (no part unless named)
    for border in (True, False):
        _check_segments(gpu, occ, obj, 0.25, 0.6, border)


@pytest.mark.parametrize("deg", [30.0, 200.0])
def test_segments_rotated_frames(gpu, deg):
    m, res = scenes.convex_segments_scene()
    occ, obj = _scene_cells(m)
    _check_segments(gpu, occ, obj, res, 1.75, True, rot_z(deg))


def test_segments_threshold_edges(gpu):
    m, res = scenes.convex_segments_scene()
    occ, obj = _scene_cells(m)
    for thr in (0.0, 1.0, math.nextafter(1.0, 2.0), math.sqrt(2.0), math.nextafter(math.sqrt(2.0), 2.0), 40.0):
        _check_segments(gpu, occ, obj, res, thr, True)


def test_segments_room_256(gpu):
    m = synth.room_mask_torch((256, 256, 256), "cpu").numpy()
    occ, obj = _scene_cells(m)
    _check_segments(gpu, occ, obj, 0.02, 0.035, True)


# ---- C++ classes through pysdf_tools -----------------------------------------------------------------------------------------------
def _grid(P, occ, obj, res, q=None):
    T = np.eye(4)
    if q is not None:
        w, x, y, z = q
        T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = (0.3, -1.0, 2.0)
    g = P.TaggedObjectCollisionMapGrid(P.Isometry3d(T), "world", res, *occ.shape, P.TAGGED_OBJECT_COLLISION_CELL(0.0, 0))
    for (x, y, z) in np.argwhere((occ != 0) | np.isnan(occ) | (obj != 0)):
        g.SetValue(int(x), int(y), int(z), P.TAGGED_OBJECT_COLLISION_CELL(float(occ[x, y, z]), int(obj[x, y, z])))
    return g, T


@pytest.mark.parametrize("deg", [None, 30.0])
def test_cpp_classes(gpu, deg):
    P = load_pysdf_tools()
    m, res = scenes.convex_segments_scene()
    occ, obj = _scene_cells(m)
    g, T = _grid(P, occ, obj, res, None if deg is None else rot_z(deg))
    q = capi.quaternion_from_matrix(T[:3, :3])
    assert g.GetNumConvexSegments() == (0, False) and not g.AreConvexSegmentsValid()
    for border in (True, False):
        sdf_obj = g.ExtractSignedDistanceField(float("inf"), [], True, True)[0] if border else None
        if border:
            sdf = sdf_obj.GetRawDataNumpy()
            ref_ext = restated_extrema(sdf, res, q)
            assert np.array_equal(sdf_obj.ComputeLocalExtremaMapNumpy().view(np.uint64), ref_ext.view(np.uint64))
            idx = sdf_obj.ComputeLocalExtremaIndicesNumpy()
            assert np.array_equal(capi.extremum_locations(idx, sdf.shape, res).view(np.uint64), ref_ext.view(np.uint64))
        else:
            sdf = _tagged_sdf(gpu, _cells(occ, obj), res, False)
            ref_ext = restated_extrema(sdf, res, q)
        ref, k_ref = restated_segments(occ, obj, ref_ext, 1.75)
        comp_before = g.UpdateConnectedComponents()
        k = g.UpdateConvexSegments(1.75, border)
        assert k == k_ref and g.GetNumConvexSegments() == (k_ref, True) and g.AreConvexSegmentsValid()
        assert np.array_equal(g.GetConvexSegmentsNumpy(), ref)
        assert g.GetNumConnectedComponents() == (comp_before, True)
        cell = g.GetValueByIndex(50, 50, 25)[0]
        assert cell.convex_segment == ref[50, 50, 25] and cell.object_id == obj[50, 50, 25]


def test_cpp_refusals(gpu):
    P = load_pysdf_tools()
    g = P.TaggedObjectCollisionMapGrid(P.Isometry3d(np.eye(4)), "world", float("inf"), 4, 4, 4, P.TAGGED_OBJECT_COLLISION_CELL(1.0, 0))
    with pytest.raises(ValueError):                                    # (std::invalid_argument)
        g.UpdateConvexSegments(1.0, True)
    assert not g.AreConvexSegmentsValid()


# ---- refusals and handle state ------------------------------------------------------------------------------------------------------
def test_refusals_allocate_nothing(gpu):
    free0 = torch.cuda.mem_get_info()[0]
    f = np.zeros((2, 2, 2), np.float32)
    for res in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(capi.SdfGpuError) as ei:
            gpu.local_extrema(f, res)
        assert ei.value.code == -1
    # 2^32 - 1 and 2^32 voxels; 2^32 - 2 = 2 (2^31 - 1), where the last index would equal the kOnCycle marker
    qq = (ctypes.c_double * 8)(*capi.quaternion_and_inverse((1.0, 0.0, 0.0, 0.0)))
    for shape in ((65535, 65537, 1), (1 << 16, 1 << 8, 1 << 8), (1, 2, 2147483647), (2147483647, 2, 1)):
        with pytest.raises(capi.SdfGpuError) as ei:
            gpu.local_extrema_device(1 << 20, shape, 1.0, 1 << 20)
        assert ei.value.code == -1
        # the host entry point, with stand-in buffers: the size is refused before either is touched
        assert gpu._lib.sdfgpu_local_extrema(gpu._h, 1 << 20, *shape, 1.0, qq, 1 << 20) == -1, shape
        assert "2^32 - 2 voxels or more" in gpu._lib.sdfgpu_last_error(gpu._h).decode(), shape
    cells = _cells(np.zeros((2, 2, 2), np.float32), np.zeros((2, 2, 2), np.uint32))
    with pytest.raises(capi.SdfGpuError) as ei:
        gpu.convex_segments_cells(cells, (2, 2, 2), 0.0, 1.0, True)
    assert ei.value.code == -1
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)


def test_builds_and_components_unchanged_around_segments(gpu):
    m, res = scenes.convex_segments_scene()
    occ, obj = _scene_cells(m)
    fresh = capi.SdfGpu(0)
    try:
        want_sdf = fresh.build(m, res, True)
        want_cc = fresh.components(m)
        before = (gpu.build(m, res, True), gpu.components(m))
        gpu.convex_segments_cells(_cells(occ, obj), m.shape, res, 1.75, False)
        after = (gpu.build(m, res, True), gpu.components(m))
        for got in (before, after):
            assert np.array_equal(got[0][0], want_sdf[0]) and got[0][1] == want_sdf[1]
            assert np.array_equal(got[1][0], want_cc[0]) and got[1][1] == want_cc[1]
    finally:
        fresh.close()
