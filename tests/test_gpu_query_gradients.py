"""Smooth and autodiff gradients and DistanceToBoundary on the MI355X (sdfgpu_query_gradients*, DeviceSignedDistanceField::
QueryGradientsBatch): values, gradients and statuses bit-equal to the host core (SignedDistanceField::QueryGradient4d, via
QueryGradientsNumpyHost) on the downloaded field, through every entry point."""
import math

import numpy as np
import pytest
import torch

from sdf_tools_amd import capi, synth
from sdf_tools_amd._bindings import load_pysdf_tools
from test_gpu_projection import FRAMES, _field, _frame, _points, _same
from test_projection_cpu import inverse, rigid

pytestmark = pytest.mark.gpu
m = load_pysdf_tools()
KINDS = [capi.QUERY_SMOOTH_GRADIENT, capi.QUERY_AUTODIFF_GRADIENT, capi.QUERY_DISTANCE_TO_BOUNDARY]


def _windows(res, shape):
    return [res / 8, res, 3 * res, -res / 2, 0.0, (max(shape) + 2) * res]


def _check(d, ptr, host, res, origin, pts, kind, window, ctx=None):
    want = host.QueryGradientsNumpyHost(pts, kind, window)
    got = d.QueryGradientsBatch(pts, kind, window)
    for k, name in enumerate(("value", "gradient", "status")):
        assert _same(got[k], want[k]), "%s differs (kind %d, window %r) at %s" % (
            name, kind, window, np.argwhere(~np.all(np.atleast_2d(np.asarray(got[k]).view(np.uint8).reshape(len(pts), -1) ==
                                                                  np.asarray(want[k]).view(np.uint8).reshape(len(pts), -1)), axis=1))[:5].ravel())
    if ctx is not None:                                           # the C ABI host-buffer form and the device form, one handle
        shape = (host.GetNumXCells(), host.GetNumYCells(), host.GetNumZCells())
        got2 = ctx.query_gradients(ptr, shape, res, pts, inverse(origin), kind, window)
        for k in range(3):
            assert _same(got2[k], want[k])
        n = len(pts)
        if n:
            dp = torch.from_numpy(np.ascontiguousarray(pts, np.float64)).cuda()
            v = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
            g = torch.full((n, 3), -1.0, dtype=torch.float64, device="cuda")
            st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
            ctx.query_gradients_device(ptr, shape, res, dp.data_ptr(), n, inverse(origin), kind, window, math.inf, v.data_ptr(),
                                       g.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert _same(v.cpu().numpy(), want[0]) and _same(g.cpu().numpy(), want[1]) and _same(st.cpu().numpy(), want[2])
    return want


def _scenes():
    yield "bernoulli08", synth.bernoulli_mask((40, 33, 48), 0.08, 7), 0.05
    yield "bernoulli50", synth.bernoulli_mask((31, 40, 27), 0.5, 8), 0.03
    yield "room", synth.room_mask_torch((128, 128, 128), device="cpu").numpy(), 0.02
    yield "solid_boxes", synth.tutorial_boxes_mask_torch((128, 128, 128), device="cpu", solid=True).numpy(), 0.02


SCENES = ["bernoulli08", "bernoulli50", "room", "solid_boxes"]


@pytest.fixture(scope="module")
def ctx():
    c = capi.SdfGpu(0)
    yield c
    c.close()


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("scene", SCENES)
def test_gpu_equals_host_core(ctx, scene, frame):
    name, mask, res = next(s for s in _scenes() if s[0] == scene)
    origin, seed = _frame(frame)
    sdf, _ = ctx.build(mask, res)
    d, ptr, host = _field(ctx, sdf, res, origin)
    pts = _points(sdf, res, origin, mask, 1500, 3 * SCENES.index(scene) + seed)
    seen = set()
    for kind in KINDS:
        for window in (_windows(res, sdf.shape) if kind == capi.QUERY_SMOOTH_GRADIENT else [0.0]):
            want = _check(d, ptr, host, res, origin, pts, kind, window, ctx=ctx if window in (0.0, res) else None)
            seen |= set(np.unique(want[2]).tolist())
    assert {capi.QUERY_OK, capi.QUERY_OUTSIDE, capi.QUERY_WINDOW_TOO_LARGE, capi.QUERY_NON_FINITE} <= seen


@pytest.mark.parametrize("shape", [(37, 64, 1), (1, 1, 50), (64, 64, 64), (256, 256, 256)])
def test_odd_shapes(ctx, shape):
    res = 0.04
    mask = synth.bernoulli_mask(shape, 0.1, 3)
    sdf, _ = ctx.build(mask, res)
    origin = rigid(-0.8, (0.3, -0.2, 1.0))
    d, ptr, host = _field(ctx, sdf, res, origin)
    pts = _points(sdf, res, origin, mask, 3000, 17)
    for kind in KINDS:
        for window in (_windows(res, shape) if kind == capi.QUERY_SMOOTH_GRADIENT else [0.0]):
            _check(d, ptr, host, res, origin, pts, kind, window, ctx=ctx if window == 0.0 else None)


@pytest.mark.parametrize("fill", [0, 1])
def test_all_empty_and_all_filled(ctx, fill):
    res = 0.05
    mask = np.full((20, 17, 9), fill, np.uint8)
    sdf, _ = ctx.build(mask, res)
    d, ptr, host = _field(ctx, sdf, res, np.eye(4))
    pts = _points(sdf, res, np.eye(4), mask, 400, 5)
    for kind in KINDS:
        want = _check(d, ptr, host, res, np.eye(4), pts, kind, res, ctx=ctx)
        if kind == capi.QUERY_AUTODIFF_GRADIENT:
            ok = want[2] == capi.QUERY_OK
            assert ok.any() and np.isnan(want[0][ok]).all() and np.isnan(want[1][ok]).all()


def test_null_outputs_and_empty_batches(ctx):
    res = 0.05
    mask = synth.bernoulli_mask((40, 33, 48), 0.1, 3)
    sdf, _ = ctx.build(mask, res)
    origin = rigid(0.2, (0.1, -0.2, 0.3))
    d, ptr, host = _field(ctx, sdf, res, origin)
    pts = _points(sdf, res, origin, mask, 2000, 1)
    n = len(pts)
    dp = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    for kind in KINDS:
        want = host.QueryGradientsNumpyHost(pts, kind, res)
        outs = [torch.full((n,), 7.0, dtype=torch.float64, device="cuda"), torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda"),
                torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")]
        for only in range(3):                                     # one output at a time, the other two NULL
            ptrs = [outs[k].data_ptr() if k == only else 0 for k in range(3)]
            ctx.query_gradients_device(ptr, sdf.shape, res, dp.data_ptr(), n, inverse(origin), kind, res, math.inf, *ptrs)
        torch.cuda.synchronize()
        for k in range(3):
            assert _same(outs[k].cpu().numpy(), want[k])
        assert ctx.query_gradients(ptr, sdf.shape, res, pts, inverse(origin), kind, res, outputs=False) is None
        empty = ctx.query_gradients(ptr, sdf.shape, res, np.zeros((0, 3)), inverse(origin), kind, res)
        assert all(len(e) == 0 for e in empty)
        ctx.query_gradients_device(ptr, sdf.shape, res, 0, 0, inverse(origin), kind, res)    # n = 0: a no-op, null points allowed
        got = d.QueryGradientsBatch(np.zeros((0, 3)), kind, res)
        assert all(len(e) == 0 for e in got)


def test_refusals(ctx):
    res = 0.05
    sdf, _ = ctx.build(synth.bernoulli_mask((8, 9, 10), 0.2, 1), res)
    d, ptr, host = _field(ctx, sdf, res, np.eye(4))
    pts = np.full((4, 3), 0.2)
    eye = np.eye(4)

    def refused(word, d_sdf=None, shape=sdf.shape, resolution=res, w2g=eye, kind=capi.QUERY_SMOOTH_GRADIENT, window=res):
        with pytest.raises(capi.SdfGpuError) as ei:
            ctx.query_gradients(ptr if d_sdf is None else d_sdf, shape, resolution, pts, w2g, kind, window)
        assert ei.value.code == -1 and "gradient query" in str(ei.value) and word in str(ei.value)

    refused("null field", d_sdf=0)
    refused("resolution", resolution=0.0)
    refused("resolution", resolution=-1.0)
    refused("resolution", resolution=math.nan)
    refused("resolution", resolution=math.inf)
    refused("grid", shape=(0, 9, 10))
    refused("grid", shape=(8, -9, 10))
    refused("grid", shape=(2 ** 40, 2 ** 40, 2))
    refused("world_to_grid", w2g=None)
    refused("kind", kind=3)
    refused("kind", kind=-1)
    for bad in (math.nan, math.inf, -math.inf):
        refused("window", window=bad)
    with pytest.raises(capi.SdfGpuError) as ei:
        ctx.query_gradients_device(ptr, sdf.shape, res, 0, 4, eye, capi.QUERY_AUTODIFF_GRADIENT)
    assert ei.value.code == -1 and "null points" in str(ei.value)
    with pytest.raises(ValueError):                                                    # host members: std::invalid_argument
        d.QueryGradientsBatch(pts, capi.QUERY_SMOOTH_GRADIENT, math.nan)
    with pytest.raises(ValueError):
        host.QueryGradientsNumpyHost(pts, capi.QUERY_SMOOTH_GRADIENT, math.inf)


def test_reference_named_members_agree_with_the_batch(ctx):
    res = 0.02
    mask = synth.tutorial_boxes_mask_torch((64, 64, 64), device="cpu", solid=True).numpy()
    sdf, _ = ctx.build(mask, res)
    origin = rigid(0.4, (0.2, 0.1, -0.3))
    d, ptr, host = _field(ctx, sdf, res, origin)
    pts = _points(sdf, res, origin, mask, 80, 5)[:-4]
    ad = d.QueryGradientsBatch(pts, capi.QUERY_AUTODIFF_GRADIENT)
    sm = d.QueryGradientsBatch(pts, capi.QUERY_SMOOTH_GRADIENT, res / 8)
    bd = d.QueryGradientsBatch(pts, capi.QUERY_DISTANCE_TO_BOUNDARY)
    for i, p in enumerate(pts):
        g = host.GetAutoDiffGradient(*p)
        assert (g == []) == (ad[2][i] == capi.QUERY_OUTSIDE) and (g == [] or _same(np.array(g), ad[1][i]))
        if sm[2][i] == capi.QUERY_WINDOW_TOO_LARGE:           # an edge point whose two window ends leave through two faces
            with pytest.raises(RuntimeError, match="Window size for GetSmoothGradient is too large for SDF"):
                host.GetSmoothGradient(*p, res / 8)
        else:
            g = host.GetSmoothGradient(*p, res / 8)
            assert (g == []) == (sm[2][i] == capi.QUERY_OUTSIDE) and (g == [] or _same(np.array(g), sm[1][i]))
        v, inside = host.DistanceToBoundary(*p)
        assert _same(np.array([v]), bd[0][i:i + 1]) and inside == (bd[2][i] == capi.QUERY_OK)


def test_redzone_clean():
    """the main case's kinds on a fresh context in red-zone mode: every store of the kernel and of the staging stays inside its buffer"""
    rz = capi.SdfGpu(0)
    try:
        rz.set_option("redzone", 1)
        res = 0.05
        mask = synth.bernoulli_mask((40, 33, 48), 0.08, 9)
        sdf, _ = rz.build(mask, res)
        ptr = rz.device_malloc(sdf.nbytes)
        rz.copy_from_host(ptr, sdf)
        origin = rigid(0.9, (1.0, 2.0, 3.0))
        pts = _points(sdf, res, origin, mask, 700, 2)
        n = len(pts)
        dbuf = rz.device_malloc(n * 24)
        vbuf, gbuf, sbuf = rz.device_malloc(n * 8), rz.device_malloc(n * 24), rz.device_malloc(n)
        rz.copy_from_host(dbuf, np.ascontiguousarray(pts))
        for kind in KINDS:
            for window in (_windows(res, sdf.shape) if kind == capi.QUERY_SMOOTH_GRADIENT else [0.0]):
                rz.query_gradients(ptr, sdf.shape, res, pts, inverse(origin), kind, window)
                rz.query_gradients_device(ptr, sdf.shape, res, dbuf, n, inverse(origin), kind, window, math.inf, vbuf, gbuf, sbuf)
        rz.redzone_check()
        for p in (dbuf, vbuf, gbuf, sbuf, ptr):
            rz.device_free(p)
    finally:
        rz.close()


def test_field_past_2_31_cells(ctx):
    """1300 x 1300 x 1272 = 2.15e9 cells: queries in the last x planes, where linear cell indices exceed 2^31, on the downloaded field"""
    shape = (1300, 1300, 1272)
    res = 0.01
    assert shape[0] * shape[1] * shape[2] > 2 ** 31
    mt = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    mt[1285:, 900:1100, 600:700] = 1
    mt[:, :, :2] = 1
    d = m.DeviceSignedDistanceField(m.Isometry3d(np.eye(4)), "world", res, *shape, math.inf)
    ptr = d.DevicePointer()
    ctx.build_device(mt.data_ptr(), shape, ptr, res, False, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del mt
    torch.cuda.empty_cache()
    host = d.Host()
    try:
        rng = np.random.default_rng(4)
        deep = np.column_stack([rng.uniform(1298, 1300, 300), rng.uniform(950, 1050, 300), rng.uniform(620, 680, 300)])
        cells = np.floor(deep)
        assert ((cells[:, 0] * shape[1] + cells[:, 1]) * shape[2] + cells[:, 2] > 2 ** 31).all()
        g = np.concatenate([deep, np.column_stack([rng.uniform(1290, 1300.5, 200), rng.uniform(0, 1300, 200), rng.uniform(-1, 3, 200)])]) * res
        for kind in KINDS:
            want = _check(d, ptr, host, res, np.eye(4), g, kind, res, ctx=ctx)
            assert (want[2][:300] == capi.QUERY_OK).all()
    finally:
        del host
