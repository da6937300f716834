"""Projection out of collision / into the valid volume on the MI355X (sdfgpu_project_points*, DeviceSignedDistanceField::
ProjectBatch): locations, statuses and step counts bit-equal to the host counted walk (SignedDistanceField::ProjectCounted4d, via
ProjectOutOfCollisionNumpyHost) on the downloaded field, through every entry point."""
import math

import numpy as np
import pytest
import torch

from sdf_tools_amd import capi, synth
from sdf_tools_amd._bindings import load_pysdf_tools
from test_projection_cpu import inverse, rigid

pytestmark = pytest.mark.gpu
m = load_pysdf_tools()

MODES = [False, True]                      # into_valid_volume_only
MULTIPLIERS = [0.125, 0.5]
# "rotated" turns about z, which leaves the z couplings of both transforms at zero; "general" (all nine rotation entries nonzero)
# and "cyclic" (x -> y -> z -> x, R != R^T) of tests/frame_judge.py do not
FRAMES = ["identity", "rotated", "general", "cyclic"]


def _frame(frame):
    """(origin, what the frame adds to the seed of a scene's points)"""
    if frame == "identity":
        return np.eye(4), 0
    if frame == "rotated":
        return rigid(0.6, (-0.4, 1.25, 0.3)), 1
    import frame_judge
    return frame_judge.frames()[frame], {"general": 2, "cyclic": 100}[frame]


def _field(ctx, sdf, res, origin):
    """sdf (float32 [nx, ny, nz], host) -> (DeviceSignedDistanceField holding it, its device address, the downloaded host field)"""
    sdf = np.ascontiguousarray(sdf, np.float32)
    d = m.DeviceSignedDistanceField(m.Isometry3d(origin), "world", float(res), *sdf.shape, math.inf)
    ptr = d.DevicePointer()
    ctx.copy_from_host(ptr, sdf)
    torch.cuda.synchronize()
    host = d.Host()
    assert np.array_equal(host.GetRawDataNumpy().view(np.uint32), sdf.view(np.uint32))
    return d, ptr, host


def _points(sdf, res, origin, mask, n_random, seed):
    """world-frame points: uniform over the grid and a margin around it (inside and outside), on faces, edges and corners (grid
    frame 0 and size exactly, and size - res 1e-4), deep in obstacles (cells of `mask`, jittered), and NaN / inf"""
    rng = np.random.default_rng(seed)
    size = np.array(sdf.shape, np.float64) * res
    g = [rng.uniform(-0.1, 1.1, (n_random, 3)) * size]
    faces = rng.uniform(0.0, 1.0, (64, 3)) * size
    for k in range(64):
        faces[k, k % 3] = (0.0, size[k % 3], size[k % 3] - res * 1e-4, res * 1e-4)[(k // 3) % 4]
    g.append(faces)
    g.append(np.array([[a, b, c] for a in (0.0, size[0]) for b in (0.0, size[1]) for c in (0.0, size[2])]))
    cells = np.argwhere(mask != 0)
    if len(cells):
        pick = cells[rng.integers(0, len(cells), min(len(cells), n_random))]
        g.append((pick + rng.uniform(0.02, 0.98, pick.shape)) * res)
    g = np.concatenate(g)
    o = np.asarray(origin, np.float64)
    w = np.empty_like(g)                                          # origin * (g, 1), eigen_lite's order
    for i in range(3):
        w[:, i] = o[i, 0] * g[:, 0] + o[i, 1] * g[:, 1] + o[i, 2] * g[:, 2] + o[i, 3]
    bad = np.array([[math.nan, 0.5, 0.5], [0.5, math.inf, 0.5], [0.5, 0.5, -math.inf], [math.nan] * 3])
    return np.concatenate([w, bad])


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def _check(d, ptr, host, res, origin, pts, md, mult, valid_only, max_steps=0, ctx=None):
    want = host.ProjectOutOfCollisionNumpyHost(pts, md, mult, max_steps, valid_only)
    got = d.ProjectBatch(pts, md, mult, max_steps, valid_only)
    for k, name in enumerate(("location", "status", "steps")):
        assert _same(got[k], want[k]), "%s differs at %s" % (name, np.argwhere(~np.all(np.atleast_2d(
            np.asarray(got[k]).view(np.uint8).reshape(len(pts), -1) == np.asarray(want[k]).view(np.uint8).reshape(len(pts), -1)), axis=1))[:5].ravel())
    if ctx is not None:                                           # the C ABI host-buffer form, its own handle
        shape = (host.GetNumXCells(), host.GetNumYCells(), host.GetNumZCells())
        got2 = ctx.project_points(ptr, shape, res, pts, inverse(origin), origin, md, mult, max_steps, valid_only)
        for k in range(3):
            assert _same(got2[k], want[k])
    return want


def _scenes():
    yield "bernoulli", synth.bernoulli_mask((40, 33, 48), 0.1, 7), 0.05
    yield "room", synth.room_mask_torch((128, 128, 128), device="cpu").numpy(), 0.02
    yield "solid_boxes", synth.tutorial_boxes_mask_torch((128, 128, 128), device="cpu", solid=True).numpy(), 0.02


@pytest.fixture(scope="module")
def ctx():
    c = capi.SdfGpu(0)
    yield c
    c.close()


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("scene", ["bernoulli", "room", "solid_boxes"])
def test_gpu_equals_host_walk(ctx, scene, frame):
    name, mask, res = next(s for s in _scenes() if s[0] == scene)
    origin, seed = _frame(frame)
    sdf, _ = ctx.build(mask, res)
    d, ptr, host = _field(ctx, sdf, res, origin)
    pts = _points(sdf, res, origin, mask, 1500, 3 * ["bernoulli", "room", "solid_boxes"].index(scene) + seed)
    seen = set()
    for valid_only in MODES:
        for md in (0.0, 1.5 * res, 4.0 * res):
            for mult in MULTIPLIERS:
                want = _check(d, ptr, host, res, origin, pts, md, mult, valid_only, ctx=ctx if md == 0.0 else None)
                seen |= set(np.unique(want[1]).tolist())
    assert {capi.PROJECT_CONVERGED, capi.PROJECT_NON_FINITE} <= seen
    if scene != "bernoulli":
        assert int(host.ProjectOutOfCollisionNumpyHost(pts, 0.0, 0.125)[2].max()) > 20          # deep walks were exercised


def test_failing_walks_and_the_step_limit(ctx):
    """flat gradients (medial planes of a slab), walks that leave the grid (a minimum distance beyond any distance), and the step
    limit (max_steps 1 and 7): the status, the step count and the last location reached agree"""
    res = 0.1
    mask = np.zeros((41, 20, 17), np.uint8)
    mask[10:31] = 1
    sdf, _ = ctx.build(mask, res)
    origin = rigid(-0.3, (0.5, 0.25, -1.0))
    d, ptr, host = _field(ctx, sdf, res, origin)
    pts = _points(sdf, res, origin, mask, 800, 11)
    statuses = set()
    for md, max_steps in ((0.0, 0), (0.0, 1), (0.0, 7), (5.0, 0), (0.2, 3)):
        want = _check(d, ptr, host, res, origin, pts, md, 0.125, False, max_steps, ctx=ctx)
        statuses |= set(np.unique(want[1]).tolist())
    assert {capi.PROJECT_CONVERGED, capi.PROJECT_FLAT_GRADIENT, capi.PROJECT_LEFT_GRID, capi.PROJECT_STEP_LIMIT,
            capi.PROJECT_NON_FINITE} <= statuses


@pytest.mark.parametrize("n", [0, 1, 1000, 70001])
def test_batch_sizes_and_device_form(ctx, n):
    mask = synth.bernoulli_mask((40, 33, 48), 0.1, 3)
    res = 0.05
    sdf, _ = ctx.build(mask, res)
    origin = rigid(0.2, (0.1, -0.2, 0.3))
    d, ptr, host = _field(ctx, sdf, res, origin)
    rng = np.random.default_rng(n)
    pts = (rng.uniform(-0.05, 1.05, (n, 3)) * np.array(sdf.shape) * res) if n else np.zeros((0, 3))
    for valid_only in MODES:
        want = _check(d, ptr, host, res, origin, pts, 0.5 * res, 0.125, valid_only, ctx=ctx)
        # the device form on the caller's stream
        dp = torch.from_numpy(np.ascontiguousarray(pts, np.float64)).cuda()
        out = torch.full((n, 3), -1.0, dtype=torch.float64, device="cuda")
        st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        sp = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ctx.project_points_device(ptr, sdf.shape, res, dp.data_ptr() if n else 0, n, out.data_ptr() if n else 0, inverse(origin),
                                  origin, 0.5 * res, 0.125, 0, valid_only, st.data_ptr() if n else 0, sp.data_ptr() if n else 0,
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy(), want[0]) and _same(st.cpu().numpy(), want[1]) and _same(sp.cpu().numpy(), want[2])
        if n:                                                     # status and steps may be NULL
            out2 = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
            ctx.project_points_device(ptr, sdf.shape, res, dp.data_ptr(), n, out2.data_ptr(), inverse(origin), origin, 0.5 * res,
                                      0.125, 0, valid_only)
            torch.cuda.synchronize()
            assert _same(out2.cpu().numpy(), want[0])


def test_refusals(ctx):
    res = 0.05
    sdf, _ = ctx.build(synth.bernoulli_mask((8, 9, 10), 0.2, 1), res)
    d, ptr, host = _field(ctx, sdf, res, np.eye(4))
    pts = np.full((4, 3), 0.2)
    eye = np.eye(4)
    ok = dict(shape=sdf.shape, resolution=res, points=pts, world_to_grid=eye, grid_to_world=eye)

    def refused(**kw):
        a = dict(ok, **kw)
        with pytest.raises(capi.SdfGpuError) as ei:
            ctx.project_points(kw.get("d_sdf", ptr), a["shape"], a["resolution"], a["points"], a["world_to_grid"], a["grid_to_world"],
                               kw.get("minimum_distance", 0.0), kw.get("stepsize_multiplier", 0.125), kw.get("max_steps", 0))
        assert ei.value.code == -1 and "projection" in str(ei.value)

    refused(d_sdf=0)
    refused(resolution=0.0)
    refused(resolution=-1.0)
    refused(resolution=math.nan)
    refused(stepsize_multiplier=0.0)
    refused(stepsize_multiplier=-0.5)
    refused(stepsize_multiplier=math.inf)
    refused(max_steps=-1)
    refused(shape=(0, 9, 10))
    refused(shape=(8, -9, 10))
    refused(world_to_grid=None)
    refused(grid_to_world=None)
    with pytest.raises(capi.SdfGpuError) as ei:
        ctx.project_points_device(ptr, sdf.shape, res, 0, 4, 0, eye, eye)
    assert ei.value.code == -1
    with pytest.raises(capi.SdfGpuError) as ei:
        dp = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
        ctx.project_points_device(ptr, sdf.shape, res, dp.data_ptr(), 4, dp.data_ptr(), eye, eye, mode=7)
    assert ei.value.code == -1 and "mode" in str(ei.value)
    ctx.project_points_device(ptr, sdf.shape, res, 0, 0, 0, eye, eye)                # n = 0: a no-op, null points allowed
    with pytest.raises(ValueError):                                                    # host members: std::invalid_argument
        d.ProjectBatch(pts, 0.0, 0.0)
    with pytest.raises(ValueError):
        host.ProjectOutOfCollisionNumpyHost(pts, 0.0, 0.125, -1)


def test_reference_named_members_agree_with_the_batch(ctx):
    res = 0.02
    mask = synth.tutorial_boxes_mask_torch((64, 64, 64), device="cpu", solid=True).numpy()
    sdf, _ = ctx.build(mask, res)
    origin = rigid(0.4, (0.2, 0.1, -0.3))
    d, ptr, host = _field(ctx, sdf, res, origin)
    pts = _points(sdf, res, origin, mask, 60, 5)[:-4]
    got = d.ProjectBatch(pts, 0.03, 0.125, 0, False)
    for i, p in enumerate(pts):
        if got[1][i] == capi.PROJECT_CONVERGED:
            r = host.ProjectOutOfCollisionToMinimumDistance(*p, 0.03)
            assert _same(np.array(r), got[0][i])
        elif got[1][i] == capi.PROJECT_FLAT_GRADIENT:
            with pytest.raises(RuntimeError, match="flat gradient"):
                host.ProjectOutOfCollisionToMinimumDistance(*p, 0.03)
    v = d.ProjectBatch(pts, 0.0, 0.125, 0, True)
    for i, p in enumerate(pts):
        assert _same(np.array(host.ProjectIntoValidVolume(*p)), v[0][i])
    with pytest.raises(ValueError):
        host.ProjectOutOfCollision(math.nan, 0.0, 0.0)


def test_redzone_clean():
    """one run on a fresh context in red-zone mode: every store of the kernel and of the staging stays inside its buffer"""
    rz = capi.SdfGpu(0)
    try:
        rz.set_option("redzone", 1)
        res = 0.05
        mask = synth.bernoulli_mask((40, 33, 48), 0.1, 9)
        sdf, _ = rz.build(mask, res)
        ptr = rz.device_malloc(sdf.nbytes)
        rz.copy_from_host(ptr, sdf)
        origin = rigid(0.9, (1.0, 2.0, 3.0))
        pts = _points(sdf, res, origin, mask, 700, 2)
        for valid_only in MODES:
            rz.project_points(ptr, sdf.shape, res, pts, inverse(origin), origin, 0.1, 0.125, 0, valid_only)
        n = len(pts)
        dbuf = rz.device_malloc(n * 24)
        obuf, sbuf, tbuf = rz.device_malloc(n * 24), rz.device_malloc(n), rz.device_malloc(n * 4)
        rz.copy_from_host(dbuf, np.ascontiguousarray(pts))
        rz.project_points_device(ptr, sdf.shape, res, dbuf, n, obuf, inverse(origin), origin, 0.1, 0.125, 0, False, sbuf, tbuf)
        rz.redzone_check()
        for p in (dbuf, obuf, sbuf, tbuf, ptr):
            rz.device_free(p)
    finally:
        rz.close()


def test_field_past_2_31_cells(ctx):
    """1300 x 1300 x 1272 = 2.15e9 cells: walks in the last x planes, where linear cell indices exceed 2^31, on the downloaded field"""
    shape = (1300, 1300, 1272)
    res = 0.01
    assert shape[0] * shape[1] * shape[2] > 2 ** 31
    mt = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    mt[1285:, 900:1100, 600:700] = 1                              # a block against the far x face
    mt[:, :, :2] = 1                                              # and a floor
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
        for md in (0.0, 0.05):
            want = _check(d, ptr, host, res, np.eye(4), g, md, 0.125, False, ctx=ctx)
            assert want[2][:300].min() > 80 and (want[1] == capi.PROJECT_CONVERGED).mean() > 0.9
    finally:
        del host
