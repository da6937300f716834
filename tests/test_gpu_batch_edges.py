"""GPU: fixed inputs aimed at the machinery of the batched small-grid build that seeded noise does not reach
(sdf_tools_amd/csrc/sdfgpu_batch.hip): every value of P (planes per workgroup of k_batch_zy) and the plane
sizes either side of its changes, workgroups that straddle two grids, the z pass's hop between a row's two 64-bit words, the
tiles of k_batch_x_finish, the int16 plane field's largest finite value (2 * 127^2 = 32258) beside its sentinel (32767),
structured far-field scenes, the pinned parameter ring growing and wrapping, k_batch_gradient past 65535 grids, streams, and a
launch of 2^32 threads and more.

The yardstick is oracle.exact_sdf, every voxel as uint32 and the extrema as exact doubles; the single build of each grid is the
second comparison.  Everything runs with red zones on and device buffers of exact size from sdfgpu_device_malloc (the ring wrap
also with red zones off, where calls stay asynchronous)."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O
from sdf_tools_amd import capi, synth

import analysis_scenes as A

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_batch as FB  # noqa: E402  (the scene families and the restated launch plan)

pytestmark = pytest.mark.gpu

RES = (1.0, 0.5, 0.25, 0.05, 0.037, 0.01)
INF = float("inf")


@pytest.fixture
def rz(gpu):
    gpu.set_option("redzone", 1)
    yield gpu
    gpu.set_option("redzone", 0)


@pytest.fixture
def fresh():
    """A handle of its own: its pinned parameter ring still has its first size (64 KiB), whatever ran on the shared one."""
    ctx = capi.SdfGpu(0)
    yield ctx
    ctx.close()


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _planes_per_workgroup(shape, batch):
    """P = max(1, min(1024 / (ny nz), 8, B nx)) with singleton axes moved to the front"""
    dims = [int(s) for s in shape if s > 1]
    nx, ny, nz = [1] * (3 - len(dims)) + dims
    return max(1, min(1024 // (ny * nz), 8, batch * nx))


def _device_batch(ctx, masks, res, vb, stream=0):
    B, n = masks.shape[0], int(np.prod(masks.shape[1:]))
    d_in, d_out = ctx.device_malloc(B * n), ctx.device_malloc(B * n * 4)
    ctx.copy_from_host(d_in, masks)
    r = np.array(res, np.float64) if np.ndim(res) else res
    ctx.build_batch_device(d_in, B, masks.shape[1:], d_out, r, vb, stream)
    if np.ndim(res):
        r[:] = -1.0
    ext = ctx.get_extrema_batch(B)
    got = ctx.copy_to_host(np.empty(masks.shape, np.float32), d_out)
    ctx.device_free(d_in)
    ctx.device_free(d_out)
    return got, ext


def _check(ctx, masks, res, vb, fast=True, single=True):
    """host and device entry points against the oracle and (once) against the single builds; returns the fields"""
    masks = np.ascontiguousarray(masks, np.uint8)
    B = masks.shape[0]
    rs = [float(v) for v in res] if np.ndim(res) else [float(res)] * B
    wants = [O.exact_sdf(masks[b], rs[b], vb) for b in range(B)]
    for name in ("host", "device"):
        got, ext = ctx.build_batch(masks, res, vb) if name == "host" else _device_batch(ctx, masks, res, vb)
        assert ctx.last_batch_info() == ((True, 2) if fast else (False, -1)), (name, masks.shape)
        assert got.shape == masks.shape and got.dtype == np.float32 and len(ext) == B
        for b in range(B):
            want, want_ext, _ = wants[b]
            assert _bits_equal(got[b], want), (name, "oracle", masks.shape, b, vb, int((got[b].view(np.uint32) != want.view(np.uint32)).sum()),
                                               np.argwhere(got[b].view(np.uint32) != want.view(np.uint32))[:3].tolist())
            assert ext[b] == tuple(float(v) for v in want_ext), (name, "extrema", masks.shape, b, vb, ext[b], want_ext)
    if single:
        for b in range(B):
            one, one_ext = ctx.build(masks[b], rs[b], vb)
            assert _bits_equal(got[b], one) and ext[b] == one_ext, ("single build", masks.shape, b, vb)
    return got, ext


def _mixed(shape, B, seed):
    """all filled beside all free beside noise, a voxel on the last x plane, a structured scene, ...: grid b of a batch"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        k = b % 6
        if k == 0:
            m = np.ones(shape, np.uint8)
        elif k == 1:
            m = np.zeros(shape, np.uint8)
        elif k == 2:
            m = synth.bernoulli_mask(shape, 0.5, seed + b)
        elif k == 3:
            m = np.zeros(shape, np.uint8)
            m[shape[0] - 1, shape[1] - 1, shape[2] - 1] = 1
        elif k == 4:
            m = FB.structured(rng, shape)
        else:
            m = synth.bernoulli_mask(shape, 0.01, seed + b)
        out.append(m)
    return np.stack(out)


# ---- planes per workgroup ----------------------------------------------------------------------------------------------------------
# (shape, B, P, what the row is for)
PLANES = [
    ((4, 33, 32), 2, 1, "P = 1"),
    ((3, 16, 25), 3, 2, "P = 2, B nx % P = 1 = P - 1"),
    ((25, 20, 15), 2, 3, "P = 3, B nx % P = P - 1"),
    ((5, 20, 15), 2, 3, "P = 3, B nx % P = 1"),
    ((3, 16, 15), 3, 4, "P = 4, B nx % P = 1"),
    ((5, 16, 15), 3, 4, "P = 4, B nx % P = P - 1"),
    ((3, 20, 10), 3, 5, "P = 5, B nx % P = P - 1"),
    ((7, 20, 10), 3, 5, "P = 5, B nx % P = 1"),
    ((7, 10, 16), 1, 6, "P = 6, B nx % P = 1"),
    ((11, 10, 16), 1, 6, "P = 6, B nx % P = P - 1"),
    ((5, 9, 16), 4, 7, "P = 7, B nx % P = P - 1"),
    ((5, 9, 16), 3, 7, "P = 7, B nx % P = 1"),
    ((11, 8, 8), 3, 8, "P = 8, B nx % P = 1"),
    ((5, 8, 8), 3, 8, "P = 8, B nx % P = P - 1"),
    ((5, 8, 16), 3, 8, "a plane of 128 cells"),
    ((5, 3, 43), 3, 7, "a plane of 129 cells"),
    ((5, 16, 32), 2, 2, "a plane of 512 cells"),
    ((5, 19, 27), 2, 1, "a plane of 513 cells"),
    ((4, 33, 31), 3, 1, "a plane of 1023 cells"),
    ((4, 32, 32), 3, 1, "a plane of 1024 cells"),
    ((4, 25, 41), 3, 1, "a plane of 1025 cells"),
    ((1, 8, 8), 2, 2, "B nx < P"),
    ((2, 4, 4), 1, 2, "B nx < P"),
    ((3, 2, 2), 2, 6, "B nx < P"),
    ((5, 1, 1), 3, 3, "B nx < P: a line (canonical 1 x 1 x 5)"),
    ((20, 40, 1), 2, 1, "a singleton z axis moves to the front: the plane is 20 x 40"),
    ((4, 20, 15), 2, 3, "workgroup 1 holds the last plane of grid 0 (all filled) and two planes of grid 1 (all free)"),
]


@pytest.mark.parametrize("vb", [False, True], ids=["noborder", "border"])
@pytest.mark.parametrize("shape,B,P,what", PLANES, ids=["%s-B%d-P%d" % ("x".join(map(str, r[0])), r[1], r[2]) for r in PLANES])
def test_every_planes_per_workgroup_and_the_plane_sizes_where_it_changes(rz, shape, B, P, what, vb):
    assert _planes_per_workgroup(shape, B) == P == FB.planes_per_workgroup(shape, B), what
    masks = _mixed(shape, B, 11)
    _check(rz, masks, np.array([RES[(b + 1) % 6] for b in range(B)]), vb)
    _check(rz, masks[::-1].copy(), 0.05, vb, single=False)


def test_the_table_covers_what_it_says():
    canon = [(FB.canonical(r[0]), r[1], r[2]) for r in PLANES]             # (singleton axes in front: nx and the plane are these)
    assert {P for _, _, P in canon} == set(range(1, 9))
    assert {128, 129, 512, 513, 1023, 1024, 1025} <= {c[1] * c[2] for c, _, _ in canon}
    for P in range(2, 9):                                                  # both remainders for every P
        rem = {(B * c[0]) % P for c, B, p in canon if p == P}
        assert {1, P - 1} <= rem, (P, rem)
    assert any(B * c[0] < min(1024 // (c[1] * c[2]), 8) for c, B, _ in canon)


@pytest.mark.parametrize("vb", [False, True], ids=["noborder", "border"])
def test_a_workgroup_that_straddles_an_all_filled_and_an_all_free_grid(rz, vb):
    for shape, B in (((4, 20, 15), 4), ((3, 8, 8), 5), ((1, 5, 7), 6)):
        P = _planes_per_workgroup(shape, B)
        assert P > 1 and shape[0] % P != 0
        masks = np.stack([np.full(shape, (b + 1) % 2, np.uint8) for b in range(B)])
        got, ext = _check(rz, masks, np.array([RES[b % 6] for b in range(B)]), vb)
        if not vb:
            for b in range(B):
                v = -INF if b % 2 == 0 else INF
                assert np.all(got[b] == v) and ext[b] == (v, v)


# ---- z rows ------------------------------------------------------------------------------------------------------------------------
def _z_rows(nz):
    """rows of nz voxels: one filled voxel at the word edges and the row's end, blocks that fill exactly one of the two 64-bit
    words, a pair whose nearer member lies in the other word from the voxels between them; and every complement"""
    rows = []
    for z in sorted({z for z in (0, 31, 32, 63, 64, nz - 1) if z < nz}):
        r = np.zeros(nz, np.uint8)
        r[z] = 1
        rows.append(r)
    if nz > 64:
        r = np.zeros(nz, np.uint8)
        r[:64] = 1                           # the only free voxels are in the high word
        rows.append(r)
        r = np.zeros(nz, np.uint8)
        r[64:] = 1                           # the only filled voxels are in the high word
        rows.append(r)
        r = np.zeros(nz, np.uint8)
        r[5] = 1
        r[min(nz - 1, 70)] = 1               # z = 40 .. 63: the nearest filled voxel is in the high word, a farther one in the low word
        rows.append(r)
        r = np.zeros(nz, np.uint8)
        r[60] = 1
        r[nz - 1] = 1                        # z = 64 ..: the nearest filled voxel may be in the low word
        rows.append(r)
    rows += [1 - r for r in rows]
    return np.stack(rows)


@pytest.mark.parametrize("nz", [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128])
def test_z_rows_at_the_word_edges_and_across_the_two_words(rz, nz):
    rows = _z_rows(nz)
    B = len(rows)
    res = np.array([RES[b % 6] for b in range(B)])
    for vb in (False, True):
        # each grid is one row: the z pass alone decides
        got, ext = _check(rz, rows.reshape(B, 1, 1, nz), res, vb)
        if not vb and nz > 64:
            r = rows[len(rows) // 2 - 2]                      # filled at 5 and 70 (or nz - 1)
            far = min(nz - 1, 70)
            b = len(rows) // 2 - 2
            assert got[b, 0, 0, 50] == np.float32(float(far - 50) * res[b]) and r[5] == 1 and r[far] == 1
        # the row inside a grid: the y and x passes carry its values on
        masks = np.zeros((B, 2, 3, nz), np.uint8)
        masks[:, 1, 2, :] = rows
        _check(rz, masks, res, vb)
        masks = np.ones((B, 2, 3, nz), np.uint8)
        masks[:, 0, 1, :] = rows
        _check(rz, masks, 0.25, vb, single=False)


# ---- x tiles -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 8, 16), (3, 3, 43), (3, 5, 51), (5, 16, 24), (5, 7, 55), (5, 17, 15), (128, 1, 1), (128, 3, 43)],
                         ids=lambda s: "x".join(map(str, s)))
def test_x_tiles_whose_last_tile_is_full_one_column_or_one_short(rz, shape):
    plane = shape[1] * shape[2]
    assert plane % 128 in (0, 1, 127) or shape == (128, 1, 1)
    first, last = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    first[0, 0, 0] = 1
    last[shape[0] - 1, shape[1] - 1, shape[2] - 1] = 1                    # the last column of the last tile
    col = np.zeros(shape, np.uint8)
    col[:, shape[1] - 1, shape[2] - 1] = 1
    col[shape[0] // 2, shape[1] - 1, shape[2] - 1] = 0
    masks = np.stack([last, first, 1 - last, 1 - first, col, 1 - col])
    for vb in (False, True):
        _check(rz, masks, np.array([RES[b % 6] for b in range(6)]), vb)


# ---- the int16 plane field -----------------------------------------------------------------------------------------------------------
def test_the_largest_in_plane_distance_beside_the_sentinel_at_128_cubed(rz):
    n = 128
    a = np.zeros((n, n, n), np.uint8)
    a[0, 0, 0] = 1                         # its x = 0 plane holds d^2 up to 2 * 127^2 = 32258; every other plane holds the sentinel
    c = np.zeros((n, n, n), np.uint8)
    c[n - 1, 0, n - 1] = 1
    masks = np.stack([a, 1 - a, c])
    res = np.array([1.0, 0.037, 0.25])
    got, ext = _check(rz, masks, res, False)
    assert got[0, 127, 127, 127] == np.float32(np.sqrt(3.0 * 127 * 127) * 1.0) and ext[0][0] == np.sqrt(3.0 * 127 * 127)
    assert got[1, 127, 127, 127] == np.float32(-(np.sqrt(3.0 * 127 * 127) * 0.037))
    # the x line through (y, z) = (127, 127): 32258 in the voxel's own plane, the sentinel in every other one
    for x in (0, 1, 64, 127):
        assert got[0, x, 127, 127] == np.float32(np.sqrt(float(32258 + x * x)) * 1.0), x
        assert got[2, 127 - x, 127, 0] == np.float32(np.sqrt(float(32258 + x * x)) * 0.25), x
    _check(rz, masks, res, True, single=False)


def test_an_axis_of_129_takes_the_single_builds_and_still_matches(rz):
    shape = (128, 128, 129)
    a = np.zeros(shape, np.uint8)
    a[0, 0, 0] = 1
    masks = np.stack([a, synth.bernoulli_mask(shape, 0.3, 5)])
    got, ext = _check(rz, masks, np.array([1.0, 0.05]), False, fast=False)
    assert got[0, 127, 127, 128] == np.float32(np.sqrt(2.0 * 127 * 127 + 128.0 * 128))


# ---- structured far-field scenes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 64, 64), (100, 100, 50), (25, 20, 15)], ids=lambda s: "x".join(map(str, s)))
def test_structured_scenes_with_per_grid_resolutions(rz, shape):
    rng = np.random.default_rng(7)
    masks = np.stack([FB.structured(rng, shape), FB.structured(rng, shape), A.nested_shells(shape, 2), A.serpentine(shape),
                      A.comb(shape, 1), A.stripes(shape, 0), A.checkerboard(shape)]).astype(np.uint8)
    res = np.array([RES[b % 6] for b in range(7)])
    for vb in (False, True):
        _check(rz, masks, res, vb)


# ---- the pinned parameter ring ---------------------------------------------------------------------------------------------------------
def _pool(shape, count, seed):
    """`count` distinct masks of a tiny shape (all free, all filled, single voxels, noise) and their oracle fields per resolution"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    masks = [np.zeros(n, np.uint8), np.ones(n, np.uint8)]
    for i in range(n):
        m = np.zeros(n, np.uint8)
        m[i] = 1
        masks += [m, 1 - m]
    while len(masks) < count:
        masks.append((rng.random(n) < rng.random()).astype(np.uint8))
    masks = np.stack(masks[:count]).reshape((count,) + tuple(shape))
    return masks


def _tables(masks, vb):
    """oracle fields [mask][resolution] and extrema [mask][resolution][2]"""
    K = len(masks)
    sdf = np.empty((K, len(RES)) + masks.shape[1:], np.float32)
    ext = np.empty((K, len(RES), 2), np.float64)
    for k in range(K):
        for r, res in enumerate(RES):
            sdf[k, r], e, _ = O.exact_sdf(masks[k], res, vb)
            ext[k, r] = e
    return sdf, ext


def _same_or_nan(a, b):
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def test_70000_grids_grow_the_ring_and_the_gradient_walks_past_65535(fresh):
    """B = 70000 grids of 2 x 3 x 2 with per-grid resolutions: 560 KB of parameters (the ring of this handle of its own still has
    its first 64 KiB, so it must grow), P = 8, and k_batch_gradient's second grid dimension (65535 at most) strides."""
    rz = fresh
    rz.set_option("redzone", 1)
    shape, B = (2, 3, 2), 70000
    n = 12
    rng = np.random.default_rng(3)
    pool = _pool(shape, 64, 1)
    mi, ri = rng.integers(0, 64, B), rng.integers(0, 6, B)
    mi[-1], ri[-1] = 2, 4                                  # (a single voxel in the very last grid)
    masks = pool[mi]
    res = np.asarray(RES)[ri]
    assert B * 8 > 64 << 10 and _planes_per_workgroup(shape, B) == 8
    d_in, d_out = rz.device_malloc(B * n), rz.device_malloc(B * n * 4)
    rz.copy_from_host(d_in, masks)
    for vb in (True, False):
        sdf_t, ext_t = _tables(pool, vb)
        arr = res.copy()
        rz.build_batch_device(d_in, B, shape, d_out, arr, vb, 0)
        arr[:] = -1.0
        assert rz.last_batch_info() == (True, 2)
        ext = np.asarray(rz.get_extrema_batch(B))
        got = rz.copy_to_host(np.empty((B,) + shape, np.float32), d_out)
        want = sdf_t[mi, ri]
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(B, -1).any(axis=1))
        assert bad.size == 0, (vb, bad.size, bad[:5].tolist())
        assert np.array_equal(ext, ext_t[mi, ri]), (vb, np.flatnonzero((ext != ext_t[mi, ri]).any(axis=1))[:5].tolist())
        for k in range(64):                                # the single build per distinct (mask, resolution)
            for r in range(6):
                one, one_ext = rz.build(pool[k], RES[r], vb)
                assert _bits_equal(one, sdf_t[k, r]) and one_ext == tuple(ext_t[k, r])
    # the gradient of the 70000 fields (no border), per-grid resolutions: fp32 and fp64
    for f64, edge in ((False, True), (True, True), (True, False)):
        dt, w = (np.float64, 8) if f64 else (np.float32, 4)
        grad_t = np.empty((64, 6) + shape + (3,), dt)
        for k in range(64):
            for r in range(6):
                grad_t[k, r] = A.grid_gradient(sdf_t[k, r], RES[r], edge).astype(dt)
        d_g = rz.device_malloc(B * n * 3 * w)
        rz.copy_from_host(d_g, np.full(B * n * 3 * w, 0x7B, np.uint8))
        rz.gradient_batch_device(d_out, B, shape, d_g, res.copy(), edge, f64, 0)
        grad = rz.copy_to_host(np.empty((B,) + shape + (3,), dt), d_g)
        rz.device_free(d_g)
        want = grad_t[mi, ri]
        u = np.uint64 if f64 else np.uint32
        ok = ((grad.view(u) == want.view(u)) | (np.isnan(grad) & np.isnan(want))).reshape(B, -1).all(axis=1)
        assert ok.all(), (f64, edge, int((~ok).sum()), np.flatnonzero(~ok)[:5].tolist())
    rz.device_free(d_in)
    rz.device_free(d_out)


@pytest.mark.parametrize("redzone", [0, 1], ids=["asynchronous", "redzones"])
def test_300_calls_wrap_the_ring_twice(fresh, redzone):
    """300 build_batch_device calls of B = 64 back to back on one stream, every call with its own resolutions and its own slice
    of the output, no host wait in between (red zones off; with them on, every call ends with a check and a synchronisation).
    The ring only ever grows, so this runs on a handle of its own, whose ring is the first 64 KiB: 512 B of parameters a call,
    128 calls a lap, two wraps into slots whose copies may still be in flight."""
    import torch
    gpu = fresh
    gpu.set_option("redzone", redzone)
    try:
        shape, B, calls = (3, 4, 5), 64, 300
        n = 60
        assert B * 8 == 512 and calls * 512 > 2 * (64 << 10)
        pool = _pool(shape, B, 2)
        sdf_t, ext_t = _tables(pool, False)
        rng = np.random.default_rng(9)
        ri = rng.integers(0, 6, (calls, B))
        stream = torch.cuda.Stream()
        d_in, d_out = gpu.device_malloc(B * n), gpu.device_malloc(calls * B * n * 4)
        gpu.copy_from_host(d_in, pool)
        torch.cuda.synchronize()
        for c in range(calls):
            arr = np.asarray(RES)[ri[c]]
            gpu.build_batch_device(d_in, B, shape, d_out + c * B * n * 4, arr, False, stream.cuda_stream)
            arr[:] = -1.0
        ext = np.asarray(gpu.get_extrema_batch(B))
        assert np.array_equal(ext, ext_t[np.arange(B), ri[-1]])
        got = gpu.copy_to_host(np.empty((calls, B) + shape, np.float32), d_out)
        want = sdf_t[np.arange(B)[None, :], ri]
        bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)).reshape(calls, B, -1).any(axis=2))
        assert len(bad) == 0, (len(bad), bad[:5].tolist())
        for k in range(B):                                 # the single build per distinct (mask, resolution)
            for r in range(6):
                one, one_ext = gpu.build(pool[k], RES[r], False)
                assert _bits_equal(one, sdf_t[k, r]) and one_ext == tuple(ext_t[k, r])
        gpu.device_free(d_in)
        gpu.device_free(d_out)
    finally:
        gpu.set_option("redzone", 0)


# ---- streams ---------------------------------------------------------------------------------------------------------------------------
def test_batches_single_builds_and_gradients_on_two_streams(rz):
    import torch
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    shape_a, shape_b, shape_1 = (25, 20, 15), (40, 40, 40), (33, 17, 96)
    ma, mb = _mixed(shape_a, 7, 21), _mixed(shape_b, 5, 22)
    m1 = synth.bernoulli_mask(shape_1, 0.1, 23)
    res_a, res_b = np.array([RES[b % 6] for b in range(7)]), np.array([RES[(b + 2) % 6] for b in range(5)])
    na, nb, n1 = int(np.prod(shape_a)), int(np.prod(shape_b)), int(np.prod(shape_1))
    d = {k: rz.device_malloc(v) for k, v in (("ia", 7 * na), ("oa", 7 * na * 4), ("ib", 5 * nb), ("ob", 5 * nb * 4), ("i1", n1), ("o1", n1 * 4),
                                             ("ga", 7 * na * 3 * 8))}
    rz.copy_from_host(d["ia"], ma)
    rz.copy_from_host(d["ib"], mb)
    rz.copy_from_host(d["i1"], m1)
    torch.cuda.synchronize()
    rz.build_batch_device(d["ia"], 7, shape_a, d["oa"], res_a.copy(), False, sa.cuda_stream)
    rz.build_device(d["i1"], shape_1, d["o1"], 0.05, True, sb.cuda_stream)
    rz.build_batch_device(d["ib"], 5, shape_b, d["ob"], res_b.copy(), True, sb.cuda_stream)
    rz.gradient_batch_device(d["oa"], 7, shape_a, d["ga"], res_a.copy(), True, True, sa.cuda_stream)
    ext_b = rz.get_extrema_batch(5)
    ext_1 = rz.get_extrema()
    torch.cuda.synchronize()
    got_a = rz.copy_to_host(np.empty(ma.shape, np.float32), d["oa"])
    got_b = rz.copy_to_host(np.empty(mb.shape, np.float32), d["ob"])
    got_1 = rz.copy_to_host(np.empty(shape_1, np.float32), d["o1"])
    grad = rz.copy_to_host(np.empty(ma.shape + (3,), np.float64), d["ga"])
    want_1, want_1_ext, _ = O.exact_sdf(m1, 0.05, True)
    assert _bits_equal(got_1, want_1) and ext_1 == tuple(float(v) for v in want_1_ext)
    for b in range(7):
        want = O.exact_sdf(ma[b], res_a[b], False)[0]
        assert _bits_equal(got_a[b], want), b
        assert _same_or_nan(grad[b], A.grid_gradient(want, res_a[b], True)), b
    for b in range(5):
        want, want_ext, _ = O.exact_sdf(mb[b], res_b[b], True)
        assert _bits_equal(got_b[b], want) and ext_b[b] == tuple(float(v) for v in want_ext), b
    for p in d.values():
        rz.device_free(p)


# ---- tagged objects --------------------------------------------------------------------------------------------------------------------
def test_tagged_objects_id_zero_wide_records_and_the_per_grid_path(rz):
    rng = np.random.default_rng(17)
    for shape, fast in (((12, 10, 9), True), ((6, 5, 130), False)):
        n = int(np.prod(shape))
        occ = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=shape, p=[0.5, 0.1, 0.4])
        obj = rng.choice(np.array([0, 1, 2, 9], np.uint32), size=shape)
        ids = [9, 0, 4, 1, 0, 2]                                 # id 0 twice, 4 absent
        for stride, occ_off, obj_off in ((16, 0, 8), (24, 4, 16), (24, 8, 20)):
            raw = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
            raw[:, occ_off:occ_off + 4] = occ.reshape(-1).view(np.uint8).reshape(n, 4)
            raw[:, obj_off:obj_off + 4] = obj.reshape(-1).view(np.uint8).reshape(n, 4)
            for unknown in (False, True):
                kw = dict(unknown_is_filled=unknown, resolution=0.037, add_virtual_border=unknown, cell_stride=stride, occupancy_offset=occ_off,
                          object_id_offset=obj_off)
                got, ext = rz.build_tagged_objects(raw, shape, ids, **kw)
                assert rz.last_batch_info() == ((True, 2) if fast else (False, -1))
                filled = (occ > 0.5) | (unknown & (occ == 0.5))
                for b, i in enumerate(ids):
                    want, want_ext, _ = O.exact_sdf((filled & (obj == i)).astype(np.uint8), 0.037, unknown)
                    assert _bits_equal(got[b], want) and ext[b] == tuple(float(v) for v in want_ext), (shape, stride, unknown, i)
                    # single tagged builds between the ids of the per-grid path
                    one, one_ext = rz.build_tagged_cells(raw, shape, object_mode=2, object_ids=[i], **kw)
                    assert _bits_equal(got[b], one) and ext[b] == one_ext, (shape, stride, unknown, i)
                again, ext2 = rz.build_tagged_objects(None, shape, ids[::-1], **kw)
                assert _bits_equal(again, got[::-1]) and ext2 == ext[::-1]


# ---- the red-zone switch ---------------------------------------------------------------------------------------------------------------
def test_switching_red_zones_on_releases_the_batch_scratch(fresh):
    """A handle that built a batch before set_option("redzone", 1) must not keep the batch's scratch without canaries: the switch
    releases it (the device's free memory rises by the plane field at least), sdfgpu_get_extrema_batch asks for a new batch
    build, and the next batch, on scratch with zones, is right and leaves every canary alone."""
    import torch
    shape, B = (64, 64, 64), 64
    n = 64 ** 3
    masks = np.stack([synth.bernoulli_mask(shape, (0.5, 0.01)[b % 2], 40 + b) for b in range(B)])
    d_in, d_out = fresh.device_malloc(B * n), fresh.device_malloc(B * n * 4)
    fresh.copy_from_host(d_in, masks)
    res = np.array([RES[b % 6] for b in range(B)])
    fresh.build_batch_device(d_in, B, shape, d_out, res.copy(), False, 0)
    before = fresh.get_extrema_batch(B)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    fresh.set_option("redzone", 1)
    assert torch.cuda.mem_get_info()[0] - free0 >= B * n * 2 - (4 << 20)          # the int16 plane field (32 MiB) went
    with pytest.raises(capi.SdfGpuError) as e:
        fresh.get_extrema_batch(B)
    assert e.value.code == -1
    fresh.build_batch_device(d_in, B, shape, d_out, res.copy(), False, 0)
    assert fresh.get_extrema_batch(B) == before
    fresh.redzone_check()
    got = fresh.copy_to_host(np.empty(masks.shape, np.float32), d_out)
    for b in (0, 1, B - 1):
        want, want_ext, _ = O.exact_sdf(masks[b], res[b], False)
        assert _bits_equal(got[b], want) and before[b] == tuple(float(v) for v in want_ext)
    fresh.device_free(d_in)
    fresh.device_free(d_out)


# ---- the documented batch limit ----------------------------------------------------------------------------------------------------------
def test_131073_grids_of_1x128x128_launch_2_to_the_32_threads(rz):
    """include/sdfgpu.h accepts batches up to 2^24.  k_batch_x_finish takes one 256-thread workgroup per (grid, tile of 128 columns):
    131073 grids of 1 x 128 x 128 are 131073 * 128 * 256 = 2^32 + 32768 threads, more than one grid dimension of a HIP launch takes.
    Measured on an MI355X while that was a one-dimensional launch: no refusal, SDFGPU_OK and wrong fields;
    batch_launch now spreads the workgroups over two grid dimensions, so every field and every extrema pair must be right.
    Device resident (2.1 GB of masks, 8.6 GB of fields, 4.3 GB of plane field); skipped where that much memory is not free."""
    import torch
    shape, B = (1, 128, 128), 131073
    n = 128 * 128
    need = B * n * (1 + 4 + 2) + (3 << 30)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %.1f GB of free device memory, %.1f GB are free" % (need / 1e9, free / 1e9))
    rng = np.random.default_rng(5)
    corner = np.zeros(shape, np.uint8)
    corner[0, 0, 0] = 1
    distinct = np.stack([synth.bernoulli_mask(shape, 0.5, 1), corner, np.zeros(shape, np.uint8), np.ones(shape, np.uint8),
                         FB.structured(rng, shape)])
    period = 30                                                  # 5 masks x 6 resolutions
    res = np.asarray(RES)[np.arange(B) % 6]
    want = np.stack([O.exact_sdf(distinct[k % 5], RES[k % 6], False)[0] for k in range(period)])
    want_ext = [tuple(float(v) for v in O.exact_sdf(distinct[k % 5], RES[k % 6], False)[1]) for k in range(period)]
    for k in range(period):                                      # the single build of each distinct (mask, resolution)
        one, one_ext = rz.build(distinct[k % 5], RES[k % 6], False)
        assert _bits_equal(one, want[k]) and one_ext == want_ext[k]
    d_masks = torch.from_numpy(distinct).cuda()[torch.arange(B, device="cuda") % 5].contiguous()
    d_out = torch.full((B,) + shape, 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rz.build_batch_device(d_masks.data_ptr(), B, shape, d_out.data_ptr(), res.copy(), False, 0)
    assert rz.last_batch_info() == (True, 2)
    ext = rz.get_extrema_batch(B)
    torch.cuda.synchronize()
    d_want = torch.from_numpy(want).cuda().view(torch.int32)
    whole = (B // period) * period
    for lo in range(0, whole, period * 128):
        hi = min(whole, lo + period * 128)
        chunk = d_out[lo:hi].view(torch.int32).view((hi - lo) // period, period, 1, 128, 128)
        assert bool((chunk == d_want[None]).all()), ("grids", lo, hi)
    tail = d_out[whole:].view(torch.int32)
    assert bool((tail == d_want[:B - whole]).all())
    assert _bits_equal(d_out[B - 1].cpu().numpy(), want[(B - 1) % period]) and _bits_equal(d_out[0].cpu().numpy(), want[0])
    assert ext == [want_ext[b % period] for b in range(B)]
    del d_masks, d_out
    torch.cuda.empty_cache()
    small = _mixed((5, 8, 8), 3, 4)                              # the handle goes on working
    _check(rz, small, 0.5, True)
