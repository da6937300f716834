"""GPU: the mesh rasteriser (sdfgpu_rasterize_meshes*, include/sdfgpu.h "Planes and triangle meshes") and the plane of the shape
list bit-equal to the numpy restatement (tests/mesh_raster_restated.py, which tests/test_mesh_raster_cpu.py holds against the exact
judge) through the host form and the device form, on bits, mask and object ids.

Scenes (tests/mesh_cases.py): icosahedra, a box as 12 triangles, a floor of two triangles over a whole layer, a sliver across the
diagonal, a mesh outside, triangles far larger than the grid, zero-area triangles, a tiny triangle, overlapping meshes whose ids do
not ascend; dyadic contact scenes; meshes of 1 .. 1025 triangles; a height field of 131 072 sub-voxel triangles; accumulation onto
the shape rasteriser's output and onto a random field; permuted triangles and meshes; every refusal; a red-zoned handle in this
process and SDFGPU_REDZONE=1 in a child."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_judge as J
import mesh_raster_restated as R
import scene_raster_restated as SR
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu
CASES = MC.cases()
DYADIC = MC.dyadic_cases()
PLANES = dict(MC.plane_cases(), **MC.dyadic_plane_cases())
SENTINEL = 0xA5
GUARD = 64
CORE = ["three-33x9x40-general", "sliver-24x20x17-general", "floor-64x8x64-identity", "huge-24x20x17-general", "segment-24x20x17-identity"]


@pytest.fixture(scope="module", autouse=True)
def _release_cached_device_memory():
    """what this module's torch buffers took from the device goes back when the module is done (a 0.27 GB field among them)"""
    yield
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _want(name):
    meshes, vertices, triangles, origin, res, grid = CASES[name] if name in CASES else DYADIC[name]
    return R.restated(meshes, vertices, triangles, origin, res, grid)


def _upload(a, pad=256):
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = torch.zeros(raw.size + pad, dtype=torch.uint8, device="cuda")
    if raw.size:
        d[:raw.size] = torch.from_numpy(raw.copy()).cuda()
    return d


def _device(ctx, meshes, vertices, triangles, origin, res, grid, bits=True, mask=True, ids=True, check=True, onto=None, stream=None):
    """the device form on torch buffers with GUARD sentinel bytes in front of and behind each output; onto = (bits, mask, ids) numpy:
    accumulate onto them.  Returns (bits, mask, ids, bad)"""
    n = int(np.prod(grid))
    words = (n + 31) // 32
    d_m, d_v, d_t = _upload(np.ascontiguousarray(meshes, capi.MESH_DTYPE)), _upload(np.ascontiguousarray(vertices, np.float64)), \
        _upload(np.ascontiguousarray(triangles, np.uint32))
    sizes = {"bits": words * 4 if bits else 0, "mask": n if mask else 0, "ids": n * 4 if ids else 0}
    bufs = {k: torch.full((v + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    if onto is not None:
        for k, a in zip(("bits", "mask", "ids"), onto):
            if sizes[k]:
                bufs[k][GUARD:GUARD + sizes[k]] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    ptr = {k: bufs[k].data_ptr() + GUARD if v else 0 for k, v in sizes.items()}
    try:
        bad = ctx.rasterize_meshes_device(d_m.data_ptr(), len(meshes), d_v.data_ptr(), len(np.asarray(vertices).reshape(-1, 3)), d_t.data_ptr(),
                                          len(np.asarray(triangles).reshape(-1, 3)), origin, res, grid, ptr["bits"], ptr["mask"], ptr["ids"],
                                          accumulate=onto is not None, check=check,
                                          stream=torch.cuda.current_stream().cuda_stream if stream is None else stream)
    finally:
        torch.cuda.synchronize()
    out = {}
    for k, v in sizes.items():
        host = bufs[k].cpu().numpy()
        assert bool((host[:GUARD] == SENTINEL).all() and (host[GUARD + v:] == SENTINEL).all()), "bytes around %s were written" % k
        out[k] = host[GUARD:GUARD + v].copy()
    if bits and n % 32:
        assert int(out["bits"].view(np.uint32)[-1]) >> (n % 32) == 0, "spare bits of the last word are set"
    return (out["bits"].view(np.uint32) if bits else None, out["mask"].reshape(grid) if mask else None,
            out["ids"].view(np.uint32).reshape(grid) if ids else None, bad)


def _equal(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d differ, first at %s: got %s, want %s" % (what, len(bad), got.size, bad[0].tolist(),
                                                                                   got[tuple(bad[0])], want[tuple(bad[0])]))


def _check_all(ctx, what, meshes, vertices, triangles, origin, res, grid, want, host=True):
    mask, ids, bits = want
    if host:
        got = ctx.rasterize_meshes(meshes, vertices, triangles, origin, res, grid, bits=True, mask=True, object_ids=True)
        _equal(what + " host bits", got["bits"], bits)
        _equal(what + " host mask", got["mask"], mask)
        _equal(what + " host ids", got["object_ids"], ids)
    d_bits, d_mask, d_ids, bad = _device(ctx, meshes, vertices, triangles, origin, res, grid)
    assert bad == -1
    _equal(what + " device bits", d_bits, bits)
    _equal(what + " device mask", d_mask, mask)
    _equal(what + " device ids", d_ids, ids)


@pytest.mark.parametrize("name", list(CASES))
def test_every_scene_through_both_forms(gpu, name):
    meshes, vertices, triangles, origin, res, grid = CASES[name]
    _check_all(gpu, name, meshes, vertices, triangles, origin, res, grid, _want(name))


@pytest.mark.parametrize("name", list(DYADIC))
def test_dyadic_contact_scenes_equal_the_exact_judge(gpu, name):
    meshes, vertices, triangles, origin, res, grid = DYADIC[name]
    _check_all(gpu, name, meshes, vertices, triangles, origin, res, grid, _want(name))
    _, d_mask, _, _ = _device(gpu, meshes, vertices, triangles, origin, res, grid, bits=False, ids=False)
    ratio = J.mesh_ratio(meshes, vertices, triangles, origin, res, grid)
    J.check(d_mask, ratio, ties_only=True)
    assert int((ratio == 0).sum()) > 0


def test_single_outputs_alone(gpu):
    name = "three-33x9x40-general"
    meshes, vertices, triangles, origin, res, grid = CASES[name]
    mask, ids, bits = _want(name)
    _equal("bits alone", _device(gpu, meshes, vertices, triangles, origin, res, grid, mask=False, ids=False, check=False)[0], bits)
    _equal("mask alone", _device(gpu, meshes, vertices, triangles, origin, res, grid, bits=False, ids=False)[1], mask)
    _equal("ids alone", _device(gpu, meshes, vertices, triangles, origin, res, grid, bits=False, mask=False)[2], ids)
    _equal("host bits alone", gpu.rasterize_meshes(meshes, vertices, triangles, origin, res, grid)["bits"], bits)
    assert len(np.unique(ids)) == 4                                            # three objects and the background


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_triangle_counts(gpu, count):
    origin, grid = MC.origins()["general"], MC.GRIDS[1]
    v, t = MC.patch(count, np.asarray(grid) * MC.RES, MC.RES)
    meshes, vertices, triangles = capi.make_meshes([(5, v, t, origin)])
    want = R.restated(meshes, vertices, triangles, origin, MC.RES, grid)
    _check_all(gpu, "%d triangles" % count, meshes, vertices, triangles, origin, MC.RES, grid, want)
    assert bool(want[0].any()) == (count > 0)


def test_a_height_field_of_131072_sub_voxel_triangles(gpu):
    grid, res, origin = MC.GRIDS[2], MC.RES, MC.origins()["translation"]
    ext = np.asarray(grid) * res
    v, t = MC.height_field(256, 256, ext[0], ext[2], lambda x, z: ext[1] * (0.5 + 0.3 * np.sin(3.0 * x / ext[0]) * np.cos(2.0 * z / ext[2])))
    assert len(t) == 131072
    meshes, vertices, triangles = capi.make_meshes([(9, v, t, origin)])
    want = R.restated(meshes, vertices, triangles, origin, res, grid)
    assert 64 * 64 <= int(want[0].sum()) < 4 * 64 * 64
    _check_all(gpu, "height field", meshes, vertices, triangles, origin, res, grid, want, host=False)


def test_many_meshes_some_empty_some_sharing_runs(gpu):
    """40 meshes, every fifth without triangles, two naming the same run of triangles and vertices under different poses"""
    origin, grid, res = MC.origins()["general"], MC.GRIDS[0], MC.RES
    ext = np.asarray(grid) * res
    rng = np.random.default_rng(11)
    items = []
    for i in range(40):
        v, t = MC.icosahedron(float(rng.uniform(0.8, 2.5)) * res)
        if i % 5 == 4:
            t = t[:0]
        items.append((1 + (i * 7) % 13, v, t, origin @ MC._local(rng.normal(size=4), rng.uniform(0.1, 0.9, 3) * ext)))
    meshes, vertices, triangles = capi.make_meshes(items)
    meshes = meshes.copy()
    meshes[4]["first_triangle"], meshes[4]["n_triangles"] = meshes[0]["first_triangle"], 10          # the empty slot's share: 8 x 20 unused
    meshes[4]["first_vertex"], meshes[4]["n_vertices"] = meshes[0]["first_vertex"], meshes[0]["n_vertices"]
    meshes[1]["n_triangles"] = 10                                             # (the counts may sum to the array's length, no further)
    assert R.mesh_refusal(meshes, vertices, triangles) is None
    _check_all(gpu, "forty meshes", meshes, vertices, triangles, origin, res, grid, R.restated(meshes, vertices, triangles, origin, res, grid))


def test_the_smallest_id_wins_whatever_the_order(gpu):
    name = "three-24x20x17-general"
    meshes, vertices, triangles, origin, res, grid = CASES[name]
    mask, ids, bits = _want(name)
    a = _device(gpu, meshes, vertices, triangles, origin, res, grid)
    b = _device(gpu, meshes, vertices, triangles, origin, res, grid)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y), "two runs differ"
    rng = np.random.default_rng(3)
    for _ in range(3):
        order = rng.permutation(len(meshes))
        tri = np.asarray(triangles).copy()
        for m in meshes:                                                      # the triangles of every mesh among themselves
            s = slice(int(m["first_triangle"]), int(m["first_triangle"] + m["n_triangles"]))
            tri[s] = tri[s][rng.permutation(int(m["n_triangles"]))][:, rng.permutation(3)]
        got = _device(gpu, meshes[order], vertices, tri, origin, res, grid)
        _equal("permuted ids", got[2], ids)
        _equal("permuted bits", got[0], bits)
    overlap = np.zeros(grid, int)
    for i in range(len(meshes)):
        overlap += R.restated(meshes[i:i + 1], vertices, triangles, origin, res, grid)[0]
    assert (overlap > 1).any(), "the scene has no overlap of distinct ids"


def test_accumulate_onto_the_shape_rasteriser_and_onto_a_random_field(gpu):
    import scene_cases
    name = "three-24x20x17-general"
    meshes, vertices, triangles, origin, res, grid = CASES[name]
    meshes = meshes.copy()
    meshes["object_id"] += 3                                                  # behind the shapes' ids, as SDF_Builder numbers them
    shapes = scene_cases.cases()["three-24x20x17-general"][0]
    base = gpu.rasterize_shapes(shapes, origin, res, grid, bits=True, mask=True, object_ids=True)
    smask, sids, _ = SR.restated(shapes, origin, res, grid)
    _equal("shapes", base["mask"], smask)
    want = R.restated(meshes, vertices, triangles, origin, res, grid, onto=(smask, sids))
    got = _device(gpu, meshes, vertices, triangles, origin, res, grid, onto=(base["bits"], base["mask"], base["object_ids"]))
    _equal("onto shapes: bits", got[0], want[2])
    _equal("onto shapes: mask", got[1], want[0])
    _equal("onto shapes: ids", got[2], want[1])
    assert (want[0] > smask).any() and (smask & R.restated(meshes, vertices, triangles, origin, res, grid)[0]).any()
    # a random field: the OR, and the smallest non-zero id (existing ids both above and below the meshes')
    rng = np.random.default_rng(8)
    rmask = (rng.random(grid) < 0.3).astype(np.uint8)
    rids = np.where(rmask, rng.integers(1, 9, grid), 0).astype(np.uint32)
    want = R.restated(meshes, vertices, triangles, origin, res, grid, onto=(rmask, rids))
    got = _device(gpu, meshes, vertices, triangles, origin, res, grid, onto=(R.pack_bits(rmask), rmask, rids))
    _equal("onto random: bits", got[0], want[2])
    _equal("onto random: mask", got[1], want[0])
    _equal("onto random: ids", got[2], want[1])
    hit = R.restated(meshes, vertices, triangles, origin, res, grid)[0].astype(bool)
    assert (want[1][hit & (rids > 0)] == np.minimum(rids, R.restated(meshes, vertices, triangles, origin, res, grid)[1])[hit & (rids > 0)]).all()
    assert np.array_equal(want[1][~hit], rids[~hit])
    # no meshes at all under accumulate: nothing changes
    none = capi.make_meshes([])
    got = _device(gpu, *none, origin, res, grid, onto=(R.pack_bits(rmask), rmask, rids))
    _equal("nothing onto random", got[2], rids)
    _equal("nothing onto random", got[0], R.pack_bits(rmask))


@pytest.mark.parametrize("seed", range(30))
def test_random_scenes(gpu, seed):
    meshes, vertices, triangles, origin, res, grid = MC.random_scene(seed)
    _check_all(gpu, "random scene %d" % seed, meshes, vertices, triangles, origin, res, grid, R.restated(meshes, vertices, triangles, origin, res, grid))


# ---- planes through the shape rasteriser -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PLANES))
def test_planes_through_the_shape_rasteriser(gpu, name):
    import test_gpu_scene_raster as TS
    shapes, origin, res, grid = PLANES[name]
    TS._check_all(gpu, name, shapes, origin, res, grid, R.restated_shapes(shapes, origin, res, grid))


def test_random_planes_and_refused_planes(gpu):
    import test_gpu_scene_raster as TS
    for seed in range(20):
        shapes, origin, res, grid = MC.random_plane_scene(seed)
        TS._check_all(gpu, "random plane %d" % seed, shapes, origin, res, grid, R.restated_shapes(shapes, origin, res, grid))
    eye, grid = np.eye(4), (6, 5, 4)
    nan_pose = np.eye(4)
    nan_pose[1, 1] = np.nan
    for what, (dims, pose) in {"zero normal": ((0.0, 0.0, 0.0), eye), "NaN normal": ((0.0, np.nan, 1.0), eye), "infinite normal": ((np.inf, 0.0, 0.0), eye),
                               "NaN pose": ((0.0, 0.0, 1.0), nan_pose)}.items():
        shapes = capi.make_shapes([(capi.SHAPE_SPHERE, 2, (0.1,), eye), (capi.SHAPE_PLANE, 1, dims, pose)])
        rc, msg = TS._refused_host(gpu, shapes, eye, 0.1, grid)
        assert rc == -1 and "shape 1 " in msg, (what, rc, msg)
        with pytest.raises(capi.SdfGpuError) as e:
            TS._device(gpu, shapes, eye, 0.1, grid, check=True)
        assert "shape 1 " in str(e.value), what
    ok = capi.make_shapes([(capi.SHAPE_PLANE, 1, (-1.0, -2.0, -0.5), eye)])
    assert TS._refused_host(gpu, ok, eye, 0.1, grid)[0] == 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _host_call(ctx, meshes, vertices, triangles, origin, res, grid, **kw):
    n = int(np.prod(np.maximum(grid, 1)))
    bits = np.full((n + 31) // 32, 0xA5A5A5A5, np.uint32)
    mask = np.full(n, SENTINEL, np.uint8)
    ids = np.full(n, 0xA5A5A5A5, np.uint32)
    m = np.ascontiguousarray(meshes, capi.MESH_DTYPE)
    v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    o = (ctypes.c_double * 16)(*np.asarray(origin, np.float64).reshape(-1))
    rc = ctx._lib.sdfgpu_rasterize_meshes(ctx._h, m.ctypes.data + kw.get("mesh_off", 0), kw.get("n_meshes", m.size), v.ctypes.data + kw.get("vertex_off", 0),
                                          kw.get("n_vertices", len(v)), t.ctypes.data + kw.get("triangle_off", 0), kw.get("n_triangles", len(t)), o,
                                          float(res), *[int(x) for x in grid], bits.ctypes.data + kw.get("bits_off", 0) if kw.get("bits", True) else None,
                                          mask.ctypes.data if kw.get("mask", True) else None,
                                          ids.ctypes.data + kw.get("ids_off", 0) if kw.get("ids", True) else None)
    untouched = bool((bits == 0xA5A5A5A5).all() and (mask == SENTINEL).all() and (ids == 0xA5A5A5A5).all())
    assert untouched == (rc != 0), "a refused call wrote to its outputs" if rc else "an accepted call wrote nothing"
    return rc, ctx._lib.sdfgpu_last_error(ctx._h).decode()


def test_every_host_refusal_leaves_the_outputs_untouched(gpu):
    import test_mesh_raster_cpu as TC
    grid, eye = (6, 5, 4), np.eye(4)
    for what, (meshes, vertices, triangles, with_ids, without) in TC.refusals().items():
        rc, msg = _host_call(gpu, meshes, vertices, triangles, eye, 0.1, grid)
        assert (rc, ("mesh %d " % with_ids) in msg) == (-1, True) if with_ids is not None else rc == 0, (what, rc, msg)
        rc, msg = _host_call(gpu, meshes, vertices, triangles, eye, 0.1, grid, ids=False)
        assert (rc, ("mesh %d " % without) in msg) == (-1, True) if without is not None else rc == 0, (what, rc, msg)
    good = capi.make_meshes([(1, *MC.icosahedron(0.2), eye)])
    inf_origin = np.eye(4)
    inf_origin[0, 3] = np.inf
    for what, (args, kw) in {"resolution 0": ((eye, 0.0, grid), {}), "a negative resolution": ((eye, -0.1, grid), {}), "a NaN resolution": ((eye, np.nan, grid), {}),
                             "an infinite resolution": ((eye, np.inf, grid), {}), "a zero dimension": ((eye, 0.1, (6, 0, 4)), {}),
                             "a negative dimension": ((eye, 0.1, (-6, 5, 4)), {}), "an infinite origin": ((inf_origin, 0.1, grid), {}),
                             "no output": ((eye, 0.1, grid), dict(bits=False, mask=False, ids=False)), "negative meshes": ((eye, 0.1, grid), dict(n_meshes=-1)),
                             "too many meshes": ((eye, 0.1, grid), dict(n_meshes=capi.MAX_MESHES + 1)),
                             "too many triangles": ((eye, 0.1, grid), dict(n_triangles=capi.MAX_TRIANGLES + 1)),
                             "negative triangles": ((eye, 0.1, grid), dict(n_triangles=-1)), "negative vertices": ((eye, 0.1, grid), dict(n_vertices=-1)),
                             "misaligned meshes": ((eye, 0.1, grid), dict(mesh_off=4)), "misaligned vertices": ((eye, 0.1, grid), dict(vertex_off=4)),
                             "misaligned triangles": ((eye, 0.1, grid), dict(triangle_off=2)), "misaligned bits": ((eye, 0.1, grid), dict(bits_off=2)),
                             "misaligned ids": ((eye, 0.1, grid), dict(ids_off=1))}.items():
        rc, msg = _host_call(gpu, *good, *args, **kw)
        assert rc == -1 and msg, (what, rc, msg)
        assert ("resolution" in msg) == ("resolution" in what), (what, msg)
        if "too many" in what:
            assert "limit" in msg
    assert _host_call(gpu, *good, eye, 0.1, grid)[0] == 0


def test_device_form_refusals_write_nothing(gpu):
    grid, eye = (6, 5, 4), np.eye(4)
    meshes, vertices, triangles = capi.make_meshes([(1, *MC.icosahedron(0.2), eye)])
    d_m, d_v, d_t = _upload(meshes), _upload(vertices), _upload(triangles)
    out = torch.full((2048,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = out.data_ptr()
    base = dict(d_meshes=d_m.data_ptr(), n_meshes=1, d_vertices=d_v.data_ptr(), n_vertices=len(vertices), d_triangles=d_t.data_ptr(),
                n_triangles=len(triangles), origin=eye, resolution=0.1, shape=grid, d_bits=p)
    for what, change in {"misaligned meshes": dict(d_meshes=d_m.data_ptr() + 4), "misaligned vertices": dict(d_vertices=d_v.data_ptr() + 4),
                         "misaligned triangles": dict(d_triangles=d_t.data_ptr() + 2), "misaligned bits": dict(d_bits=p + 2),
                         "misaligned ids": dict(d_object_ids=p + 1025), "no output": dict(d_bits=0), "null meshes": dict(d_meshes=0),
                         "null vertices": dict(d_vertices=0), "null triangles": dict(d_triangles=0), "too many meshes": dict(n_meshes=capi.MAX_MESHES + 1),
                         "too many triangles": dict(n_triangles=capi.MAX_TRIANGLES + 1), "negative triangles": dict(n_triangles=-1),
                         "a NaN resolution": dict(resolution=np.nan), "resolution 0": dict(resolution=0.0), "a zero dimension": dict(shape=(6, 0, 4))}.items():
        for accumulate in (False, True):
            with pytest.raises(capi.SdfGpuError) as e:
                gpu.rasterize_meshes_device(**dict(base, **change), accumulate=accumulate, check=True)
            assert e.value.code == -1, what
    with pytest.raises(capi.SdfGpuError):
        gpu._check(gpu._lib.sdfgpu_rasterize_meshes_device(gpu._h, d_m.data_ptr(), 1, d_v.data_ptr(), len(vertices), d_t.data_ptr(), len(triangles),
                                                           (ctypes.c_double * 16)(*eye.reshape(-1)), 0.1, 6, 5, 4, p, None, None, 2, None, None))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_a_mesh_refused_on_the_device_is_reported_and_nothing_is_scattered(gpu):
    import test_mesh_raster_cpu as TC
    origin, res, grid = np.eye(4), 0.1, (6, 5, 4)
    rng = np.random.default_rng(2)
    rmask = (rng.random(grid) < 0.3).astype(np.uint8)
    rids = np.where(rmask, rng.integers(1, 9, grid), 0).astype(np.uint32)
    for what, (meshes, vertices, triangles, with_ids, without) in TC.refusals().items():
        for ids, index in ((True, with_ids), (False, without)):
            if index is None:
                assert _device(gpu, meshes, vertices, triangles, origin, res, grid, ids=ids)[3] == -1, what
                continue
            with pytest.raises(capi.SdfGpuError) as e:
                _device(gpu, meshes, vertices, triangles, origin, res, grid, ids=ids, check=True)
            assert e.value.code == -1 and "mesh %d " % index in str(e.value), (what, str(e.value))
            d_bits, d_mask, d_ids, _ = _device(gpu, meshes, vertices, triangles, origin, res, grid, ids=ids, check=False)
            assert not d_bits.any() and not d_mask.any() and (d_ids is None or not d_ids.any()), what      # cleared
            d_bits, d_mask, d_ids, _ = _device(gpu, meshes, vertices, triangles, origin, res, grid, ids=ids, check=False,
                                               onto=(R.pack_bits(rmask), rmask, rids))
            assert np.array_equal(d_bits, R.pack_bits(rmask)) and np.array_equal(d_mask, rmask) and (d_ids is None or np.array_equal(d_ids, rids)), what
    meshes, vertices, triangles, origin, res, grid = CASES["three-24x20x17-general"]
    two = meshes.copy()
    two[1]["pose"][5], two[2]["object_id"] = np.nan, 0
    with pytest.raises(capi.SdfGpuError) as e:
        _device(gpu, two, vertices, triangles, origin, res, grid, check=True)
    assert "mesh 1 " in str(e.value)                                           # the lowest index
    _equal("the next call", _device(gpu, meshes, vertices, triangles, origin, res, grid)[1], _want("three-24x20x17-general")[0])


# ---- red zones -------------------------------------------------------------------------------------------------------------------------
def core_cases_on(ctx):
    for name in CORE:
        meshes, vertices, triangles, origin, res, grid = CASES[name]
        _check_all(ctx, name + " (red zones)", meshes, vertices, triangles, origin, res, grid, _want(name))
    v, t = MC.patch(1025, np.asarray(MC.GRIDS[2]) * MC.RES, MC.RES)
    meshes, vertices, triangles = capi.make_meshes([(5, v, t, np.eye(4))])
    _check_all(ctx, "1025 triangles (red zones)", meshes, vertices, triangles, np.eye(4), MC.RES, MC.GRIDS[2],
               R.restated(meshes, vertices, triangles, np.eye(4), MC.RES, MC.GRIDS[2]))
    import test_gpu_scene_raster as TS
    shapes, origin, res, grid = PLANES["plane-and-box-24x20x17-general"]
    TS._check_all(ctx, "plane (red zones)", shapes, origin, res, grid, R.restated_shapes(shapes, origin, res, grid))


def test_on_a_red_zoned_handle():
    ctx = capi.SdfGpu(0)
    try:
        ctx.set_option("redzone", 1)
        core_cases_on(ctx)
    finally:
        ctx.close()


def test_the_core_cases_in_a_child_process_with_red_zones_from_the_environment():
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from sdf_tools_amd import capi\nimport test_gpu_mesh_raster as T\n"
            "ctx = capi.SdfGpu(0)\nT.core_cases_on(ctx)\nctx.redzone_check()\nctx.close()\nprint('core cases clean')\n") % (tests, os.path.dirname(tests))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SDFGPU_REDZONE="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "core cases clean" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
