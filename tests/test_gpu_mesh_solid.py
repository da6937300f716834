"""GPU: sdfgpu_rasterize_solid_meshes[_device] against the numpy restatement (mesh_solid_restated.py), bit for bit in bits, mask and ids.

  - every scene of mesh_solid_cases.py through both forms; the centre voxel of a closed cube is filled
  - grids chosen as the smallest at which each mechanism can break (mesh_solid_cases.GRIDS): 1 x 1 x 1 (every index 0); 3 x 2 x 1
    (nz = 1: six columns in one word of the field); 5 x 4 x 33 (one bit in a second word: the word carry, a full lane group of 2, a
    spill word); 7 x 6 x 67 (an odd nz: columns start at every bit offset; a lane group with an idle lane); 17 x 33 x 40 (the edges of
    the 16 x 16 column tiles); 16 x 16 x 2100 (more than 64 words per column: the chunk carry, always 1 there)
  - mesh_solid_cases.stack_scene on 12 x 6 x nz for nz = 32 .. 4128: every lane-group size of the merge (1 .. 64), exactly full and one
    word over; nz % 32 == 0 (no tail mask, no shift, no spill word) and not; one, two and three chunks, the last a single word; at
    every boundary a column whose parity is 1 across it and one whose parity is 0 after earlier toggles; a column that is inside
    where it ends.  test_mesh_solid_cpu.py shows on a word-level model that each of these grids tells a merge without its word
    carry, chunk carry, tail mask, spill word or word before a chunk from the truth, wherever that step can act
  - mesh_solid_cases.slot_scene: 1328 triangles in one call -- slots past a scan block of 1024, empty meshes beside others, meshes
    and slots with zero column tiles between slots with some, 25 tiles in a slot (chunks of 16 end inside it), unused trailing
    triangles, two records on one triangle run -- also shuffled; two stack grids back to back on one handle (another row length)
  - shuffled triangle and mesh order; accumulate 0 and 1 onto a pre-filled field; refusals; the toggle field zero after every call
    (two scenes back to back on one handle against fresh handles); a non-blocking side stream with late inputs; red zones
  - a generic-pose box as 12 solid triangles equals the same box as SDFGPU_SHAPE_BOX; the surface call's bits are a subset"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_judge as J
import mesh_raster_restated as R
import mesh_solid_cases as SC
import mesh_solid_restated as S
import scene_judge
import scene_raster_restated as SR
import stream_harness as H
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu
CASES = SC.cases()
DYADIC = SC.dyadic_cases()
SENTINEL, GUARD = 0xA5, 64
GRIDS = SC.GRIDS                                                               # (mesh_solid_cases.py says which mechanism each is the smallest for)
STACK_IDS = ["x".join(map(str, g)) for g in SC.STACK_GRIDS]


@pytest.fixture(scope="module", autouse=True)
def _release_cached_device_memory():
    yield
    torch.cuda.empty_cache()


def _upload(a, pad=256):
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = torch.zeros(raw.size + pad, dtype=torch.uint8, device="cuda")
    if raw.size:
        d[:raw.size] = torch.from_numpy(raw.copy()).cuda()
    return d


def _device(ctx, meshes, vertices, triangles, origin, res, grid, bits=True, mask=True, ids=True, check=True, onto=None, solid=True):
    """the device form on torch buffers with GUARD sentinel bytes around each output; onto = (bits, mask, ids): accumulate onto them.
    Returns (bits, mask, ids, bad)"""
    n = int(np.prod(grid))
    d_m, d_v, d_t = _upload(np.ascontiguousarray(meshes, capi.MESH_DTYPE)), _upload(np.ascontiguousarray(vertices, np.float64)), \
        _upload(np.ascontiguousarray(triangles, np.uint32))
    sizes = {"bits": (n + 31) // 32 * 4 if bits else 0, "mask": n if mask else 0, "ids": n * 4 if ids else 0}
    bufs = {k: torch.full((v + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    if onto is not None:
        for k, a in zip(("bits", "mask", "ids"), onto):
            if sizes[k]:
                bufs[k][GUARD:GUARD + sizes[k]] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    ptr = {k: bufs[k].data_ptr() + GUARD if v else 0 for k, v in sizes.items()}
    call = ctx.rasterize_solid_meshes_device if solid else ctx.rasterize_meshes_device
    try:
        bad = call(d_m.data_ptr(), len(meshes), d_v.data_ptr(), len(np.asarray(vertices).reshape(-1, 3)), d_t.data_ptr(),
                   len(np.asarray(triangles).reshape(-1, 3)), origin, res, grid, ptr["bits"], ptr["mask"], ptr["ids"],
                   accumulate=onto is not None, check=check, stream=torch.cuda.current_stream().cuda_stream)
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


def _check_all(ctx, what, scene, want, host=True):
    mask, ids, bits = want
    if host:
        got = ctx.rasterize_solid_meshes(*scene, bits=True, mask=True, object_ids=True)
        _equal(what + " host bits", got["bits"], bits)
        _equal(what + " host mask", got["mask"], mask)
        _equal(what + " host ids", got["object_ids"], ids)
    d_bits, d_mask, d_ids, bad = _device(ctx, *scene)
    assert bad == -1
    _equal(what + " device bits", d_bits, bits)
    _equal(what + " device mask", d_mask, mask)
    _equal(what + " device ids", d_ids, ids)
    only_bits, _, _, _ = _device(ctx, *scene, mask=False, ids=False, check=False)
    _equal(what + " device bits alone", only_bits, bits)


@functools.lru_cache(maxsize=None)
def _want(name):
    return S.restated(*(CASES.get(name) or DYADIC[name]))


grid_scene = SC.grid_scene                                                     # (shared with test_mesh_solid_cpu.py, which puts the word model on it)


# ---- scenes and grids ------------------------------------------------------------------------------------------------------------------
def test_the_centre_voxel_of_a_closed_cube_is_filled(gpu):
    v, t = SC.box_triangles((0.75, 0.75, 0.75))                                # dyadic: the faces pass through the centres of cells 2 and 8
    pose = np.eye(4)
    pose[:3, 3] = 0.6875
    meshes, vertices, triangles = capi.make_meshes([(7, v, t, pose)])
    got = gpu.rasterize_solid_meshes(meshes, vertices, triangles, np.eye(4), 0.125, (11, 11, 11), bits=False, mask=True, object_ids=True)
    surface = gpu.rasterize_meshes(meshes, vertices, triangles, np.eye(4), 0.125, (11, 11, 11), bits=False, mask=True)
    assert got["mask"][5, 5, 5] == 1 and got["object_ids"][5, 5, 5] == 7 and surface["mask"][5, 5, 5] == 0
    assert int(got["mask"].sum()) == 7 ** 3 and got["mask"][2:9, 2:9, 2:9].all()


@pytest.mark.parametrize("name", list(CASES) + list(DYADIC))
def test_every_scene_through_both_forms(gpu, name):
    _check_all(gpu, name, CASES.get(name) or DYADIC[name], _want(name))


@pytest.mark.parametrize("grid", GRIDS, ids=["x".join(map(str, g)) for g in GRIDS])
def test_grids_at_which_a_mechanism_can_break(gpu, grid):
    scene = grid_scene(grid)
    want = S.restated(*scene)
    surface = R.restated(*scene)[0]
    if min(grid) > 1:
        assert int(want[0].sum()) > int(surface.sum()), "no interior cell"
    _check_all(gpu, "grid %s" % (grid,), scene, want, host=grid != GRIDS[-1])
    d_bits, _, _, _ = _device(gpu, *scene, mask=False, ids=False, solid=False)
    assert not (d_bits & ~want[2]).any(), "the surface call's bits are a subset of the solid call's"


@functools.lru_cache(maxsize=None)
def _want_stack(grid):
    return S.restated(*SC.stack_scene(grid))


@functools.lru_cache(maxsize=None)
def _want_slot(variant):
    return S.restated(*SC.slot_scene(variant))


@pytest.mark.parametrize("grid", SC.STACK_GRIDS, ids=STACK_IDS)
def test_the_stack_scene_at_every_lane_group_word_and_chunk_boundary(gpu, grid):
    """test_mesh_solid_cpu.py shows that a merge without its word carry, chunk carry, tail mask, spill word or word before a chunk
    gives other bits than these on every grid on which that step can act"""
    _check_all(gpu, "stack %s" % (grid,), SC.stack_scene(grid), _want_stack(grid), host=grid[2] <= 1030)


@pytest.mark.parametrize("variant", SC.SLOT_VARIANTS)
def test_the_slot_scene_against_the_work_distribution(gpu, variant):
    _check_all(gpu, "slots (%s)" % variant, SC.slot_scene(variant), _want_slot(variant))


def _shuffled(scene, rng):
    """the records in another order, every mesh's triangle rows in another order"""
    meshes, vertices, triangles = scene[:3]
    items = []
    for m in meshes[rng.permutation(len(meshes))]:
        ft, nt, fv, nv = (int(m[k]) for k in ("first_triangle", "n_triangles", "first_vertex", "n_vertices"))
        items.append((int(m["object_id"]), vertices[fv:fv + nv], triangles[ft:ft + nt][rng.permutation(nt)], np.asarray(m["pose"]).reshape(4, 4)))
    return capi.make_meshes(items) + scene[3:]


def test_the_slot_scene_with_mesh_and_triangle_order_shuffled(gpu):
    scene = SC.slot_scene("trailing")
    rng = np.random.default_rng(6)
    for _ in range(2):
        other = _shuffled(scene, rng)
        assert [int(m["n_triangles"]) for m in other[0]] != [int(m["n_triangles"]) for m in scene[0]]
        d_bits, d_mask, d_ids, _ = _device(gpu, *other)
        mask, ids, bits = _want_slot("trailing")
        _equal("shuffled slots bits", d_bits, bits)
        _equal("shuffled slots mask", d_mask, mask)
        _equal("shuffled slots ids", d_ids, ids)


def test_two_stack_grids_back_to_back_reuse_the_toggle_field_with_another_row_length():
    """one handle, grids of wz = 66, 3, 17 and 66 again: the toggle field is kept, laid out anew per call, and must be all zero whatever
    the row length of the call before; each result against a fresh handle's and against the restatement"""
    grids = [(12, 6, 2081), (12, 6, 96), (12, 6, 530)]
    fresh = []
    for grid in grids:
        ctx = capi.SdfGpu(0)
        fresh.append(_device(ctx, *SC.stack_scene(grid)))
        ctx.close()
    ctx = capi.SdfGpu(0)
    try:
        for k in (0, 1, 2, 0, 2, 1):
            got = _device(ctx, *SC.stack_scene(grids[k]))
            for j, what in enumerate(("bits", "mask", "ids")):
                _equal("%s after another grid: %s" % (grids[k], what), got[j], fresh[k][j])
            _equal("%s bits" % (grids[k],), got[0], _want_stack(grids[k])[2])
    finally:
        ctx.close()


def test_triangle_and_mesh_order_play_no_part(gpu):
    scene = CASES["two-overlapping"]
    meshes, vertices, triangles = scene[:3]
    rng = np.random.default_rng(3)
    items = []
    for m in meshes[::-1]:
        ft, nt, fv, nv = (int(m[k]) for k in ("first_triangle", "n_triangles", "first_vertex", "n_vertices"))
        items.append((int(m["object_id"]), vertices[fv:fv + nv], triangles[ft:ft + nt][rng.permutation(nt)], np.asarray(m["pose"]).reshape(4, 4)))
    shuffled = capi.make_meshes(items) + scene[3:]
    a, b = _device(gpu, *scene), _device(gpu, *shuffled)
    for k, what in enumerate(("bits", "mask", "ids")):
        _equal("shuffled " + what, b[k], a[k])
    _equal("ids", a[2], _want("two-overlapping")[1])


def test_accumulate_onto_a_prefilled_field(gpu):
    scene = CASES["two-overlapping"]                                            # ids 3 and 2
    grid = scene[5]
    rng = np.random.default_rng(4)
    rmask = (rng.random(grid) < 0.3).astype(np.uint8)
    rids = np.where(rmask, rng.integers(1, 6, grid), 0).astype(np.uint32)      # some below, some above the meshes' ids
    mask, ids, bits = S.restated(*scene, onto=(rmask, rids))
    d_bits, d_mask, d_ids, bad = _device(gpu, *scene, onto=(R.pack_bits(rmask), rmask, rids))
    assert bad == -1
    _equal("accumulated bits", d_bits, bits)
    _equal("accumulated mask", d_mask, mask)
    _equal("accumulated ids", d_ids, ids)
    assert ((ids == rids) & (rids != 0) & (_want("two-overlapping")[1] > rids)).any(), "an id already there that is the smallest"
    assert ((ids != rids) & (rids != 0)).any(), "an id already there that is not"
    # accumulate == 0 clears first
    d_bits, d_mask, d_ids, _ = _device(gpu, *scene)
    _equal("cleared ids", d_ids, _want("two-overlapping")[1])


def test_refusals_leave_the_outputs_cleared_or_untouched(gpu):
    meshes, vertices, triangles, origin, res, grid = CASES["two-overlapping"]
    bad = meshes.copy()
    bad[1]["pose"][5] = np.nan
    rng = np.random.default_rng(5)
    rmask = (rng.random(grid) < 0.3).astype(np.uint8)
    rids = np.where(rmask, rng.integers(1, 6, grid), 0).astype(np.uint32)
    with pytest.raises(capi.SdfGpuError) as e:
        _device(gpu, bad, vertices, triangles, origin, res, grid, check=True)
    assert e.value.code == -1 and "mesh 1 " in str(e.value)
    d_bits, d_mask, d_ids, _ = _device(gpu, bad, vertices, triangles, origin, res, grid, check=False)
    assert not d_bits.any() and not d_mask.any() and not d_ids.any()
    d_bits, d_mask, d_ids, _ = _device(gpu, bad, vertices, triangles, origin, res, grid, check=False, onto=(R.pack_bits(rmask), rmask, rids))
    assert np.array_equal(d_bits, R.pack_bits(rmask)) and np.array_equal(d_mask, rmask) and np.array_equal(d_ids, rids)
    # an origin without an inverse, and more meshes than the limit: refused by the arguments, nothing is written
    singular = np.array(origin, np.float64)
    singular[:3, 2] = 0.0
    many = np.repeat(meshes[:1], capi.MAX_SOLID_MESHES + 1)
    for args, text in (((meshes, vertices, triangles, singular, res, grid), "inverse"), ((many, vertices, triangles, origin, res, grid), "limit")):
        with pytest.raises(capi.SdfGpuError) as e:
            _device(gpu, *args, check=False, onto=(R.pack_bits(rmask), rmask, rids))
        assert text in str(e.value)
    # two refusals in one call, found by different kernels: mesh 0 has finite world vertices whose grid coordinates overflow (the
    # solid call's own check), mesh 2 a pose that is not finite (the mesh records' check).  The LOWEST index is reported by both forms.
    tiny = np.eye(4)
    tiny[:3, :3] *= 1e-100                                                      # its inverse is 1e100
    far = capi.make_meshes([(1, SC.icosahedron(1.0)[0] * 1e250, SC.icosahedron(1.0)[1], np.eye(4)), (2, *SC.icosahedron(0.2), np.eye(4)),
                            (3, *SC.icosahedron(0.2), np.eye(4))])
    far[0][2]["pose"][5] = np.nan
    for _ in range(3):
        with pytest.raises(capi.SdfGpuError) as e:
            _device(gpu, *far, tiny, 0.05, (4, 4, 4), check=True)
        assert "rasterize_solid_meshes: mesh 0 " in str(e.value)
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.rasterize_solid_meshes(*far, tiny, 0.05, (4, 4, 4))
    assert "rasterize_solid_meshes: mesh 0 is refused" in str(e.value)
    # the host form checks closedness
    with pytest.raises(capi.SdfGpuError) as e:
        opened = triangles.copy()
        opened[-1] = (opened[-1][0], opened[-1][0], opened[-1][1])                # the last triangle of mesh 1 collapsed to a segment
        gpu.rasterize_solid_meshes(meshes, vertices, opened, origin, res, grid)
    assert "mesh 1 is not closed" in str(e.value)
    _check_all(gpu, "the next call", CASES["two-overlapping"], _want("two-overlapping"))


def test_the_toggle_field_is_zero_after_every_call():
    """two different scenes back to back on one handle, each against a fresh handle: what a call left in the toggle field would
    show in the next one; a refused call and a larger grid in between"""
    first, second, third = CASES["torus"], CASES["cube-in-cube-one-mesh"], grid_scene((7, 6, 67))
    fresh = []
    for scene in (first, second, third):
        ctx = capi.SdfGpu(0)
        fresh.append(_device(ctx, *scene))
        ctx.close()
    ctx = capi.SdfGpu(0)
    try:
        bad = first[0].copy()
        bad[0]["pose"][3] = np.inf
        for k, scene in enumerate((first, second, third, first, second)):
            got = _device(ctx, *scene)
            for j, what in enumerate(("bits", "mask", "ids")):
                _equal("call %d %s" % (k, what), got[j], fresh[k % 3][j])
            _device(ctx, bad, *first[1:], check=False)
    finally:
        ctx.close()


# ---- cross-checks against what exists --------------------------------------------------------------------------------------------------
def test_a_box_as_twelve_solid_triangles_equals_the_box_primitive(gpu):
    grid, res = (24, 20, 17), SC.RES
    origin = SC.MC.origins()["general"]
    (meshes, vertices, triangles), shapes = SC.MC.box_pair(grid, origin)
    judged = scene_judge.check(SR.restated(shapes, origin, res, grid)[0], scene_judge.scene_ratio(shapes, origin, res, grid))
    ratio = J.mesh_ratio(meshes, vertices, triangles, origin, res, grid)
    assert judged[1] == 0 and int((np.abs(ratio) <= 1.0).sum()) == 0, "the pose was chosen to have no cell that either judge calls ambiguous"
    d_bits, d_mask, d_ids, _ = _device(gpu, meshes, vertices, triangles, origin, res, grid)
    n = int(np.prod(grid))
    bufs = [torch.zeros(s, dtype=torch.uint8, device="cuda") for s in ((n + 31) // 32 * 4, n, n * 4)]
    d_s = _upload(shapes)
    gpu.rasterize_shapes_device(d_s.data_ptr(), len(shapes), origin, res, grid, *(b.data_ptr() for b in bufs), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _equal("bits", d_bits, bufs[0].cpu().numpy().view(np.uint32))
    _equal("mask", d_mask, bufs[1].cpu().numpy().reshape(grid))
    _equal("ids", d_ids, bufs[2].cpu().numpy().view(np.uint32).reshape(grid))
    assert int(d_mask.sum()) > int(_device(gpu, meshes, vertices, triangles, origin, res, grid, solid=False)[1].sum())


# ---- a non-blocking side stream --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def delay():
    return H.Delay()


@pytest.fixture(scope="module")
def streams(delay):
    return H.pick_streams(delay)


@pytest.mark.parametrize("check", [False, True], ids=["pending", "checked"])
def test_the_solid_call_honours_its_stream(gpu, delay, streams, check):
    grid, res = (33, 17, 96), SC.RES
    origin = SC.MC.origins()["general"]
    ext = np.asarray(grid) * res

    def meshes(shift, first_id, scale):
        items = []
        for i, where in enumerate([(0.3, 0.5, 0.3), (0.6, 0.4, 0.6), (0.5, 0.6, 0.8)]):
            v, t = SC.icosahedron(scale * (3.0 + i) * res) if i != 1 else SC.box_triangles(np.full(3, scale * 6.3 * res))
            items.append((first_id + i, v, t, origin @ SC._local(SC.GENERIC_Q, ext * (np.asarray(where) + shift))))
        return capi.make_meshes(items)

    decoy, real = meshes(-0.08, 11, 0.8), meshes(0.0, 1, 1.0)
    decoy[2][:] = decoy[2][:, ::-1]                                            # (same counts, other index orders: the arrays differ)
    want =[S.restated(*s, origin, res, grid) for s in (decoy, real)]
    case = H.Case(delay, streams[0], streams[1])
    n = int(np.prod(grid))
    d_in = [case.input(name, np.ascontiguousarray(d).view(np.uint8).reshape(-1), np.ascontiguousarray(r).view(np.uint8).reshape(-1))
            for name, d, r in zip(("meshes", "vertices", "triangles"), decoy, real)]
    d_bits, d_mask, d_ids = case.output("bits", (n + 31) // 32 * 4), case.output("mask", n), case.output("ids", n * 4)

    def call():
        return gpu.rasterize_solid_meshes_device(d_in[0], len(real[0]), d_in[1], len(real[1]), d_in[2], len(real[2]), origin, res, grid, d_bits, d_mask, d_ids,
                                                 check=check, stream=case.side.cuda_stream)
    case.warm(call)
    case.arm()
    bad = call()
    if not check:
        case.witness("when the asynchronous call had returned")
    case.consume()
    got = case.finish()
    H.expect("the bits", H.view(got["bits"], np.uint32), want[1][2], want[0][2])
    H.expect("the mask", H.view(got["mask"], np.uint8, grid), want[1][0], want[0][0])
    H.expect("the ids", H.view(got["ids"], np.uint32, grid), want[1][1], want[0][1])
    assert bad == (-1 if check else None)
    assert not np.array_equal(want[0][0], want[1][0])
    # the same handle on the null stream afterwards: the toggle field was left clean on the side stream
    _check_all(gpu, "after the side stream", CASES["torus"], _want("torus"), host=False)


# ---- red zones -------------------------------------------------------------------------------------------------------------------------
def core_cases_on(ctx):
    for name in ("torus", "poking-out-of-all-faces", "two-overlapping", "outside"):    # (outside: a mesh whose column box stays empty)
        _check_all(ctx, name + " (red zones)", CASES[name], _want(name))
    scene = grid_scene((7, 6, 67))
    _check_all(ctx, "7x6x67 (red zones)", scene, S.restated(*scene))
    _check_all(ctx, "stack 12x6x2081 (red zones)", SC.stack_scene((12, 6, 2081)), _want_stack((12, 6, 2081)), host=False)
    _check_all(ctx, "slots (red zones)", SC.slot_scene(), _want_slot("trailing"))


def test_the_core_cases_in_a_child_process_with_red_zones_from_the_environment():
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from sdf_tools_amd import capi\nimport test_gpu_mesh_solid as T\n"
            "ctx = capi.SdfGpu(0)\nT.core_cases_on(ctx)\nctx.redzone_check()\nctx.close()\nprint('core cases clean')\n") % (tests, os.path.dirname(tests))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SDFGPU_REDZONE="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "core cases clean" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
