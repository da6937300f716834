"""Component surfaces on the MI355X (sdfgpu_component_surfaces*, CollisionMapGrid / TaggedObjectCollisionMapGrid
ExtractComponentSurfaces): counts, grouped indices and surface bits bit-equal to the numpy restatement
(tests/component_surfaces_restated.py), through every entry point.

Chunk sizes of the kernels (sdfgpu_surfaces.hpp / .hip): a wave handles 64 voxels or elements a round, k_sf_flag 256 a round,
a tile is kSfTile = 4096 voxels or elements, the scan works in segments of kSfScanSeg = 2048 table entries, and the sort takes
kSfDigitBits = 8 label bits a pass."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import analysis_scenes as A
import scenes
from component_surfaces_restated import as_map, class_select, restated_surfaces
from sdf_tools_amd import capi, synth
from sdf_tools_amd._bindings import load_pysdf_tools

pytestmark = pytest.mark.gpu

IDENT = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
ISSUE_SHAPES = [(1, 1, 1), (1, 1, 40), (7, 1, 1), (5, 6, 7), (9, 9, 33), (3, 4, 65), (2, 3, 31), (2, 3, 32)]
CHUNKS = [64, 256, 2048, 4096, 8192]
OCC_VALUES = np.array([0.0, 0.25, 0.5, 0.50000006, 0.75, 1.0, -10000.0, np.nan], np.float32)   # (test_gpu_size_limits_entry_points.py)


def _dev(a, dtype=np.uint32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype).reshape(-1).view(np.int32)).cuda()


def _device_call(ctx, labels, select, max_label, want_bits=True):
    """-> (counts, indices, reported bits as bool [n] or None) through sdfgpu_component_surfaces_device."""
    n = labels.size
    d_labels = _dev(labels)
    d_sel = None if select is None else torch.from_numpy(capi.pack_bits_host(select).view(np.int32)).cuda()
    d_bits = torch.full(((n + 31) // 32 + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if want_bits else None
    s = torch.cuda.current_stream().cuda_stream
    counts, idx = ctx.component_surfaces_device(d_labels.data_ptr(), labels.shape, max_label, None if d_sel is None else d_sel.data_ptr(),
                                                d_surface_bits=None if d_bits is None else d_bits.data_ptr(), stream=s)
    bits = None
    if want_bits:
        w = d_bits.cpu().numpy().view(np.uint32)
        assert w[-1] == 0x5A5A5A5A, "the word behind the surface bits was written"
        bits = np.unpackbits(w[:-1].view(np.uint8), bitorder="little")[:n].astype(bool)
        tail = np.unpackbits(w[:-1].view(np.uint8), bitorder="little")[n:]
        assert not tail.any(), "bits past the last voxel must be 0"
    return counts, idx, bits


def _cells(occ, labels, stride):
    c = np.zeros(occ.shape + (stride // 4,), np.float32)
    c[..., 0] = occ
    c[..., 1].view(np.uint32)[...] = labels
    if stride == 16:
        c[..., 2].view(np.uint32)[...] = 7
        c[..., 3].view(np.uint32)[...] = 9
    return c


def _same(what, got, ref, shape=None):
    assert np.array_equal(got[0], ref[0]), "%s: counts differ %s" % (what, shape)
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], ref[1]), "%s: indices differ %s" % (what, shape)


def _all_entry_points(ctx, labels, select=None, max_label=None, occ=None, class_mask=None):
    labels = np.ascontiguousarray(labels, np.uint32)
    if max_label is None:
        max_label = int(labels.max())
    ref = restated_surfaces(labels, select, max_label)
    _same("sdfgpu_component_surfaces", ctx.component_surfaces(labels, select, max_label), ref, labels.shape)
    counts, idx, bits = _device_call(ctx, labels, select, max_label)
    _same("sdfgpu_component_surfaces_device", (counts, idx), ref, labels.shape)
    assert np.array_equal(bits, ref[2].reshape(-1)), "d_surface_bits %s" % (labels.shape,)
    if occ is not None:
        for stride in (8, 16):
            cells = _cells(occ, labels, stride)
            before = cells.copy()
            got = ctx.component_surfaces_cells(cells, labels.shape, class_mask, max_label, stride, 0, 4)
            _same("sdfgpu_component_surfaces_cells (%d-byte records)" % stride, got, ref, labels.shape)
            assert np.array_equal(cells.view(np.uint32), before.view(np.uint32)), "the records are read only"
    return ref


def _random_labels(rng, shape, max_label):
    """values in 0..max_label with gaps: label 0 and max_label in use, about half of the range absent"""
    pool = np.unique(np.concatenate([[0, max_label], rng.integers(0, max_label + 1, size=max(2, min(max_label, 4000) // 2))]))
    return rng.choice(pool, size=shape).astype(np.uint32)


@pytest.mark.parametrize("shape", ISSUE_SHAPES)
def test_small_shapes(gpu, shape):
    rng = np.random.default_rng(sum(shape))
    for k in (0, 1, 5):
        labels = rng.integers(0, k + 1, size=shape).astype(np.uint32)
        sel = rng.random(shape) < 0.6
        _all_entry_points(gpu, labels, None, k)
        _all_entry_points(gpu, labels, sel, k)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_voxel_counts_around_each_chunk(gpu, chunk):
    rng = np.random.default_rng(chunk)
    for n in (chunk - 1, chunk, chunk + 1):
        labels = rng.integers(0, 3, size=(1, 1, n)).astype(np.uint32)      # (a line: every voxel is on a grid face)
        _all_entry_points(gpu, labels, None, 300)                           # two sort passes: chunk - 1 .. chunk + 1 pairs, too
        _all_entry_points(gpu, labels, rng.random((1, 1, n)) < 0.5, 2)


def test_one_label_everywhere(gpu):
    shape = (40, 33, 35)
    labels = np.full(shape, 3, np.uint32)
    counts, idx, _ = _all_entry_points(gpu, labels, None, 3)
    assert counts.tolist() == [0, 0, 0, 40 * 33 * 35 - 38 * 31 * 33] and len(idx) == counts[3]


def test_checkerboard_every_voxel_its_own_group(gpu):
    m = A.checkerboard((8, 8, 8))
    labels, k = gpu.components(m)
    assert k == 512
    counts, idx, _ = _all_entry_points(gpu, labels, None, k, m.astype(np.float32), 7)
    assert counts[0] == 0 and (counts[1:] == 1).all() and np.array_equal(np.sort(idx), np.arange(512))
    _all_entry_points(gpu, labels, m != 0, k, m.astype(np.float32), capi.TOPOLOGY_FILLED)


@pytest.mark.parametrize("p", [0.5, 0.3116])
def test_bernoulli_components(gpu, p):
    m = synth.bernoulli_mask((64, 64, 64), p, 11)
    labels, k = gpu.components(m)
    occ = m.astype(np.float32)
    _all_entry_points(gpu, labels, None, k, occ, 7)
    _all_entry_points(gpu, labels, m != 0, k, occ, capi.TOPOLOGY_FILLED)
    _all_entry_points(gpu, labels, m == 0, k, occ, capi.TOPOLOGY_EMPTY)


@pytest.mark.parametrize("scene", ["serpentine", "comb", "stripes", "nested_shells", "tori_chain"])
def test_structured_scenes(gpu, scene):
    m = getattr(A, scene)((21, 18, 23)).astype(np.uint8)
    labels, k = gpu.components(m)
    occ = m.astype(np.float32)
    _all_entry_points(gpu, labels, None, k, occ, 7)
    _all_entry_points(gpu, labels, m != 0, k, occ, capi.TOPOLOGY_FILLED)


@pytest.mark.parametrize("scene", ["test_bindings_scene", "tutorial_scene"])
def test_reference_scenes(gpu, scene):
    m, _ = getattr(scenes, scene)()
    labels, k = gpu.components(m)
    _all_entry_points(gpu, labels, None, k, np.asarray(m, np.float32), 7)


@pytest.mark.parametrize("max_label", [1, 255, 256, 65536])
def test_arbitrary_labels(gpu, max_label):
    """Labels that components would never produce, the radix pass count on both sides of a digit (8 bits: 255 | 256; 16: 65536)."""
    rng = np.random.default_rng(max_label)
    shape = (17, 19, 37)
    labels = _random_labels(rng, shape, max_label)
    assert labels.min() == 0 and labels.max() == max_label
    _all_entry_points(gpu, labels, None, max_label)
    _all_entry_points(gpu, labels, rng.random(shape) < 0.5, max_label + 7)   # (rows above the largest label stay 0)


@pytest.mark.parametrize("class_mask", [None, 1, 2, 4, 5, 7])
def test_selections_by_class(gpu, class_mask):
    rng = np.random.default_rng(8)
    shape = (23, 19, 29)
    occ = rng.choice(OCC_VALUES, size=shape)
    labels, k = gpu.components(class_select(occ, 1))
    sel = None if class_mask in (None, 7) else class_select(occ, class_mask)
    _all_entry_points(gpu, labels, sel, k, occ, 7 if class_mask is None else class_mask)
    arb = _random_labels(rng, shape, 700)                                   # each voxel stands alone: partly selected labels
    _all_entry_points(gpu, arb, sel, 700, occ, 7 if class_mask is None else class_mask)


def test_counts_only_capacity_and_canary(gpu):
    rng = np.random.default_rng(5)
    shape = (17, 19, 37)
    labels = _random_labels(rng, shape, 300)
    ref = restated_surfaces(labels, None, 300)
    total = len(ref[1])
    d_labels = _dev(labels)
    s = torch.cuda.current_stream().cuda_stream
    counts, t = gpu.component_surfaces_device(d_labels.data_ptr(), shape, 300, stream=s, counts_only=True)
    assert np.array_equal(counts, ref[0]) and t == total
    buf = torch.full((total + 64,), -77, dtype=torch.int32, device="cuda")
    counts, t = gpu.component_surfaces_device(d_labels.data_ptr(), shape, 300, d_indices=buf.data_ptr(), capacity=total, stream=s)
    got = buf.cpu().numpy()
    assert t == total and np.array_equal(counts, ref[0]) and np.array_equal(got[:total].view(np.uint32), ref[1])
    assert (got[total:] == -77).all(), "stored past the capacity"
    buf.fill_(-77)
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.component_surfaces_device(d_labels.data_ptr(), shape, 300, d_indices=buf.data_ptr(), capacity=total - 1, stream=s)
    assert e.value.code == -1 and e.value.total == total
    assert (buf.cpu().numpy() == -77).all(), "a refused call stored indices"


def test_refusals(gpu):
    labels = np.arange(24, dtype=np.uint32).reshape(2, 3, 4)
    for call in (lambda: gpu.component_surfaces(labels, None, 22),
                 lambda: _device_call(gpu, labels, None, 22),
                 lambda: gpu.component_surfaces_cells(_cells(np.zeros(labels.shape, np.float32), labels, 8), labels.shape, 7, 22)):
        with pytest.raises(capi.SdfGpuError) as e:
            call()
        assert e.value.code == -1 and "exceeds max_label" in str(e.value)
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.component_surfaces(labels, None, 2 ** 32 - 1)
    assert e.value.code == -1 and "max_label" in str(e.value)
    d = torch.zeros(16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.component_surfaces_device(d.data_ptr(), (65536, 65536, 1), 3, counts_only=True)      # 2^32 voxels: refused by shape alone
    assert e.value.code == -1 and "2^32 - 1 voxels" in str(e.value)
    assert torch.cuda.mem_get_info()[0] == before, "a call refused by its shape allocated device memory"


def test_repeat_calls_are_identical(gpu):
    m = synth.bernoulli_mask((61, 40, 53), 0.3116, 6)
    labels, k = gpu.components(m)
    a = gpu.component_surfaces(labels, m, k)
    b = gpu.component_surfaces(labels, m, k)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_surfaces_leave_sdf_builds_alone(gpu):
    a = synth.bernoulli_mask((128, 128, 128), 0.02, 3)
    b = synth.bernoulli_mask((96, 80, 72), 0.5, 4)
    sa, ea = gpu.build(a, 0.1)
    info = gpu.last_build_info()
    labels, k = gpu.components(b)
    info_cc = gpu.last_build_info()
    gpu.component_surfaces(labels, b, k)
    gpu.component_surfaces_cells(_cells(b.astype(np.float32), labels, 8), b.shape, 7, k)
    assert gpu.last_build_info() == info_cc == info
    sb, eb = gpu.build(b, 0.1)
    fresh = capi.SdfGpu(0)
    try:
        ra, fa = fresh.build(a, 0.1)
        rb, fb = fresh.build(b, 0.1)
    finally:
        fresh.close()
    assert np.array_equal(sa, ra) and ea == fa
    assert np.array_equal(sb, rb) and eb == fb


def test_fuzz(gpu):
    """200 seeded cases: axes in 1..48, random or components labels, random selections; device and host forms."""
    master = np.random.default_rng(20240607)
    for case in range(200):
        seed = int(master.integers(1 << 31))
        rng = np.random.default_rng(seed)
        shape = tuple(int(v) for v in rng.integers(1, 49, size=3))
        kind = int(rng.integers(3))
        if kind == 0:
            labels, max_label = gpu.components(rng.random(shape) < rng.random())
        else:
            max_label = int(rng.choice([0, 1, 2, 7, 255, 256, 1000, 70000, 2 ** 24 + 3]))
            labels = _random_labels(rng, shape, max_label) if kind == 1 else rng.integers(0, max_label + 1, size=shape).astype(np.uint32)
        sel = None if rng.random() < 0.3 else rng.random(shape) < rng.random()
        ref = restated_surfaces(labels, sel, max_label)
        try:
            if case % 4 == 0:
                got = gpu.component_surfaces(labels, sel, max_label)
                bits = None
            else:
                got_c, got_i, bits = _device_call(gpu, labels, sel, max_label)
                got = (got_c, got_i)
            ok = np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and (bits is None or np.array_equal(bits, ref[2].reshape(-1)))
        except Exception as e:                                              # noqa: BLE001
            raise AssertionError("fuzz case %d raised: shape %s seed %d kind %d max_label %d: %r" % (case, shape, seed, kind, max_label, e))
        assert ok, "fuzz case %d: shape %s seed %d kind %d max_label %d" % (case, shape, seed, kind, max_label)


_REDZONE_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
from sdf_tools_amd import capi, synth
from component_surfaces_restated import restated_surfaces
ctx = capi.SdfGpu(0)
rng = np.random.default_rng(3)
for shape, p in [((25, 20, 15), 0.4), ((64, 64, 64), 0.5), ((1, 300, 1), 0.5), ((7, 65, 33), 0.3116), ((1, 1, 4097), 0.5)]:
    m = synth.bernoulli_mask(shape, p, 5)
    labels, k = ctx.components(m)
    for sel in (m, None):
        ref = restated_surfaces(labels, sel, k)
        got = ctx.component_surfaces(labels, sel, k)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    cells = np.zeros(shape + (4,), np.float32)
    cells[..., 0] = m
    cells[..., 1].view(np.uint32)[...] = labels
    ref = restated_surfaces(labels, m, k)
    got = ctx.component_surfaces_cells(cells, shape, 1, k, 16, 0, 4)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    arb = rng.integers(0, 70000, size=shape).astype(np.uint32)
    ref = restated_surfaces(arb, None, 70000)
    got = ctx.component_surfaces(arb, None, 70000)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
ctx.close()
print("redzone clean")
"""


def test_redzone_clean(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "surfaces_redzone.py"
    script.write_text(_REDZONE_CHILD)
    env = dict(os.environ, SDFGPU_REDZONE="1")
    r = subprocess.run([sys.executable, str(script), os.path.dirname(here), here], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "redzone clean" in r.stdout


# ---- the C++ / pybind surface -------------------------------------------------------------------------------------------------
def _to_sets(result):
    return {int(c): set(cells) for c, cells in result.items()}


@pytest.mark.parametrize("tagged", [False, True])
def test_pysdf_tools_extract_component_surfaces(tagged):
    m = load_pysdf_tools()
    occ = np.zeros((10, 10, 10), np.float32)
    occ[3:7, 3:7, 3:7] = 1.0
    occ[0, 0, 0] = 0.5                                                      # one unknown voxel in the free component
    if tagged:
        g = m.TaggedObjectCollisionMapGrid(m.Isometry3d(IDENT), "world", 0.5, 10, 10, 10, m.TAGGED_OBJECT_COLLISION_CELL(0.0, 0))
        for x, y, z in np.argwhere(occ != 0):
            g.SetValue(int(x), int(y), int(z), m.TAGGED_OBJECT_COLLISION_CELL(float(occ[x, y, z]), 1))
        types = m.TaggedObjectCollisionMapGrid
    else:
        g = m.CollisionMapGrid(m.Isometry3d(IDENT), "world", 0.5, 10, 10, 10, m.COLLISION_CELL(0.0))
        g.SetOccupancyFromNumpy(occ)
        types = m.CollisionMapGrid
    assert g.UpdateConnectedComponents() == 2
    labels = np.where(occ > 0.5, 2, 1).astype(np.uint32)                    # scan order: free space first
    for call, mask in ((lambda: g.ExtractFilledComponentSurfaces(), 1), (lambda: g.ExtractEmptyComponentSurfaces(), 2),
                       (lambda: g.ExtractUnknownComponentSurfaces(), 4), (lambda: g.ExtractComponentSurfaces(7), 7),
                       (lambda: g.ExtractComponentSurfaces(int(types.FILLED_COMPONENTS) | int(types.UNKNOWN_COMPONENTS)), 5)):
        ref = restated_surfaces(labels, class_select(occ, mask), 2)
        want = as_map(ref[0], ref[1], occ.shape)
        got = call()
        assert _to_sets(got) == want, mask
        assert all(v == 1 for cells in got.values() for v in cells.values())
        offsets, idx = g.ExtractComponentSurfaceIndicesNumpy(mask)
        assert offsets.dtype == np.int64 and idx.dtype == np.uint32
        assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(ref[0])])) and np.array_equal(idx, ref[1])
