"""Connected components on the MI355X (sdfgpu_components*, CollisionMapGrid / TaggedObjectCollisionMapGrid
UpdateConnectedComponents): labels bit-equal to the C++ restatement of the reference's scan + BFS, through every entry point."""
import os

import numpy as np
import pytest
import torch

import scenes
from sdf_tools_amd import capi, synth
from sdf_tools_amd._bindings import load_pysdf_tools
from test_components_cpu import occupancy_class, restated_labels

pytestmark = pytest.mark.gpu

IDENT = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
ODD_SHAPES = [(1, 1, 1), (25, 20, 15), (100, 100, 50), (1, 300, 1), (1, 1, 77), (3, 1, 40), (33, 2, 1), (7, 65, 33)]


def _cells8(occ):
    c = np.zeros(occ.shape + (2,), np.float32)
    c[..., 0] = occ
    c[..., 1].view(np.uint32)[...] = 0xDEADBEEF           # stale labels: every record must be overwritten
    return c


def _cells16(occ):
    c = np.zeros(occ.shape + (4,), np.float32)
    c[..., 0] = occ
    c[..., 1].view(np.uint32)[...] = 0xDEADBEEF
    c[..., 2].view(np.uint32)[...] = 7                     # object id and convex segment stay untouched
    c[..., 3].view(np.uint32)[...] = 9
    return c


def _device_labels(ctx, mask):
    bits = torch.from_numpy(capi.pack_bits_host(mask).view(np.int32)).cuda()
    out = torch.empty(mask.size, dtype=torch.int32, device="cuda")
    k = ctx.components_bits_device(bits.data_ptr(), mask.shape, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy().view(np.uint32).reshape(mask.shape), k


def _all_entry_points(ctx, occ):
    """occ: float occupancy [nx, ny, nz].  Checks the mask, bits-device and both cell-record forms against the restatement."""
    cls = occupancy_class(occ)
    ref, k = restated_labels(cls)
    got, kg = ctx.components(cls)
    assert kg == k and np.array_equal(got, ref), "sdfgpu_components"
    got, kg = _device_labels(ctx, cls.astype(np.uint8))
    assert kg == k and np.array_equal(got, ref), "sdfgpu_components_bits_device"
    c8 = _cells8(occ)
    assert ctx.components_cells(c8, occ.shape, 8, 0, 4) == k
    assert np.array_equal(c8[..., 1].view(np.uint32), ref), "sdfgpu_components_cells (8-byte records)"
    assert np.array_equal(c8[..., 0], occ, equal_nan=True)
    c16 = _cells16(occ)
    assert ctx.components_cells(c16, occ.shape, 16, 0, 4) == k
    assert np.array_equal(c16[..., 1].view(np.uint32), ref), "sdfgpu_components_cells (16-byte records)"
    assert np.all(c16[..., 2].view(np.uint32) == 7) and np.all(c16[..., 3].view(np.uint32) == 9)
    return k


@pytest.mark.parametrize("scene, k", [("tutorial_scene", 2), ("convex_segments_scene", 9), ("estimate_distance_scene", 5),
                                      ("test_bindings_scene", 2)])
def test_scenes_known_answers(gpu, scene, k):
    m, _ = getattr(scenes, scene)()
    assert _all_entry_points(gpu, m.astype(np.float32)) == k


def test_checkerboard(gpu):
    x, y, z = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    assert _all_entry_points(gpu, ((x + y + z) % 2).astype(np.float32)) == 64


def test_unknown_and_nan_are_free(gpu):
    rng = np.random.default_rng(3)
    occ = rng.choice(np.array([0.0, 0.5, np.nan, 1.0, 0.50001, 0.49999], np.float32), size=(37, 29, 45))
    _all_entry_points(gpu, occ)
    wall = np.zeros((3, 1, 5), np.float32)
    wall[1, 0, :] = 1.0
    wall[1, 0, 2] = np.nan
    assert _all_entry_points(gpu, wall) == 3


@pytest.mark.parametrize("shape", ODD_SHAPES)
@pytest.mark.parametrize("p", [0.0, 0.3, 0.6, 1.0])
def test_odd_shapes(gpu, shape, p):
    occ = (np.random.default_rng(hash((shape, p)) & 0xFFFF).random(shape) < p).astype(np.float32)
    _all_entry_points(gpu, occ)


# (129, 256, 255): 8 421 120 voxels in 1028 ranking chunks of 8192, the last one partial.  k_cc_scan's 1024 threads then take two
# chunk counts each, the threads from 514 on none, and the rank of a root adds up chunk offsets across many chunk boundaries; every
# other shape of this file has at most 1024 chunks (one count per thread or none) or a whole number of counts per thread.
BERNOULLI = [
    ((64, 64, 64), 0.02), ((200, 130, 97), 0.02),
    ((64, 64, 64), 0.3116), ((200, 130, 97), 0.3116),
    ((64, 64, 64), 0.5), ((200, 130, 97), 0.5),
    ((64, 64, 64), 0.98), ((200, 130, 97), 0.98),
    ((129, 256, 255), 0.5),
]
BERNOULLI_IDS = ["0.02-shape0", "0.02-shape1", "0.3116-shape0", "0.3116-shape1", "0.5-shape0", "0.5-shape1", "0.98-shape0", "0.98-shape1",
                 "0.5-shape2"]       # (the ids the two stacked parametrize marks gave the first eight)


@pytest.mark.parametrize("shape, p", BERNOULLI, ids=BERNOULLI_IDS)
def test_bernoulli(gpu, shape, p):
    m = synth.bernoulli_mask(shape, p, 11)
    _all_entry_points(gpu, m.astype(np.float32))


def test_512_percolation_threshold(gpu):
    n = 512
    m = synth.bernoulli_mask((n, n, n), 0.3116, 2)
    ref, k = restated_labels(m)
    got, kg = _device_labels(gpu, m)
    assert kg == k
    assert np.array_equal(got, ref)


def test_voxelize_bits_labels_chain(gpu):
    n = 96
    pts = torch.from_numpy(synth.two_box_points(20000, seed=4)).cuda()
    origin, res = (0.0, 0.0, 0.0), 1.0 / n
    stream = torch.cuda.current_stream().cuda_stream
    bits = torch.zeros((n ** 3 + 31) // 32, dtype=torch.int32, device="cuda")
    gpu.voxelize_points_bits_device(pts.data_ptr(), pts.shape[0], origin, res, (n, n, n), bits.data_ptr(), True, stream)
    labels = torch.empty(n ** 3, dtype=torch.int32, device="cuda")
    k = gpu.components_bits_device(bits.data_ptr(), (n, n, n), labels.data_ptr(), stream)
    mask = torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
    gpu.voxelize_points_device(pts.data_ptr(), pts.shape[0], origin, res, (n, n, n), mask.data_ptr(), True, stream)
    ref, kr = restated_labels(mask.cpu().numpy())
    assert k == kr and kr > 2
    assert np.array_equal(labels.cpu().numpy().view(np.uint32).reshape(n, n, n), ref)


def test_redzone_clean():
    ctx = capi.SdfGpu(0)
    try:
        ctx.set_option("redzone", 1)
        for shape in [(25, 20, 15), (64, 64, 64), (1, 300, 1)]:
            occ = (np.random.default_rng(1).random(shape) < 0.4).astype(np.float32)
            _all_entry_points(ctx, occ)
        m = synth.bernoulli_mask((200, 130, 97), 0.3116, 5)
        ref, k = restated_labels(m)
        bits = torch.from_numpy(capi.pack_bits_host(m).view(np.int32)).cuda()
        d_labels = ctx.device_malloc(m.size * 4)                 # covered by the canaries too
        try:
            assert ctx.components_bits_device(bits.data_ptr(), m.shape, d_labels, 0) == k
            got = np.empty(m.size, np.uint32)
            ctx.copy_to_host(got, d_labels)
        finally:
            ctx.device_free(d_labels)
        assert np.array_equal(got.reshape(m.shape), ref)
    finally:
        ctx.close()


def test_refuses_more_than_uint32_voxels(gpu):
    bits = torch.zeros(16, dtype=torch.int32, device="cuda")
    labels = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.components_bits_device(bits.data_ptr(), (65536, 65536, 1), labels.data_ptr(), 0)
    assert e.value.code == -1
    with pytest.raises(capi.SdfGpuError):
        gpu.components_bits_device(bits.data_ptr(), (0, 4, 4), labels.data_ptr(), 0)


def test_components_leave_sdf_builds_alone(gpu):
    a = synth.bernoulli_mask((128, 128, 128), 0.02, 3)
    b = synth.bernoulli_mask((96, 80, 72), 0.5, 4)
    sa, ea = gpu.build(a, 0.1)
    gpu.components(b)
    gpu.components_cells(_cells8(a.astype(np.float32)), a.shape)
    sb, eb = gpu.build(b, 0.1)
    fresh = capi.SdfGpu(0)
    try:
        ra, fa = fresh.build(a, 0.1)
        rb, fb = fresh.build(b, 0.1)
    finally:
        fresh.close()
    assert np.array_equal(sa, ra) and ea == fa
    assert np.array_equal(sb, rb) and eb == fb


# ---- the C++ / pybind surface -------------------------------------------------------------------------------------------------
def _grid(m, occ):
    g = m.CollisionMapGrid(m.Isometry3d(IDENT), "world", 0.5, *occ.shape, m.COLLISION_CELL(0.0))
    g.SetOccupancyFromNumpy(occ)
    return g


def test_collision_map_grid_surface(tmp_path):
    m = load_pysdf_tools()
    occ, _ = scenes.convex_segments_scene()
    occ = occ.astype(np.float32)
    g = _grid(m, occ)
    assert g.GetNumConnectedComponents() == (0, False)
    assert g.UpdateConnectedComponents() == 9
    assert g.GetNumConnectedComponents() == (9, True)
    ref, _ = restated_labels(occ > 0.5)
    assert np.array_equal(g.GetComponentsNumpy(), ref)
    assert g.GetValueByIndex(0, 0, 0)[0].component == ref[0, 0, 0]

    # SetValue clears the flag; the next update recomputes (a filled voxel dropped into the free region)
    assert g.SetValue(30, 30, 20, m.COLLISION_CELL(1.0))
    assert g.GetNumConnectedComponents()[1] is False
    occ2 = occ.copy()
    occ2[30, 30, 20] = 1.0
    ref2, k2 = restated_labels(occ2 > 0.5)
    assert k2 == 10
    assert g.UpdateConnectedComponents() == 10
    assert np.array_equal(g.GetComponentsNumpy(), ref2)

    # files round-trip labels, K and the flag; a loaded grid with the flag set early-outs
    path = str(tmp_path / "components.cmg")
    for compress in (False, True):
        g.SaveToFile(path, compress)
        h = m.CollisionMapGrid.LoadFromFile(path)
        assert h.GetNumConnectedComponents() == (10, True)
        assert np.array_equal(h.GetComponentsNumpy(), ref2)
    # the early-out returns the stored K without touching the cells: give the file a K nothing could compute
    h = m.CollisionMapGrid.Deserialize(_with_count(g.SerializeSelf(), 12345))
    assert h.UpdateConnectedComponents() == 12345
    assert np.array_equal(h.GetComponentsNumpy(), ref2)

    # SetOccupancyFromNumpy clears the flag too (it resets every cell's label)
    g.SetOccupancyFromNumpy(occ)
    assert g.GetNumConnectedComponents()[1] is False
    assert g.UpdateConnectedComponents() == 9
    assert np.array_equal(g.GetComponentsNumpy(), ref)


def _with_count(blob, k):
    """SerializeSelf ends with uint32 number_of_components, the frame string (uint64 length + bytes) and the uint8 flag."""
    b = bytearray(blob)
    frame_len = len("world")
    off = len(b) - 1 - frame_len - 8 - 4
    assert bytes(b[off + 4 + 8:off + 4 + 8 + frame_len]) == b"world" and b[-1] == 1
    b[off:off + 4] = np.uint32(k).tobytes()
    return bytes(b)


def test_tagged_grid_surface():
    m = load_pysdf_tools()
    occ = synth.bernoulli_mask((40, 33, 21), 0.3116, 9)
    ref, k = restated_labels(occ)
    g = m.TaggedObjectCollisionMapGrid(m.Isometry3d(IDENT), "world", 0.5, *occ.shape, m.TAGGED_OBJECT_COLLISION_CELL(0.0, 0))
    for x, y, z in zip(*np.nonzero(occ)):
        g.SetValue(int(x), int(y), int(z), m.TAGGED_OBJECT_COLLISION_CELL(1.0, int(x % 3)))
    assert g.GetNumConnectedComponents() == (0, False)
    assert g.UpdateConnectedComponents() == k
    assert g.GetNumConnectedComponents() == (k, True)
    for (x, y, z) in [(0, 0, 0), (39, 32, 20), (17, 5, 11), (3, 30, 2)]:
        cell = g.GetValueByIndex(x, y, z)[0]
        assert cell.component == ref[x, y, z]
        assert cell.object_id == (x % 3 if occ[x, y, z] else 0)


_EXTRACT = r"""
#include <cstdio>
#include "sdf_tools/collision_map.hpp"

int main() {
    const int64_t nx = 23, ny = 17, nz = 29;
    sdf_tools::CollisionMapGrid g("world", 1.0, nx, ny, nz, sdf_tools::COLLISION_CELL(0.0f));
    uint64_t s = 12345;
    for (int64_t x = 0; x < nx; ++x)
        for (int64_t y = 0; y < ny; ++y)
            for (int64_t z = 0; z < nz; ++z) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                g.SetValue(x, y, z, sdf_tools::COLLISION_CELL((s >> 33) % 100 < 40 ? 1.0f : 0.0f));
            }
    const auto parts = g.ExtractConnectedComponents();
    const auto n = g.GetNumConnectedComponents();
    if (!n.second || parts.size() != n.first) return 2;
    size_t total = 0;
    for (size_t c = 0; c < parts.size(); ++c) {
        const auto& p = parts[c];
        if (p.empty()) return 3;
        total += p.size();
        for (size_t i = 0; i < p.size(); ++i) {
            if (g.GetImmutable(p[i]).first.component != c + 1) return 4;
            if (i > 0 && g.GetDataIndex(p[i]) <= g.GetDataIndex(p[i - 1])) return 5;        // scan order inside a component
        }
        if (c > 0 && g.GetDataIndex(p[0]) <= g.GetDataIndex(parts[c - 1][0])) return 6;     // components in scan order
    }
    if (total != (size_t)(nx * ny * nz)) return 7;
    std::printf("%u %zu\n", n.first, total);
    return 0;
}
"""


def test_extract_connected_components_cpp(tmp_path):
    import subprocess

    from sdf_tools_amd import build as B

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "extract_components.cpp"
    src.write_text(_EXTRACT)
    exe = str(tmp_path / "extract_components")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-I", os.path.join(root, "include"), str(src),
                           "-o", exe, "-L", B.PKG, "-lsdfgpu", "-Wl,-rpath," + B.PKG, "-lz"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    k, total = (int(v) for v in r.stdout.split())
    assert total == 23 * 17 * 29 and k > 1
