"""Component topology on the MI355X (sdfgpu_component_topology*, CollisionMapGrid / TaggedObjectCollisionMapGrid
ComputeComponentTopology): all five counters of every label bit-equal to the C++ restatement of the reference
(tests/topology_restated.cpp, corrected mode), through every entry point."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scenes
from sdf_tools_amd import capi, synth
from sdf_tools_amd._bindings import load_pysdf_tools
from test_components_cpu import restated_labels
from test_topology_cpu import KNOWN, SHAPES, holes_voids, restated_counts

pytestmark = pytest.mark.gpu

IDENT = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
ODD_SHAPES = [(1, 1, 1), (1, 1, 77), (1, 300, 1), (3, 1, 40), (33, 2, 1), (25, 20, 15), (7, 65, 33), (40, 33, 45)]


def _device_counts(ctx, labels, select, max_label):
    d_labels = torch.from_numpy(np.ascontiguousarray(labels, np.uint32).reshape(-1).view(np.int32)).cuda()
    d_sel = None if select is None else torch.from_numpy(capi.pack_bits_host(select).view(np.int32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    return ctx.component_topology_device(d_labels.data_ptr(), labels.shape, max_label, None if d_sel is None else d_sel.data_ptr(),
                                         stream)


def _cells(occ, labels, stride):
    c = np.zeros(occ.shape + (stride // 4,), np.float32)
    c[..., 0] = occ
    c[..., 1].view(np.uint32)[...] = labels
    if stride == 16:
        c[..., 2].view(np.uint32)[...] = 7
        c[..., 3].view(np.uint32)[...] = 9
    return c


def _all_entry_points(ctx, labels, select=None, max_label=None, occ=None, class_mask=None):
    """Every form against the restatement; with occ, the cell forms too (class_mask selects like `select` does)."""
    labels = np.ascontiguousarray(labels, np.uint32)
    if max_label is None:
        max_label = int(labels.max())
    ref = restated_counts(labels, select=select, max_label=max_label)
    got = ctx.component_topology(labels, select, max_label)
    assert np.array_equal(got, ref), "sdfgpu_component_topology"
    got = _device_counts(ctx, labels, select, max_label)
    assert np.array_equal(got, ref), "sdfgpu_component_topology_device"
    if occ is not None:
        for stride in (8, 16):
            cells = _cells(occ, labels, stride)
            before = cells.copy()
            got = ctx.component_topology_cells(cells, labels.shape, class_mask, max_label, stride, 0, 4)
            assert np.array_equal(got, ref), "sdfgpu_component_topology_cells (%d-byte records)" % stride
            assert np.array_equal(cells.view(np.uint32), before.view(np.uint32)), "the records are read only"
    return ref


def _both_modes(ctx, mask):
    """mask: filled voxels.  Labels from the components restatement; FILLED-only selection and every component."""
    labels, k = restated_labels(mask)
    occ = mask.astype(np.float32)
    filled = _all_entry_points(ctx, labels, mask != 0, k, occ, capi.TOPOLOGY_FILLED)
    every = _all_entry_points(ctx, labels, None, k, occ, 7)
    return labels, filled, every


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(gpu, name):
    _, filled, every = _both_modes(gpu, SHAPES[name]())
    want_filled, want_every = KNOWN[name]
    assert holes_voids(filled) == want_filled
    if want_every is not None:
        assert holes_voids(every) == want_every


@pytest.mark.parametrize("scene", ["test_bindings_scene", "tutorial_scene", "convex_segments_scene", "estimate_distance_scene"])
def test_reference_scenes(gpu, scene):
    m, _ = getattr(scenes, scene)()
    _both_modes(gpu, m)


@pytest.mark.parametrize("shape", ODD_SHAPES)
@pytest.mark.parametrize("p", [0.05, 0.3116, 0.5, 0.9])
def test_bernoulli_odd_shapes(gpu, shape, p):
    m = synth.bernoulli_mask(shape, p, 17)
    _both_modes(gpu, m)


def test_unknown_and_empty_selected_by_class(gpu):
    """The cell form's EMPTY / UNKNOWN masks, on labels whose components never mix the classes (free space split by class)."""
    rng = np.random.default_rng(8)
    occ = rng.choice(np.array([0.0, 0.5, np.nan, 1.0], np.float32), size=(23, 19, 29))
    with np.errstate(invalid="ignore"):
        cls = np.where(occ > 0.5, 1, np.where(occ < 0.5, 2, 4)).astype(np.uint8)
    # components per class (the library's components are two-class; a three-class labelling is built from three two-class ones)
    labels = np.zeros(occ.shape, np.uint32)
    nxt = 0
    for c in (1, 2, 4):
        lab, _ = restated_labels(cls == c)
        inside = cls == c
        ids = np.unique(lab[inside])
        remap = np.zeros(int(lab.max()) + 1, np.uint32)
        remap[ids] = np.arange(nxt + 1, nxt + 1 + len(ids), dtype=np.uint32)
        labels[inside] = remap[lab[inside]]
        nxt += len(ids)
    for mask in (1, 2, 4, 3, 5, 6, 7):
        sel = (cls & mask) != 0
        _all_entry_points(gpu, labels, None if mask == 7 else sel, nxt, occ, mask)


def test_arbitrary_labels_without_selection(gpu):
    rng = np.random.default_rng(4)
    for shape, k in [((9, 8, 7), 3), ((31, 17, 40), 12), ((64, 1, 33), 2), ((20, 20, 20), 4000)]:
        labels = rng.integers(0, k, size=shape).astype(np.uint32)       # label 0 in use; labels need not be connected
        _all_entry_points(gpu, labels, None, k + 5)                       # (rows above the largest label stay 0)


def test_label_zero_in_use(gpu):
    m = SHAPES["ring"]()
    labels = m.astype(np.uint32)                                            # free 0, ring 1
    ref = _all_entry_points(gpu, labels, None, 1, m.astype(np.float32), 7)
    assert holes_voids(ref) == {0: (1, 1), 1: (1, 0)}


def test_refuses_a_label_over_both_classes(gpu):
    m = np.zeros((7, 7, 7), np.uint8)
    m[:3, :3, :3] = 1
    labels = np.zeros(m.shape, np.uint32)                                   # stale labels: 0 everywhere
    for call in (lambda: gpu.component_topology(labels, m, 0),
                 lambda: _device_counts(gpu, labels, m, 0),
                 lambda: gpu.component_topology_cells(_cells(m.astype(np.float32), labels, 8), m.shape, capi.TOPOLOGY_FILLED, 0)):
        with pytest.raises(capi.SdfGpuError) as e:
            call()
        assert e.value.code == -1 and "both selected and unselected" in str(e.value)
    assert gpu.component_topology(labels, None, 0)[0, 0] > 0              # without a selection the same labels are fine


def test_refuses_max_label_too_small(gpu):
    labels, k = restated_labels(SHAPES["two_voxels"]())
    for call in (lambda: gpu.component_topology(labels, None, k - 1),
                 lambda: _device_counts(gpu, labels, None, k - 1)):
        with pytest.raises(capi.SdfGpuError) as e:
            call()
        assert e.value.code == -1 and "exceeds max_label" in str(e.value)
    d = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.SdfGpuError):
        gpu.component_topology_device(d.data_ptr(), (65536, 65536, 1), 3)   # more than 2^32 - 1 voxels


@pytest.mark.parametrize("scene", ["bernoulli_0.5", "room"])
def test_large(gpu, scene):
    """256^3: the single-core restatement takes about 20 s per case here (512^3 takes minutes)."""
    n = 256
    if scene == "room":
        m = synth.room_mask_torch((n, n, n), "cpu").numpy()
    else:
        m = synth.bernoulli_mask((n, n, n), 0.5, 3)
    labels, k = restated_labels(m)
    ref = restated_counts(labels, max_label=k)
    got = _device_counts(gpu, labels, None, k)
    assert np.array_equal(got, ref)
    again = _device_counts(gpu, labels, None, k)
    assert np.array_equal(again, got)                                       # integer counts: bit-reproducible


def test_repeat_calls_are_identical(gpu):
    m = synth.bernoulli_mask((97, 64, 81), 0.3116, 6)
    labels, k = restated_labels(m)
    a = gpu.component_topology(labels, m, k)
    b = gpu.component_topology(labels, m, k)
    assert np.array_equal(a, b)


def test_topology_leaves_sdf_builds_alone(gpu):
    a = synth.bernoulli_mask((128, 128, 128), 0.02, 3)
    b = synth.bernoulli_mask((96, 80, 72), 0.5, 4)
    sa, ea = gpu.build(a, 0.1)
    labels, k = restated_labels(b)
    gpu.component_topology(labels, b, k)
    gpu.component_topology_cells(_cells(b.astype(np.float32), labels, 8), b.shape, 7, k)
    sb, eb = gpu.build(b, 0.1)
    fresh = capi.SdfGpu(0)
    try:
        ra, fa = fresh.build(a, 0.1)
        rb, fb = fresh.build(b, 0.1)
    finally:
        fresh.close()
    assert np.array_equal(sa, ra) and ea == fa
    assert np.array_equal(sb, rb) and eb == fb


_REDZONE_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
from sdf_tools_amd import capi, synth
from test_components_cpu import restated_labels
from test_topology_cpu import restated_counts
ctx = capi.SdfGpu(0)
for shape, p in [((25, 20, 15), 0.4), ((64, 64, 64), 0.5), ((1, 300, 1), 0.5), ((7, 65, 33), 0.3116)]:
    m = synth.bernoulli_mask(shape, p, 5)
    labels, k = restated_labels(m)
    for sel in (m, None):
        assert np.array_equal(ctx.component_topology(labels, sel, k), restated_counts(labels, select=sel, max_label=k))
    cells = np.zeros(shape + (4,), np.float32)
    cells[..., 0] = m
    cells[..., 1].view(np.uint32)[...] = labels
    assert np.array_equal(ctx.component_topology_cells(cells, shape, 1, k, 16, 0, 4), restated_counts(labels, select=m, max_label=k))
ctx.close()
print("redzone clean")
"""


def test_redzone_clean(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "topology_redzone.py"
    script.write_text(_REDZONE_CHILD)
    env = dict(os.environ, SDFGPU_REDZONE="1")
    r = subprocess.run([sys.executable, str(script), os.path.dirname(here), here], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "redzone clean" in r.stdout


# ---- the C++ / pybind surface -------------------------------------------------------------------------------------------------
def test_pysdf_binding_returns_the_same_dict():
    m = load_pysdf_tools()
    for name in ("ring", "cube_two_cavities", "convex_segments"):
        occ = SHAPES[name]().astype(np.float32)
        g = m.CollisionMapGrid(m.Isometry3d(IDENT), "world", 0.5, *occ.shape, m.COLLISION_CELL(0.0))
        g.SetOccupancyFromNumpy(occ)
        filled, every = KNOWN[name]
        assert g.ComputeComponentTopology() == filled
        assert g.GetNumConnectedComponents()[1] is True
        assert g.ComputeComponentTopology(False, False, False) == every
        assert g.ComputeComponentTopology(ignore_empty_components=False, recompute_connected_components=True) == every
        labels, k = restated_labels(occ > 0.5)
        assert g.ComputeComponentTopology(True) == holes_voids(restated_counts(labels, select=occ > 0.5, max_label=k))


_CLIENT = r"""
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include "sdf_tools/collision_map.hpp"
#include "sdf_tools/tagged_object_collision_map.hpp"

using Map = std::map<uint32_t, std::pair<int32_t, int32_t>>;

static void print(const char* tag, const Map& m) {
    std::printf("%s", tag);
    for (const auto& kv : m) std::printf(" %u:%d:%d", kv.first, kv.second.first, kv.second.second);
    std::printf("\n");
}

int main() {
    // a 7x7x3 ring in 11x11x7 (the table's ring)
    sdf_tools::CollisionMapGrid g("world", 1.0, 11, 11, 7, sdf_tools::COLLISION_CELL(0.0f));
    for (int64_t x = 2; x < 9; ++x)
        for (int64_t y = 2; y < 9; ++y)
            for (int64_t z = 2; z < 5; ++z)
                if (!(x >= 4 && x < 7 && y >= 4 && y < 7)) g.SetValue(x, y, z, sdf_tools::COLLISION_CELL(1.0f));
    print("cmg_filled", g.ComputeComponentTopology(true, true, false));
    print("cmg_all", g.ComputeComponentTopology(false, false, true));

    // tagged: the same ring; free space is empty (0.0) except an unknown (0.5) block in the ring's hole
    sdf_tools::TaggedObjectCollisionMapGrid t(Eigen::Isometry3d::Identity(), "world", 1.0, 11, 11, 7,
                                              sdf_tools::TAGGED_OBJECT_COLLISION_CELL(0.0f, 0u));
    for (int64_t x = 2; x < 9; ++x)
        for (int64_t y = 2; y < 9; ++y)
            for (int64_t z = 2; z < 5; ++z)
                if (!(x >= 4 && x < 7 && y >= 4 && y < 7)) t.SetValue(x, y, z, sdf_tools::TAGGED_OBJECT_COLLISION_CELL(1.0f, 3u));
    print("tag_filled", t.ComputeComponentTopology(sdf_tools::TaggedObjectCollisionMapGrid::FILLED_COMPONENTS, true, false));
    using T = sdf_tools::TaggedObjectCollisionMapGrid;
    print("tag_all", t.ComputeComponentTopology((T::COMPONENT_TYPES)(T::FILLED_COMPONENTS | T::EMPTY_COMPONENTS | T::UNKNOWN_COMPONENTS), false, false));
    print("tag_empty", t.ComputeComponentTopology(T::EMPTY_COMPONENTS, false, false));
    for (int64_t x = 4; x < 7; ++x)
        for (int64_t y = 4; y < 7; ++y)
            t.SetValue(x, y, 3, sdf_tools::TAGGED_OBJECT_COLLISION_CELL(0.5f, 0u));
    try {
        t.ComputeComponentTopology(T::EMPTY_COMPONENTS, true, false);     // the free component holds empty AND unknown voxels
        std::printf("no throw\n");
        return 2;
    } catch (const std::invalid_argument& e) {
        std::printf("invalid_argument %s\n", e.what());
    }
    print("tag_all_unknown", t.ComputeComponentTopology((T::COMPONENT_TYPES)(T::EMPTY_COMPONENTS | T::UNKNOWN_COMPONENTS | T::FILLED_COMPONENTS), false, false));
    return 0;
}
"""


def _parse(line):
    tag, *items = line.split()
    return tag, {int(c): (int(h), int(v)) for c, h, v in (it.split(":") for it in items)}


def test_cpp_client_both_grid_classes(tmp_path):
    from sdf_tools_amd import build as B

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "topology_client.cpp"
    src.write_text(_CLIENT)
    exe = str(tmp_path / "topology_client")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-I", os.path.join(root, "include"), str(src),
                           "-o", exe, "-L", B.PKG, "-lsdfgpu", "-Wl,-rpath," + B.PKG, "-lz"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    verbose = [ln for ln in lines if ln.startswith("Processing surface with M3 = ")]
    assert len(verbose) == 2                                               # cmg_all: one line per component
    got = dict(_parse(ln) for ln in lines if ln.split()[0] in ("cmg_filled", "cmg_all", "tag_filled", "tag_all", "tag_empty",
                                                                "tag_all_unknown"))
    filled, every = KNOWN["ring"]
    assert got["cmg_filled"] == filled and got["cmg_all"] == every
    assert got["tag_filled"] == filled and got["tag_all"] == every
    assert got["tag_empty"] == {1: every[1]}
    assert any(ln.startswith("invalid_argument") and "both selected and unselected" in ln for ln in lines)
    # with the unknown block every class is selected: the restatement on the same labels (free space is one component)
    ring = SHAPES["ring"]()
    labels, k = restated_labels(ring)
    assert got["tag_all_unknown"] == holes_voids(restated_counts(labels, max_label=k))
