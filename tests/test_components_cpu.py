"""Connected components without a GPU: the C++ restatement of the reference's scan + BFS (tests/components_restated.cpp) against
hand-counted answers, and the C++ class surface (UpdateConnectedComponents / GetNumConnectedComponents /
ExtractConnectedComponents) compiled against the in-tree headers.  tests/test_gpu_components.py compares the GPU with the same
restatement."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = []


def _restated_lib():
    if not _LIB:
        out = os.path.join(tempfile.mkdtemp(prefix="components_restated_"), "components_restated.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared",
                               os.path.join(HERE, "components_restated.cpp"), "-o", out])
        L = ctypes.CDLL(out)
        L.cc_restated.restype = ctypes.c_uint32
        L.cc_restated.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
        _LIB.append(L)
    return _LIB[0]


def restated_labels(filled):
    """filled: [nx, ny, nz] (nonzero = class 1) -> (uint32 labels [nx, ny, nz], K), the reference's numbering."""
    m = np.ascontiguousarray(filled != 0, dtype=np.uint8)
    out = np.empty(m.shape, np.uint32)
    k = _restated_lib().cc_restated(m.ctypes.data, *m.shape, out.ctypes.data)
    return out, int(k)


def occupancy_class(occ):
    """The reference's predicate (collision_map.cpp:574-588): occupancy > 0.5; unknown (0.5) and NaN are free."""
    with np.errstate(invalid="ignore"):
        return np.asarray(occ, np.float32) > np.float32(0.5)


@pytest.mark.parametrize("scene, k", [("tutorial_scene", 2), ("convex_segments_scene", 9), ("estimate_distance_scene", 5),
                                      ("test_bindings_scene", 2)])
def test_known_answers(scene, k):
    m, _ = getattr(scenes, scene)()
    labels, got = restated_labels(m)
    assert got == k
    assert labels.min() == 1 and labels.max() == k


def test_checkerboard_is_all_singletons():
    x, y, z = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    labels, k = restated_labels((x + y + z) % 2)
    assert k == 64
    assert np.array_equal(labels.reshape(-1), np.arange(1, 65, dtype=np.uint32))


def test_unknown_and_nan_join_free_space():
    occ = np.zeros((3, 1, 5), np.float32)
    occ[1, 0, :] = 1.0                               # a filled wall splits the grid in two free halves ...
    occ[1, 0, 2] = 0.5                               # ... unless the unknown voxel joins them
    _, k = restated_labels(occupancy_class(occ))
    assert k == 3                                    # free (through the 0.5 voxel), wall part z < 2, wall part z > 2
    occ[1, 0, 2] = np.nan
    labels2, k2 = restated_labels(occupancy_class(occ))
    assert k2 == 3 and labels2[0, 0, 0] == labels2[2, 0, 0] == labels2[1, 0, 2]
    occ[1, 0, 2] = np.float32(0.50001)
    _, k3 = restated_labels(occupancy_class(occ))
    assert k3 == 3                                   # now two free halves and one wall


def test_diagonal_contact_does_not_connect():
    m = np.zeros((2, 2, 2), np.uint8)
    m[0, 0, 0] = m[1, 1, 0] = m[0, 1, 1] = 1           # face-diagonal pairs only
    labels, k = restated_labels(m)
    assert k == 5                                    # three single filled voxels; (0, 1, 0) is free but walled in by them
    assert labels[0, 1, 0] != labels[1, 0, 1]
    assert len({labels[0, 0, 0], labels[1, 1, 0], labels[0, 1, 1]}) == 3
    m2 = np.zeros((2, 2, 2), np.uint8)
    m2[0, 0, 0] = m2[1, 1, 1] = 1                    # body diagonal: two filled and one free component
    assert restated_labels(m2)[1] == 3


def test_scan_order_numbering():
    # x outer, y, z inner: components are numbered by their first voxel in linear order
    m = np.array([[[0, 1, 0],
                   [1, 1, 0]],
                  [[0, 0, 1],
                   [1, 0, 1]]], np.uint8)          # [2, 2, 3]
    labels, k = restated_labels(m)
    expect = np.array([[[1, 2, 3],
                        [2, 2, 3]],
                       [[1, 1, 4],
                        [2, 1, 4]]], np.uint32)
    assert k == 4
    assert np.array_equal(labels, expect)
    # a component whose first voxel comes late keeps a late number even if it is the largest
    m3 = np.zeros((3, 3, 3), np.uint8)
    m3[2, :, :] = 1
    m3[0, 0, 1] = 1
    labels3, k3 = restated_labels(m3)
    assert k3 == 3 and labels3[0, 0, 0] == 1 and labels3[0, 0, 1] == 2 and labels3[2, 2, 2] == 3
    assert np.count_nonzero(labels3 == 3) == 9


def test_labels_are_a_partition_into_connected_sets():
    rng = np.random.default_rng(5)
    m = (rng.random((9, 7, 11)) < 0.45).astype(np.uint8)
    labels, k = restated_labels(m)
    assert labels.min() == 1 and labels.max() == k
    # first occurrences of 1..K are increasing in linear order
    flat = labels.reshape(-1)
    first = np.array([np.argmax(flat == c) for c in range(1, k + 1)])
    assert np.all(np.diff(first) > 0)
    # every face-neighbour pair of one class shares a label, every pair of different classes does not
    for ax in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[ax] = slice(1, None)
        b[ax] = slice(None, -1)
        same = m[tuple(a)] == m[tuple(b)]
        assert np.array_equal(labels[tuple(a)] == labels[tuple(b)], same)


_HEADER_CHECK = r"""
#include <cstdio>
#include "sdf_tools/collision_map.hpp"
#include "sdf_tools/tagged_object_collision_map.hpp"

int main() {
    sdf_tools::CollisionMapGrid g("world", 1.0, 4, 4, 4, sdf_tools::COLLISION_CELL(0.0f));
    const uint32_t k = g.UpdateConnectedComponents();
    const std::pair<uint32_t, bool> n = g.GetNumConnectedComponents();
    const std::vector<std::vector<VoxelGrid::GRID_INDEX>> parts = g.ExtractConnectedComponents();
    g.InvalidateConnectedComponents();
    sdf_tools::TaggedObjectCollisionMapGrid t(Eigen::Isometry3d::Identity(), "world", 1.0, 4, 4, 4,
                                              sdf_tools::TAGGED_OBJECT_COLLISION_CELL(0.0f, 0u));
    const uint32_t kt = t.UpdateConnectedComponents();
    const std::pair<uint32_t, bool> nt = t.GetNumConnectedComponents();
    std::printf("%u %u %d %zu %u %u %d\n", k, n.first, (int)n.second, parts.size(), kt, nt.first, (int)nt.second);
    return 0;
}
"""


def test_class_headers_compile_with_the_component_methods(tmp_path):
    src = tmp_path / "components_header_check.cpp"
    src.write_text(_HEADER_CHECK)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])
