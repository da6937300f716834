"""Component topology without a GPU: the C++ restatement of the reference's ComputeComponentTopology
(tests/topology_restated.cpp) on shapes whose genus and cavity count are known by construction, the evidence that the reference
as written throws on them, and the C truncation of the hole formula.  tests/test_gpu_topology.py compares the GPU with the same
restatement."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import scenes
from test_components_cpu import restated_labels

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = []


def _restated_lib():
    if not _LIB:
        out = os.path.join(tempfile.mkdtemp(prefix="topology_restated_"), "topology_restated.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared",
                               os.path.join(HERE, "topology_restated.cpp"), "-o", out])
        L = ctypes.CDLL(out)
        L.topo_restated.restype = ctypes.c_int
        L.topo_restated.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint32,
                                    ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        _LIB.append(L)
    return _LIB[0]


class WouldThrow(Exception):
    """The reference's ComputeConnectivityOfSurfaceVertices would throw std::out_of_range at vertex self.args[0]."""


def restated_counts(labels, select=None, max_label=None, literal=False, oob_component=0):
    """labels: uint32 [nx, ny, nz]; select: bool/uint8 [nx, ny, nz] or None (every voxel).  Returns int64 [max_label + 1, 5]:
    surface vertices, M3, M5, M6, surfaces per label."""
    lab = np.ascontiguousarray(labels, dtype=np.uint32)
    if max_label is None:
        max_label = int(lab.max()) if lab.size else 0
    sel = None if select is None else np.ascontiguousarray(np.asarray(select) != 0, dtype=np.uint8)
    out = np.zeros((max_label + 1, 5), np.int64)
    at = np.zeros(3, np.int64)
    rc = _restated_lib().topo_restated(lab.ctypes.data, None if sel is None else sel.ctypes.data, *lab.shape, max_label,
                                       int(literal), oob_component, out.ctypes.data, at.ctypes.data)
    if rc == 1:
        raise WouldThrow(tuple(int(v) for v in at))
    if rc != 0:
        raise ValueError("a label exceeds max_label")
    return out


def c_div(a, b):
    """C integer division (truncation toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def holes_voids(counts):
    """counters [L, 5] -> {component: (holes, voids)} for every component with a surface vertex, as the reference computes it."""
    out = {}
    for c in np.nonzero(counts[:, 0])[0]:
        _, m3, m5, m6, surfaces = (int(v) for v in counts[c])
        voids = surfaces - 1
        out[int(c)] = (1 + c_div(m5 + 2 * m6 - m3, 8) + voids, voids)
    return out


# ---- the constructed shapes (occupancy masks; components come from the components restatement) ------------------------------
def box_in(shape, lo, hi):
    m = np.zeros(shape, np.uint8)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    return m


def single_voxel_9():
    return scenes.single_voxel((9, 9, 9))


def solid_box_5_in_9():
    return box_in((9, 9, 9), (2, 2, 2), (7, 7, 7))


def ring_7x7x3():
    m = box_in((11, 11, 7), (2, 2, 2), (9, 9, 5))
    m[4:7, 4:7, :] = 0
    return m


def slab_two_tunnels():
    m = box_in((13, 9, 7), (2, 2, 2), (11, 7, 5))
    m[4, 4, :] = 0
    m[8, 4, :] = 0
    return m


def shell_with_cavity():
    m = box_in((11, 11, 11), (2, 2, 2), (9, 9, 9))
    m[4:7, 4:7, 4:7] = 0
    return m


def cube_two_cavities():
    m = box_in((13, 13, 13), (2, 2, 2), (11, 11, 11))
    m[4:6, 4:6, 4:6] = 0
    m[7:9, 7:9, 7:9] = 0
    return m


def two_voxels():
    m = np.zeros((6, 6, 6), np.uint8)
    m[1, 1, 1] = m[4, 4, 4] = 1
    return m


def all_filled():
    return np.ones((5, 5, 5), np.uint8)


SHAPES = {
    "single_voxel": single_voxel_9,
    "solid_box": solid_box_5_in_9,
    "ring": ring_7x7x3,
    "slab_two_tunnels": slab_two_tunnels,
    "shell_with_cavity": shell_with_cavity,
    "cube_two_cavities": cube_two_cavities,
    "two_voxels": two_voxels,
    "all_filled": all_filled,
    "tutorial": lambda: scenes.tutorial_scene()[0],
    "convex_segments": lambda: scenes.convex_segments_scene()[0],
    "estimate_distance": lambda: scenes.estimate_distance_scene()[0],
}

_CS_FILLED = {c: (0, 0) for c in (1, 3, 4, 5, 6, 7, 8, 9)}
_ED_FILLED = {c: (0, 0) for c in (2, 3, 4, 5)}
# name -> (filled components only, every component): the issue's table, regenerated from the restatement
KNOWN = {
    "single_voxel": ({2: (0, 0)}, None),
    "solid_box": ({2: (0, 0)}, None),
    "ring": ({2: (1, 0)}, {1: (1, 1), 2: (1, 0)}),
    "slab_two_tunnels": ({2: (2, 0)}, {1: (2, 1), 2: (2, 0)}),
    "shell_with_cavity": ({2: (0, 1)}, {1: (0, 1), 2: (0, 1), 3: (0, 0)}),
    "cube_two_cavities": ({2: (0, 2)}, {1: (0, 1), 2: (0, 2), 3: (0, 0), 4: (0, 0)}),
    "two_voxels": ({2: (0, 0), 3: (0, 0)}, {1: (0, 2), 2: (0, 0), 3: (0, 0)}),
    "all_filled": ({1: (0, 0)}, {1: (0, 0)}),
    "tutorial": ({1: (0, 0)}, {1: (0, 0), 2: (0, 0)}),
    "convex_segments": (_CS_FILLED, {**_CS_FILLED, 2: (4, 0)}),
    "estimate_distance": (_ED_FILLED, {**_ED_FILLED, 1: (3, 0)}),
}


def shape_labels(name):
    m = SHAPES[name]()
    labels, _ = restated_labels(m)
    return m, labels


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    m, labels = shape_labels(name)
    filled, every = KNOWN[name]
    assert holes_voids(restated_counts(labels, select=m)) == filled
    if every is not None:
        assert holes_voids(restated_counts(labels)) == every


@pytest.mark.parametrize("name", ["single_voxel", "estimate_distance"])
def test_literal_reference_survives_these(name):
    m, labels = shape_labels(name)
    filled, every = KNOWN[name]
    assert holes_voids(restated_counts(labels, select=m, literal=True)) == filled
    if every is not None:
        assert holes_voids(restated_counts(labels, literal=True)) == every


@pytest.mark.parametrize("mask", [
    box_in((7, 7, 7), (2, 2, 2), (4, 4, 4)),             # a 2x2x2 box
    box_in((9, 9, 9), (2, 2, 2), (7, 7, 7)),             # a 5^3 box
    scenes.tutorial_scene()[0],
], ids=["box2", "box5", "tutorial"])
def test_literal_reference_throws_where_the_corrected_one_does_not(mask):
    """Deviation 1 (z + 1 read as z + 1): with the reference's z - 1, the vertices inside a component's upper-z face never enter
    the vertex set, and the search follows an exposed edge into one of them."""
    labels, _ = restated_labels(mask)
    with pytest.raises(WouldThrow):
        restated_counts(labels, select=mask, literal=True)
    got = holes_voids(restated_counts(labels, select=mask))
    assert all(v == (0, 0) for v in got.values()) and got


def test_convex_segments_literal_throws_for_every_filled_component():
    m, labels = shape_labels("convex_segments")
    for c in _CS_FILLED:
        with pytest.raises(WouldThrow):
            restated_counts(labels, select=(labels == c), literal=True)


def test_counts_of_a_single_voxel():
    _, labels = shape_labels("single_voxel")
    counts = restated_counts(labels, select=labels == 2)
    assert counts[2].tolist() == [8, 8, 0, 0, 1]         # the 8 corners, each with 3 exposed edges: raw = 1 + (0 - 8) / 8 = 0
    assert counts[1].tolist() == [0, 0, 0, 0, 0] and counts[0].tolist() == [0] * 5


def test_c_truncation_of_a_negative_sum():
    assert c_div(-7, 8) == 0 and c_div(-9, 8) == -1 and c_div(7, 8) == 0 and c_div(-16, 8) == -2
    assert c_div(-7, 8) == math.trunc(-7 / 8) and (-7) // 8 == -1            # floor division would be wrong here
    counts = np.zeros((2, 5), np.int64)
    counts[1] = [10, 7, 0, 0, 1]                         # M5 + 2 M6 - M3 = -7: raw = 1 + 0 = 1, not 1 + (-1)
    assert holes_voids(counts) == {1: (1, 0)}
    counts[1] = [12, 9, 0, 0, 2]                         # -9 / 8 = -1: raw 0, voids 1, holes 1
    assert holes_voids(counts) == {1: (1, 1)}


def test_selection_of_nothing_gives_an_empty_map():
    m, labels = shape_labels("ring")
    assert holes_voids(restated_counts(labels, select=np.zeros_like(m))) == {}


def test_label_above_max_label_is_refused():
    labels = np.full((3, 3, 3), 4, np.uint32)
    with pytest.raises(ValueError):
        restated_counts(labels, max_label=3)


def test_mixed_selection_label_can_throw_even_corrected():
    """A stale label 0 over both classes: the corrected rule's vertex set misses the unselected part (the GPU refuses it)."""
    m = box_in((7, 7, 7), (0, 0, 0), (3, 3, 3))             # (against the grid's faces, where label 0 meets "out of grid")
    labels = np.zeros(m.shape, np.uint32)
    with pytest.raises(WouldThrow):
        restated_counts(labels, select=m)


_HEADER_CHECK = r"""
#include <cstdio>
#include <map>
#include "sdf_tools/collision_map.hpp"
#include "sdf_tools/tagged_object_collision_map.hpp"

int main() {
    sdf_tools::CollisionMapGrid g("world", 1.0, 4, 4, 4, sdf_tools::COLLISION_CELL(0.0f));
    const std::map<uint32_t, std::pair<int32_t, int32_t>> a = g.ComputeComponentTopology(true, true, false);
    sdf_tools::TaggedObjectCollisionMapGrid t(Eigen::Isometry3d::Identity(), "world", 1.0, 4, 4, 4,
                                              sdf_tools::TAGGED_OBJECT_COLLISION_CELL(0.0f, 0u));
    const std::map<uint32_t, std::pair<int32_t, int32_t>> b =
        t.ComputeComponentTopology(sdf_tools::TaggedObjectCollisionMapGrid::FILLED_COMPONENTS, true, false);
    const uint8_t all = sdf_tools::CollisionMapGrid::FILLED_COMPONENTS | sdf_tools::CollisionMapGrid::EMPTY_COMPONENTS |
                        sdf_tools::CollisionMapGrid::UNKNOWN_COMPONENTS;
    std::printf("%zu %zu %u\n", a.size(), b.size(), (unsigned)all);
    return 0;
}
"""


def test_class_headers_compile_with_the_topology_methods(tmp_path):
    src = tmp_path / "topology_header_check.cpp"
    src.write_text(_HEADER_CHECK)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])
