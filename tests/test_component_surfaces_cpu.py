"""Component surfaces without a GPU: the numpy restatement (tests/component_surfaces_restated.py) against a per-voxel
transliteration of the reference's loops (collision_map.cpp:697-754 over collision_map.hpp:93-154 and
topology_computation.hpp:298-324) in corrected mode and against hand counts, the evidence that the reference's literal argument
order and face test differ from the corrected ones, and the class headers' new methods (compile check, CheckIfCandidateCorner
through a compiled harness on stored labels).  tests/test_gpu_component_surfaces.py compares the GPU with the same restatement."""
import os
import subprocess

import numpy as np
import pytest

from component_surfaces_restated import EMPTY, FILLED, UNKNOWN, as_map, class_select, restated_surfaces, surface_mask

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def transliterated(labels, occ, types, literal=False, oob_component=0):
    """The reference's x -> y -> z loop, one voxel at a time: {label: [linear indices in insertion order]}.
    literal: IsConnectedComponentSurfaceIndex is called at (x, y, y) for filled and (x, z, z) for unknown voxels, its face test
    compares z with nz (not nz - 1), and an out-of-grid neighbour has the OOB cell's component.  Corrected: (x, y, z), nz - 1, -1."""
    nx, ny, nz = labels.shape

    def component(x, y, z):
        if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz:
            return int(labels[x, y, z])
        return oob_component if literal else -1

    def is_surface(x, y, z):
        if x < 0 or y < 0 or z < 0 or x >= nx or y >= ny or z >= nz:
            return False
        if x == 0 or y == 0 or z == 0 or x == nx - 1 or y == ny - 1 or z == (nz if literal else nz - 1):
            return True
        ours = component(x, y, z)
        for dx, dy, dz in ((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)):
            if ours != component(x + dx, y + dy, z + dz):
                return True
        return False

    out = {}
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                o = np.float32(occ[x, y, z])
                if o > 0.5:
                    hit = (types & FILLED) and (is_surface(x, y, y) if literal else is_surface(x, y, z))
                elif o < 0.5:
                    hit = (types & EMPTY) and is_surface(x, y, z)
                else:
                    hit = (types & UNKNOWN) and (is_surface(x, z, z) if literal else is_surface(x, y, z))
                if hit:
                    out.setdefault(int(labels[x, y, z]), []).append((x * ny + y) * nz + z)
    return out


def _groups(counts, indices):
    out, start = {}, 0
    for c, k in enumerate(counts.tolist()):
        if k:
            out[c] = indices[start:start + k].tolist()
        start += k
    return out


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 4, 1), (3, 3, 3), (4, 5, 3), (6, 5, 7)])
@pytest.mark.parametrize("types", [1, 2, 4, 3, 5, 7])
def test_restatement_matches_the_transliterated_loops(shape, types):
    rng = np.random.default_rng(sum(shape) * 8 + types)
    for k in (1, 3, 40):
        labels = rng.integers(0, k + 1, size=shape).astype(np.uint32)
        occ = rng.choice(np.array([0.0, 0.25, 0.5, 0.50000006, 1.0, np.nan], np.float32), size=shape)
        counts, idx, rep = restated_surfaces(labels, class_select(occ, types), k)
        assert _groups(counts, idx) == transliterated(labels, occ, types)
        assert counts.sum() == len(idx) == rep.sum() and len(counts) == k + 1
        for c, g in _groups(counts, idx).items():
            assert g == sorted(g) and (labels.reshape(-1)[g] == c).all()


def test_hand_counts():
    counts, idx, _ = restated_surfaces(np.zeros((1, 1, 1), np.uint32))
    assert counts.tolist() == [1] and idx.tolist() == [0]

    counts, idx, rep = restated_surfaces(np.full((5, 5, 5), 2, np.uint32))
    assert counts.tolist() == [0, 0, 98] and not rep[1:4, 1:4, 1:4].any()        # 125 - 27 boundary voxels

    labels = np.full((7, 7, 7), 2, np.uint32)
    labels[2:5, 2:5, 2:5] = 1                                                   # filled box 1 in free space 2
    counts, idx, rep = restated_surfaces(labels)
    shell = 6 * 9                                                               # free voxels sharing a face with the box
    # The box: 26, not 27.  Its centre voxel (3, 3, 3) has the six face centres of the box as its face neighbours, all of
    # label 1, so by the contract (and by the reference's six comparisons) it is not a surface voxel; the other 26 touch label 2.
    assert counts.tolist() == [0, 26, (7 ** 3 - 5 ** 3) + shell] and 7 ** 3 - 5 ** 3 == 218
    assert rep[2:5, 2:5, 2:5].sum() == 26 and not rep[3, 3, 3]
    assert transliterated(labels, (labels == 1).astype(np.float32), 7) == _groups(counts, idx)

    x, y, z = np.meshgrid(*[np.arange(2)] * 3, indexing="ij")
    labels = (4 * x + 2 * y + z).astype(np.uint32)                             # 2 x 2 x 2, eight labels
    counts, idx, _ = restated_surfaces(labels)
    assert counts.tolist() == [1] * 8 and idx.tolist() == list(range(8))
    checker = ((x + y + z) % 2).astype(np.uint32)
    counts, idx, _ = restated_surfaces(checker)
    assert counts.tolist() == [4, 4] and sorted(idx.tolist()) == list(range(8))


def test_literal_argument_order_differs_on_a_named_shape():
    """A filled plate, one voxel thick, at z = 5 of a 6 x 5 x 7 grid: x in 1..4, y in 1..3 (label 2 in free space 1).  Every
    plate voxel faces free space, so the corrected loop reports all 12.  The literal loop asks IsConnectedComponentSurfaceIndex
    about (x, y, y) instead: (x, 1, 1), (x, 2, 2), (x, 3, 3), interior free voxels whose six neighbours are free as well -- it
    reports none of the plate."""
    shape = (6, 5, 7)
    occ = np.zeros(shape, np.float32)
    occ[1:5, 1:4, 5] = 1.0
    labels = np.where(occ > 0.5, 2, 1).astype(np.uint32)
    corrected = transliterated(labels, occ, FILLED)
    literal = transliterated(labels, occ, FILLED, literal=True)
    assert len(corrected[2]) == 12                                             # every plate voxel faces free space
    assert literal != corrected
    assert 2 not in literal                                                    # tested at (x, y, y): free space all around
    counts, idx, _ = restated_surfaces(labels, occ > 0.5, 2)
    assert _groups(counts, idx) == corrected

    # the unknown class at (x, z, z), and the z = nz - 1 face that the literal face test (z == nz) never sees
    occ = np.full(shape, 0.5, np.float32)
    labels = np.ones(shape, np.uint32)
    corrected = transliterated(labels, occ, UNKNOWN)
    literal = transliterated(labels, occ, UNKNOWN, literal=True, oob_component=1)
    assert len(corrected[1]) == 6 * 5 * 7 - 4 * 3 * 5
    assert literal != corrected and (2 * 5 + 2) * 7 + 6 in corrected[1] and (2 * 5 + 2) * 7 + 6 not in literal.get(1, [])


_HEADER_CHECK = r"""
#include "sdf_tools/collision_map.hpp"
#include "sdf_tools/tagged_object_collision_map.hpp"

template <typename Grid>
size_t use(const Grid& g) {
    using Surfaces = std::map<uint32_t, std::unordered_map<VoxelGrid::GRID_INDEX, uint8_t>>;
    const Surfaces a = g.ExtractComponentSurfaces(Grid::FILLED_COMPONENTS);
    const Surfaces b = g.ExtractFilledComponentSurfaces();
    const Surfaces c = g.ExtractUnknownComponentSurfaces();
    const Surfaces d = g.ExtractEmptyComponentSurfaces();
    const sdf_tools::ComponentSurfaceIndices e = g.ExtractComponentSurfaceIndices((typename Grid::COMPONENT_TYPES)7);
    const std::pair<bool, bool> p0 = g.CheckIfCandidateCorner3d(Eigen::Vector3d(0.0, 0.0, 0.0));
    const std::pair<bool, bool> p1 = g.CheckIfCandidateCorner4d(Eigen::Vector4d(0.0, 0.0, 0.0, 1.0));
    const std::pair<bool, bool> p2 = g.CheckIfCandidateCorner(0.0, 0.0, 0.0);
    const std::pair<bool, bool> p3 = g.CheckIfCandidateCorner(VoxelGrid::GRID_INDEX(0, 0, 0));
    const std::pair<bool, bool> p4 = g.CheckIfCandidateCorner((int64_t)0, (int64_t)0, (int64_t)0);
    return a.size() + b.size() + c.size() + d.size() + e.indices.size() + e.offsets.size() + p0.first + p1.first + p2.first + p3.first + p4.second;
}

int main() {
    const sdf_tools::CollisionMapGrid g("world", 1.0, 4, 4, 4, sdf_tools::COLLISION_CELL(0.0f));
    const sdf_tools::TaggedObjectCollisionMapGrid t("world", 1.0, 4, 4, 4, sdf_tools::TAGGED_OBJECT_COLLISION_CELL(0.0f, 0u));
    return (int)(use(g) + use(t));
}
"""


def test_class_headers_compile_with_the_surface_methods(tmp_path):
    src = tmp_path / "surfaces_header_check.cpp"
    src.write_text(_HEADER_CHECK)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])


_CORNER_HARNESS = r"""
#include <cstdio>
#include "sdf_tools/collision_map.hpp"
#include "sdf_tools/tagged_object_collision_map.hpp"

// stored labels: component 2 fills x < 3 and the part of x >= 3 with y < 3 (an L-shaped solid), component 1 is the free corner
template <typename Grid>
void run(const char* tag, Grid& g) {
    for (int64_t x = 0; x < 6; ++x)
        for (int64_t y = 0; y < 6; ++y)
            for (int64_t z = 0; z < 6; ++z)
                g.GetMutable(x, y, z).first.component = (x < 3 || y < 3) ? 2u : 1u;
    const auto corner = g.CheckIfCandidateCorner((int64_t)3, (int64_t)3, (int64_t)2);        // free, solid at x - 1 and at y - 1
    const auto face = g.CheckIfCandidateCorner(VoxelGrid::GRID_INDEX(3, 5, 2));              // free, solid at x - 1 only
    const auto inside = g.CheckIfCandidateCorner((int64_t)1, (int64_t)1, (int64_t)1);
    const auto outside = g.CheckIfCandidateCorner((int64_t)6, (int64_t)0, (int64_t)0);
    const auto by_location = g.CheckIfCandidateCorner(3.5, 3.5, 2.5);                        // the corner cell, resolution 1
    const auto loc3 = g.CheckIfCandidateCorner3d(Eigen::Vector3d(3.5, 5.5, 2.5));
    const auto loc4 = g.CheckIfCandidateCorner4d(Eigen::Vector4d(-0.5, 0.5, 0.5, 1.0));
    std::printf("%s %d%d %d%d %d%d %d%d %d%d %d%d %d%d\n", tag, corner.first, corner.second, face.first, face.second, inside.first,
                inside.second, outside.first, outside.second, by_location.first, by_location.second, loc3.first, loc3.second, loc4.first,
                loc4.second);
}

int main() {
    sdf_tools::CollisionMapGrid g("world", 1.0, 6, 6, 6, sdf_tools::COLLISION_CELL(0.0f));
    sdf_tools::TaggedObjectCollisionMapGrid t("world", 1.0, 6, 6, 6, sdf_tools::TAGGED_OBJECT_COLLISION_CELL(0.0f, 0u));
    run("cmg", g);
    run("tag", t);
    return 0;
}
"""


def test_check_if_candidate_corner(tmp_path):
    from sdf_tools_amd import build as B

    src = tmp_path / "corner_harness.cpp"
    src.write_text(_CORNER_HARNESS)
    exe = str(tmp_path / "corner_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe, "-L", B.PKG, "-lsdfgpu", "-Wl,-rpath," + B.PKG, "-lz"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    # corner (true, true); flat face (false, true); interior (false, true); out of grid (false, false); the location overloads
    want = "11 01 01 00 11 01 00"
    assert r.stdout.splitlines() == ["cmg " + want, "tag " + want]


def test_as_map_groups_by_label():
    labels = np.zeros((2, 3, 4), np.uint32)
    labels[1] = 5
    counts, idx, _ = restated_surfaces(labels)
    m = as_map(counts, idx, labels.shape)
    assert sorted(m) == [0, 5] and m[5] == {(1, y, z) for y in range(3) for z in range(4)}
