"""Without a GPU: the scenes of tests/analysis_scenes.py are what they claim (one serpentine component, a comb joined only at its
end, colliding table labels), and its vectorised gradient / estimate restatements equal the loop forms and the host headers'
GetGradient / EstimateDistance.  tests/test_gpu_analysis_edges.py and tools/fuzz_analysis.py compare the GPU with them."""
import math

import numpy as np
import pytest

import analysis_scenes as A
from sdf_tools_amd import synth
from sdf_tools_amd._bindings import load_pysdf_tools
from test_components_cpu import restated_labels
from test_gpu_streaming import _numpy_estimate_distance
from test_topology_cpu import holes_voids, restated_counts

SHAPES = [(1, 1, 1), (1, 1, 33), (1, 17, 1), (33, 1, 1), (3, 16, 65), (17, 15, 31), (32, 17, 64), (2, 33, 97)]


@pytest.mark.parametrize("shape", SHAPES)
def test_serpentine_is_one_component_through_the_grid(shape):
    m = A.serpentine(shape)
    assert filled_components(m) == 1
    nx, ny, nz = shape
    assert m[::2, ::2, :].all()                                            # every row of the walk is in it
    assert m.sum() == len(range(0, nx, 2)) * len(range(0, ny, 2)) * nz + len(range(0, nx, 2)) * len(range(0, ny, 2)) - 1 \
        or nz == 1                                                          # rows plus one joint between consecutive rows


def filled_components(m):
    """components of the filled voxels (the labelling numbers free components too)"""
    labels, _ = restated_labels(m)
    return len(np.unique(labels[m != 0]))


@pytest.mark.parametrize("shape", [s for s in SHAPES if max(s) > 1])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_comb_joins_only_at_the_far_end(shape, axis):
    m = A.comb(shape, axis)
    assert filled_components(m) == 1
    teeth = A.stripes(shape, axis)
    k_teeth = filled_components(teeth)
    others = [s for a, s in enumerate(shape) if a != axis]
    assert k_teeth == len(range(0, others[0], 2)) * len(range(0, others[1], 2))     # one component per tooth
    sl = [slice(None)] * 3
    sl[axis] = slice(0, shape[axis] - 1)
    if shape[axis] > 1:
        assert np.array_equal(m[tuple(sl)], teeth[tuple(sl)])             # the teeth touch nothing before the last plane


def test_checkerboard_nested_shells_and_tori():
    assert restated_labels(A.checkerboard((5, 4, 3)))[1] == 60              # every voxel its own component
    m = A.nested_shells((12, 11, 10))
    labels, k = restated_labels(m)
    assert k == 3 and filled_components(m) == 2                              # shell, cavity, core
    hv = holes_voids(restated_counts(labels, select=m, max_label=k))
    assert sorted(hv.values()) == [(0, 0), (0, 1)]                          # the shell: no hole, one void (the cavity); the core: none
    t = A.tori_chain((40, 16, 16))
    assert filled_components(t) == 36                                        # rings at x = 0, 4, ..., 32; chains at y, z in {3, 12}
    labels, k = restated_labels(t)
    hv = holes_voids(restated_counts(labels, select=t, max_label=k))
    assert len(hv) == 36 and set(hv.values()) == {(1, 0)}                    # every ring: one hole, no void


def test_colliding_labels_collide():
    labels, slot = A.colliding_labels(40, start=3)
    assert len(set(labels.tolist())) == 40 and labels.min() >= 3
    for c in labels.tolist():
        assert ((c * 2654435761) % (1 << 32)) >> 22 == slot                # the kernel's uint32 product, top 10 bits
    assert A.table_slot(np.array([5, 6])).max() < A.TABLE_SLOTS


def _loop_gradient(sdf, res, edge):
    """test_gpu_slab.py's per-voxel loop form of GetGridAlignedGradient (sdf.hpp:432-526)."""
    shape = sdf.shape
    want = np.zeros(shape + (3,), np.float64)
    nx, ny, nz = shape
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                interior = 0 < x < nx - 1 and 0 < y < ny - 1 and 0 < z < nz - 1
                idx = [x, y, z]
                for ax, n in enumerate(shape):
                    lo, hi = list(idx), list(idx)
                    if interior:
                        lo[ax] -= 1
                        hi[ax] += 1
                        want[x, y, z, ax] = float(np.float32(sdf[tuple(hi)] - sdf[tuple(lo)])) * (1.0 / (2.0 * res))
                    elif not edge:
                        want[x, y, z, ax] = math.nan
                    else:
                        lo[ax] = max(0, idx[ax] - 1)
                        hi[ax] = min(n - 1, idx[ax] + 1)
                        inc = (hi[ax] - lo[ax]) * res
                        if inc > 0:
                            want[x, y, z, ax] = (float(sdf[tuple(hi)]) - float(sdf[tuple(lo)])) * (1.0 / inc)
    return want


def _host_field(sdf, res, origin=None):
    m = load_pysdf_tools()
    s = m.SignedDistanceField(m.Isometry3d(np.eye(4) if origin is None else origin), "world", float(res), *sdf.shape, math.inf)
    s.SetRawDataNumpy(np.ascontiguousarray(sdf, np.float32))
    return s


def _field(shape, seed):
    rng = np.random.default_rng(seed)
    f = (rng.integers(-6, 7, shape) * 0.25).astype(np.float32)             # quantised: many exact ties
    f[rng.random(shape) < 0.05] = np.inf
    return f


@pytest.mark.parametrize("shape", [(12, 9, 10), (1, 7, 12), (5, 2, 4), (3, 1, 1), (6, 5, 8)])
@pytest.mark.parametrize("res", [0.25, 0.03])
def test_grid_gradient_equals_loop_form_and_host(shape, res):
    f = _field(shape, sum(shape))
    host = _host_field(f, res)
    for edge in (True, False):
        got = A.grid_gradient(f, res, edge)
        assert np.array_equal(got.view(np.uint64), _loop_gradient(f, res, edge).view(np.uint64))
        for x, y, z in np.ndindex(*shape):
            h = host.GetGradient(x, y, z, edge)
            if len(h) == 3 and np.isfinite(got[x, y, z]).all():           # (the identity rotation turns inf into NaN)
                assert np.array_equal(np.asarray(h, np.float64).view(np.uint64), got[x, y, z].view(np.uint64))
            elif len(h) != 3:
                assert np.isnan(got[x, y, z]).all()


@pytest.mark.parametrize("shape", [(12, 9, 10), (1, 7, 12), (2, 1, 5), (1, 1, 1)])
@pytest.mark.parametrize("res", [1.0, 0.037])
def test_estimate_distance_equals_loop_form_and_host(shape, res):
    f = synth.bernoulli_mask(shape, 0.3, 5).astype(np.float32) * -2.0 + 1.0       # +1 free, -1 filled
    f *= np.float32(res) * np.arange(1, f.size + 1, dtype=np.float32).reshape(shape) % 7
    rng = np.random.default_rng(2)
    size = np.asarray(shape, np.float64) * res
    g = np.concatenate([rng.uniform(0.0, 1.0, (500, 3)) * size * (1 - 1e-12),
                        (np.argwhere(np.ones(shape)) + 0.5) * res,                   # cell centres (offset exactly 0)
                        np.argwhere(np.ones(shape)) * res])                          # cell corners
    vec = A.estimate_distance(f, res, g)
    loop = _numpy_estimate_distance(f, res, g)
    assert np.array_equal(vec.view(np.uint64), loop.view(np.uint64))
    host = _host_field(f, res)
    d, grad, flags = A.query_points(f, res, g, oob=7.0, edge=True)
    assert np.array_equal(d.view(np.uint64), vec.view(np.uint64)) and (flags == 3).all()
    for k in range(len(g)):
        est, ok = host.EstimateDistance(*g[k])
        assert ok and np.float64(est).view(np.uint64) == vec[k].view(np.uint64)
    out = A.query_points(f, res, np.array([[-1e-9, 0.0, 0.0], [0.0, size[1], 0.0], [np.nan, 0.0, 0.0]]), oob=7.0)
    assert (out[0] == 7.0).all() and np.isnan(out[1]).all() and (out[2] == 0).all()
