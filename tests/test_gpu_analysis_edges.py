"""GPU: fixed inputs aimed at internal paths of the analysis kernels that the scene lists of the other suites do not reach, each
compared with its reference:
  k_tp_vertex's LDS table (sdfgpu_topology.hip): 17+ labels on one slot, more than 1024 labels in one workgroup (the spill to the
      global counters)                                                              -> restated_counts
  cc_plan's tiles (sdfgpu_components.hip): tile edges just inside / outside the grid, singleton axes, the thin-grid branch, one
      component chained through every tile face (serpentine, comb)                  -> restated_labels
  the full-field gradient (k_gradient_f32x4 up to the largest nx, the generic fallback, F32SCALE or not, nz % 4 != 0)
                                                                                    -> analysis_scenes.grid_gradient
  the extrema doubling (sdfgpu_convex.hip): gradient chains as long as the grid      -> restated_extrema, doubling_model's rounds
      (an upper bound: the kernel resolves in place)
Scenes and restatements: tests/analysis_scenes.py."""
import math

import numpy as np
import pytest
import torch

import analysis_scenes as A
from sdf_tools_amd import capi
from test_convex_segments_cpu import doubling_model, next_map
from test_gpu_components import _all_entry_points as components_all
from test_gpu_topology import _all_entry_points as topology_all

pytestmark = pytest.mark.gpu


# ---- topology: the per-workgroup label table ----------------------------------------------------------------------------------
def _topology_check(gpu, labels, max_label=None):
    labels = np.ascontiguousarray(labels, np.uint32)
    nv = (labels.shape[0] + 1) * (labels.shape[1] + 1) * (labels.shape[2] + 1)
    assert nv <= 8192                                                      # one workgroup (kTpChunk vertices) sees every label
    ref = topology_all(gpu, labels, None, max_label, np.zeros(labels.shape, np.float32), 7)
    assert ref[:, 0].sum() > 0
    return ref


def test_topology_labels_colliding_in_one_table_slot(gpu):
    rng = np.random.default_rng(1)
    for count in (17, 40, 200):
        col, slot = A.colliding_labels(count, start=int(rng.integers(1, 1000)))
        assert (A.table_slot(col) == slot).all() and len(np.unique(col)) == count
        labels = col[rng.integers(0, count, (11, 9, 13))]
        labels[0, 0, :count % 13] = col[-1]                                 # the largest label is max_label
        ref = _topology_check(gpu, labels, int(col.max()))
        present = np.unique(labels)
        assert (ref[present, 0] > 0).all()                                  # every colliding label has surface vertices
        # colliding labels beside ordinary ones, max_label above the largest label
        mixed = np.where(rng.random(labels.shape) < 0.5, labels, rng.integers(0, 50, labels.shape).astype(np.uint32))
        _topology_check(gpu, mixed, int(col.max()) + 3)


def test_topology_more_labels_than_table_slots(gpu):
    rng = np.random.default_rng(2)
    shape = (14, 14, 13)                                                    # 2548 voxels, 3150 vertices: one workgroup
    distinct = rng.permutation(np.arange(1, np.prod(shape) + 1, dtype=np.uint32)).reshape(shape)
    assert len(np.unique(distinct)) > A.TABLE_SLOTS
    _topology_check(gpu, distinct)
    # pairs of voxels along z per label (edges between voxels of one label), the colliding labels on top, still > 1024 labels
    pairs = distinct[:, :, ::2].repeat(2, 2)[:, :, :shape[2]].copy()
    col, _ = A.colliding_labels(32, start=5000)
    pairs[:2] = col[rng.integers(0, 32, pairs[:2].shape)]
    assert len(np.unique(pairs)) > A.TABLE_SLOTS + 32
    _topology_check(gpu, pairs, int(max(pairs.max(), col.max())))


@pytest.mark.parametrize("shape", [(2, 1, 1), (1, 1, 3), (3, 2, 1), (5, 3, 5)])
def test_topology_cell_records_of_tiny_grids(gpu, shape):
    """the cell form stages its labels through the pinned chunks even for a few bytes: a chunk shorter than the host team once
    went up unfilled (fuzz_analysis seed 1), so the kernel read stale labels"""
    from test_components_cpu import restated_labels
    from test_gpu_topology import _both_modes
    m = A.stripes(shape, 2)
    _both_modes(gpu, m)
    labels, k = restated_labels(m)
    topology_all(gpu, labels, m != 0, k + 17, m.astype(np.float32), capi.TOPOLOGY_FILLED)


# ---- components: the tile plan ------------------------------------------------------------------------------------------------
NZ = [1, 31, 32, 33, 63, 64, 65, 97]
NY = [1, 15, 16, 17]
NX = [1, 15, 16, 17, 31, 32, 33]


def _plan_shapes():
    out = []
    for i, nz in enumerate(NZ):
        for j, ny in enumerate(NY):
            out.append((NX[(i + 3 * j) % len(NX)], ny, nz))
    out += [(33, 17, 1), (17, 1, 65), (1, 33, 17), (65, 1, 1), (1, 97, 1), (1, 1, 97), (16, 16, 64), (32, 16, 32), (17, 16, 64)]
    return out


@pytest.mark.parametrize("shape", _plan_shapes())
def test_components_on_the_tile_plan(gpu, shape):
    for mask in (A.serpentine(shape), A.comb(shape, 0), A.comb(shape, 2), A.stripes(shape, 0), A.stripes(shape, 1),
                 A.stripes(shape, 2)):
        components_all(gpu, mask.astype(np.float32))


def test_components_long_chains_across_many_tiles(gpu):
    for shape in ((66, 34, 130), (17, 129, 97), (300, 3, 33)):
        for mask in (A.serpentine(shape), A.comb(shape, 0), A.comb(shape, 1), A.tori_chain(shape)):
            components_all(gpu, mask.astype(np.float32))


# ---- the full-field gradient ----------------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def _quantised(shape, seed):
    rng = np.random.default_rng(seed)
    f = (rng.integers(-40, 41, shape) * 0.125).astype(np.float32)
    f[rng.random(shape) < 0.02] = np.inf
    return f


def _device_gradient(gpu, f, res, edge, f64, in_shift=0, out_shift=0):
    """f on the device at a 4-byte shift from a 16-byte boundary (in_shift floats), output likewise; returns the host copy."""
    n = f.size
    fin = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    fin[in_shift:in_shift + n] = torch.from_numpy(f.reshape(-1)).cuda()
    dt, w = (torch.float64, 8) if f64 else (torch.float32, 4)
    out = torch.full((3 * n + 4,), -7.0, dtype=dt, device="cuda")
    gpu.gradient_device(fin.data_ptr() + 4 * in_shift, f.shape, out.data_ptr() + w * out_shift, res, edge, f64)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:out_shift] == -7.0).all() and (o[out_shift + 3 * n:] == -7.0).all()          # nothing written outside
    return o[out_shift:out_shift + 3 * n].reshape(f.shape + (3,))


@pytest.mark.parametrize("shape", [(16384, 2, 4), (16384, 3, 8), (16383, 3, 12)])
def test_gradient_vector_kernel_at_the_largest_accepted_nx(gpu, shape):
    """one x plane per blockIdx.y up to the largest nx check_dims accepts (16384): the vector kernel's loop over further planes
    (x += gridDim.y, nx > 65535) is out of reach of every entry point, which the next test pins"""
    f = _quantised(shape, 3)
    for res in (0.25, 0.03):                                                # F32SCALE and the fp64 scale
        for edge in (True, False):
            want = A.grid_gradient(f, res, edge)
            assert _same(_device_gradient(gpu, f, res, edge, False), want.astype(np.float32))
    assert _same(_device_gradient(gpu, f, 0.25, True, True), A.grid_gradient(f, 0.25, True))


def test_gradient_refuses_more_than_16384_planes(gpu):
    d = torch.zeros(64, dtype=torch.float32, device="cuda")
    for shape in ((65540, 2, 4), (16385, 1, 4)):
        with pytest.raises(capi.SdfGpuError) as e:
            gpu.gradient_device(d.data_ptr(), shape, d.data_ptr(), 0.25, True, False)
        assert e.value.code == -3


@pytest.mark.parametrize("shape", [(12, 9, 10), (10, 9, 16), (3, 5, 8), (1, 7, 12), (40, 33, 64), (2, 1, 16), (5, 2, 4), (9, 11, 7),
                                   (4, 4, 4), (1, 1, 9), (33, 17, 65)])
def test_gradient_restatement_every_path(gpu, shape):
    f = _quantised(shape, sum(shape))
    for res in (0.25, 0.01, 0.03, 0.007):
        for edge in (True, False):
            want = A.grid_gradient(f, res, edge)
            assert _same(_device_gradient(gpu, f, res, edge, True), want)
            want32 = want.astype(np.float32)
            for in_shift, out_shift in ((0, 0), (1, 0), (0, 1), (3, 2)):    # 16-byte aligned (vector kernel if nz % 4 == 0), or not
                assert _same(_device_gradient(gpu, f, res, edge, False, in_shift, out_shift), want32), (res, edge, in_shift, out_shift)


# ---- extrema: the doubling rounds ----------------------------------------------------------------------------------------------
def _ramp(n, two_cycle):
    v = np.arange(1, n + 1, dtype=np.float64)
    if two_cycle:                                           # f[n-3] < f[n-1] < f[n-2]: n-2 -> n-1 -> n-2, everything else flows in
        v[n - 2], v[n - 1] = n + 2, n
    return v


@pytest.mark.parametrize("n", [256, 257, 2048, 2049])
@pytest.mark.parametrize("two_cycle", [False, True])
def test_extrema_chain_as_long_as_the_grid(gpu, n, two_cycle):
    from test_gpu_convex_segments import _check_extrema
    for axis in (0, 1, 2):
        for res in (1.0, 0.05):
            shape = [1, 1, 1]
            shape[axis] = n
            f = (_ramp(n, two_cycle) * res).astype(np.float32).reshape(shape)
            idx = _check_extrema(gpu, f, res)
            rounds = gpu.convex_last_info()["rounds"]
            nxt = next_map(f, res)
            assert nxt[:n - 3] == list(range(1, n - 2))                    # one chain through the whole grid
            want, want_rounds = doubling_model(nxt)
            # k_cx_round also stores a node it resolves into its input, so later lanes of the same round may see it resolved: the GPU
            # needs at most the model's rounds (which resolve from the round's input alone), and the model at most ceil(log2 n) + 1
            assert 1 <= rounds <= want_rounds <= math.ceil(math.log2(n)) + 1, (rounds, want_rounds)
            if two_cycle:
                assert len(set(idx.reshape(-1).tolist())) == 1 and int(idx.reshape(-1)[0]) in (n - 2, n - 1)
            else:
                assert (idx == 0xFFFFFFFF).all()                           # the walk leaves the grid at its far end
            assert [v if v >= 0 else 0xFFFFFFFF for v in want] == idx.reshape(-1).tolist()
