"""The object contours on the MI355X (sdfgpu_display_select_contour*, include/sdfgpu.h "Display export: contours"):
every result bit-equal to tests/contour_restated.py::by_neighbours, through the host and the device entry points.

k_dp_contour works on wave rounds of 64 consecutive cells: shapes whose rows are whole waves ((3, 3, 64), (2, 2, 128)), shapes where
many rows meet in one round ((33, 1, 5), (1, 33, 5), (4, 5, 3)), and (17, 16, 33), which puts neighbourhoods across an edge of the
4096-voxel tiles, run beside the display export's own shapes.  The cross-check builds the reference's per-object SDFs on the GPU
and applies its literal threshold in numpy.  Grids past 2^31 voxels: tests/test_gpu_contour_large.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import contour_cases as K
import contour_restated as CR
import display_cases as C
import display_restated as R
from sdf_tools_amd import capi
from test_gpu_display import ISSUE_SHAPES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ISSUE_SHAPES + [(3, 3, 64), (2, 2, 128), (33, 1, 5), (1, 33, 5), (4, 5, 3)]


def _noise(rng, shape, filled=0.0):
    occ = rng.choice(C.OCC_VALUES, size=shape)
    if filled:
        occ = np.where(rng.random(shape) < filled, np.float32(1.0), occ).astype(np.float32)
    return occ


@pytest.mark.parametrize("shape", SHAPES)
def test_contour_rule(gpu, shape):
    rng = np.random.default_rng(sum(shape) + 7)
    pool = np.array([0, 1, 2, 300], np.uint32)
    for s, filled in enumerate((0.0, 0.9)):
        occ = _noise(rng, shape, filled)
        keys = rng.choice(pool, size=shape)
        if filled:                                              # two objects in slabs: interiors, a contact face, ids 0 beside them
            keys = np.where(np.arange(shape[2])[None, None, :] * 2 < shape[2], 1, 300).astype(np.uint32) * np.ones(shape, np.uint32)
            keys[rng.random(shape) < 0.05] = 0
        for reach in range(4):
            for uif in (True, False):
                full = reach == 3 and uif
                K.check(gpu, occ, keys, reach, unknown_is_filled=uif, draw_zero=bool(s),
                        layouts=K.LAYOUTS if full else (K.LAYOUTS[(reach + uif) % 3],), forms=("host", "device") if full else (("host", "device")[uif],))
        K.check(gpu, occ, keys, 3, draw_keys=[1, 300], layouts=K.LAYOUTS[1:2], forms=("device",))
        K.check(gpu, occ, keys, 2, draw_keys=[2, 77, 300], draw_zero=True, layouts=K.LAYOUTS[2:], forms=("host",))
        K.check(gpu, occ, keys, 3, draw_keys=[], layouts=K.LAYOUTS[:1], forms=("device",))


def _scene(shape, fill=0.0, key=0):
    return np.full(shape, fill, np.float32), np.full(shape, key, np.uint32)


def _drawn(gpu, occ, keys, reach, **opts):
    idx, k = K.check(gpu, occ, keys, reach, layouts=K.LAYOUTS[1:2], **opts)
    out = np.zeros(occ.size, bool)
    out[idx] = True
    return out.reshape(occ.shape)


def test_constructed_scenes(gpu):
    # a solid 6^3 box inside 8^3: a shell exactly one cell thick, at every reach >= 1
    occ, keys = _scene((8, 8, 8))
    occ[1:7, 1:7, 1:7], keys[1:7, 1:7, 1:7] = 1.0, 5
    shell = np.zeros(occ.shape, bool)
    shell[1:7, 1:7, 1:7] = True
    shell[2:6, 2:6, 2:6] = False
    for reach in (1, 2, 3):
        assert np.array_equal(_drawn(gpu, occ, keys, reach), shell)
    assert not _drawn(gpu, occ, keys, 0).any()
    # a slab over the grid's full x-y section draws only its two z faces
    occ, keys = _scene((5, 6, 70))
    occ[:, :, 3:68], keys[:, :, 3:68] = 1.0, 9
    d = _drawn(gpu, occ, keys, 3)
    assert d[:, :, 3].all() and d[:, :, 67].all() and d.sum() == 2 * 30
    # an object that fills the grid draws nothing
    occ, keys = _scene((9, 9, 33), 1.0, 4)
    assert not _drawn(gpu, occ, keys, 3).any()
    # only a corner neighbour is foreign: drawn at reach 3, not at 2; only an edge neighbour: at 2, not at 1
    occ, keys = _scene((5, 5, 5), 1.0, 4)
    occ[0, 0, 0] = 0.0
    assert _drawn(gpu, occ, keys, 3)[1, 1, 1] and not _drawn(gpu, occ, keys, 2)[1, 1, 1]
    occ, keys = _scene((5, 5, 5), 1.0, 4)
    occ[0, 0, :] = 0.0
    d2, d1 = _drawn(gpu, occ, keys, 2), _drawn(gpu, occ, keys, 1)
    assert d2[1, 1, 2] and not d1[1, 1, 2] and d1[1, 0, 2] and d1[0, 1, 2]
    # two abutting objects both draw their contact faces; one fills the grid's low half, the other the high half
    occ, keys = _scene((6, 6, 6), 1.0, 1)
    keys[3:] = 2
    d = _drawn(gpu, occ, keys, 1)
    assert d[2].all() and d[3].all() and d.sum() == 72
    # a listed id beside an unlisted one is drawn; the unlisted cells never
    d = _drawn(gpu, occ, keys, 3, draw_keys=[2])
    assert d[3].all() and d.sum() == 36
    # own-id cells with occupancy < 0.5 or NaN count as foreign; 0.5 only without unknown_is_filled
    for value, uif, foreign in ((0.25, True, True), (np.nan, True, True), (0.5, True, False), (0.5, False, True)):
        occ, keys = _scene((5, 5, 5), 1.0, 4)
        occ[2, 2, 2] = value
        d = _drawn(gpu, occ, keys, 3, unknown_is_filled=uif)
        assert d.sum() == (26 if foreign else 0) and not d[2, 2, 2]


def test_sort_passes_none_and_four(gpu):
    rng = np.random.default_rng(3)
    shape = (17, 16, 33)
    occ = _noise(rng, shape, 0.5)
    keys = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)        # 32 differing bits: four passes
    keys.reshape(-1)[:2] = (1, 2 ** 32 - 1)
    occ.reshape(-1)[:2] = 1.0
    idx, k = K.check(gpu, occ, keys, 3)
    assert len(np.unique(k)) > 3000 and k.min() == 1 and k.max() == 2 ** 32 - 1
    idx, k = K.check(gpu, occ, np.full(shape, 2 ** 32 - 1, np.uint32), 3)                   # one key: nothing to sort
    assert len(idx) > 1000 and len(np.unique(k)) == 1


def test_capacity_and_sentinels(gpu):
    rng = np.random.default_rng(5)
    shape = (9, 9, 33)
    occ = _noise(rng, shape, 0.6)
    keys = rng.choice(np.array([1, 3, 300, 70000], np.uint32), size=shape)
    layout = K.LAYOUTS[1]
    cells = R.cells_of(occ, keys, layout[0], layout[2], layout[1])
    want = K.reference(occ, keys, 3, True)
    total, groups = len(want[0]), len(want[2])
    assert total > 500 and groups == 4
    d_cells = C.dev(cells)
    args = (d_cells.data_ptr(), shape, 3) + layout
    assert gpu.display_select_contour_device(*args) == (total, 0)                          # count-only
    for grouped in (False, True):
        for cap in (total - 1, 0):
            idx, k, gk, go = C.words(total), C.words(total), C.words(groups), C.words(groups + 1)
            with pytest.raises(capi.SdfGpuError) as e:
                gpu.display_select_contour_device(*args, grouped=grouped, d_indices=idx.data_ptr(), d_keys=k.data_ptr(), capacity=cap,
                                                  d_group_keys=gk.data_ptr(), d_group_offsets=go.data_ptr(), group_capacity=groups)
            assert e.value.code == -1 and e.value.total == total and "drawn" in str(e.value)
            for t in (idx, k, gk, go):
                assert (t.cpu().numpy().view(np.uint32) == C.SENTINEL).all(), "a refused call stored results"
            with pytest.raises(capi.SdfGpuError) as e:
                gpu.display_select_contour(cells, shape, 3, *layout, grouped=grouped, capacity=cap)
            assert e.value.code == -1 and e.value.total == total
        # total and total + 1: the results, and nothing behind them
        for cap in (total, total + 1):
            idx, k, gk, go = C.words(cap), C.words(cap), C.words(groups), C.words(groups + 1)
            t, g = gpu.display_select_contour_device(*args, grouped=grouped, d_indices=idx.data_ptr(), d_keys=k.data_ptr(), capacity=cap,
                                                     d_group_keys=gk.data_ptr(), d_group_offsets=go.data_ptr(), group_capacity=groups)
            assert t == total and g == (groups if grouped else 0)
            ref = want if grouped else K.reference(occ, keys, 3, False)
            assert np.array_equal(C.host_words(idx, cap)[:total], ref[0]) and np.array_equal(C.host_words(k, cap)[:total], ref[1])
            assert (idx.cpu().numpy().view(np.uint32)[total:] == C.SENTINEL).all()
            got = gpu.display_select_contour(cells, shape, 3, *layout, grouped=grouped, capacity=cap)
            C.same("host form, capacity %d" % cap, got, ref)
    idx, k, gk, go = C.words(total), C.words(total), C.words(groups - 1), C.words(groups)
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.display_select_contour_device(*args, grouped=True, d_indices=idx.data_ptr(), d_keys=k.data_ptr(), capacity=total,
                                          d_group_keys=gk.data_ptr(), d_group_offsets=go.data_ptr(), group_capacity=groups - 1)
    assert e.value.code == -1 and (e.value.total, e.value.groups) == (total, groups)
    assert (gk.cpu().numpy().view(np.uint32) == C.SENTINEL).all() and (go.cpu().numpy().view(np.uint32) == C.SENTINEL).all()
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.display_select_contour(cells, shape, 3, *layout, grouped=True, group_capacity=groups - 1)
    assert (e.value.total, e.value.groups) == (total, groups)


def test_refusals(gpu):
    d = torch.zeros(128, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.display_select_contour_device(d.data_ptr(), (65536, 65536, 1), 3)                # 2^32 voxels: refused by shape alone
    assert e.value.code == -1 and "2^32 - 1 voxels" in str(e.value)
    assert torch.cuda.mem_get_info()[0] == before, "a call refused by its shape allocated device memory"
    shape = (2, 3, 4)
    cells = R.cells_of(np.ones(shape, np.float32), np.ones(shape, np.uint32), 16, 8)
    out = C.words(24)
    base = dict(shape=shape, reach=3, cell_stride=16, occupancy_offset=0, key_offset=8)
    for bad in (dict(reach=-1), dict(reach=4), dict(key_offset=16), dict(key_offset=6), dict(cell_stride=6, key_offset=0), dict(occupancy_offset=16),
                dict(occupancy_offset=2), dict(draw_keys=[3, 2]), dict(shape=(2, 3, 0)), dict(shape=(2, -3, 4)), dict(capacity=-1)):
        o = dict(dict(base, capacity=24), **bad)
        with pytest.raises(capi.SdfGpuError) as e:
            gpu.display_select_contour_device(d.data_ptr(), o.pop("shape"), o.pop("reach"), d_indices=out.data_ptr(), **o)
        assert e.value.code == -1, bad
        if "reach" in bad:
            assert "reach" in str(e.value)
        if "shape" not in bad and "cell_stride" not in bad:       # the host form checks the same arguments
            o = dict(base, **bad)
            with pytest.raises(capi.SdfGpuError) as e:
                gpu.display_select_contour(cells, o.pop("shape"), o.pop("reach"), **o)
            assert e.value.code == -1, bad
    # the grouped form without its arrays; misaligned device pointers; null records
    with pytest.raises(capi.SdfGpuError):
        gpu.display_select_contour_device(d.data_ptr(), shape, 3, grouped=True, d_indices=out.data_ptr(), capacity=24)
    for kw in (dict(d_indices=out.data_ptr() + 2), dict(d_indices=out.data_ptr(), d_keys=out.data_ptr() + 1)):
        with pytest.raises(capi.SdfGpuError) as e:
            gpu.display_select_contour_device(d.data_ptr(), shape, 3, capacity=8, **kw)
        assert "aligned" in str(e.value)
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.display_select_contour_device(d.data_ptr() + 2, shape, 3)
    assert "aligned" in str(e.value)
    with pytest.raises(capi.SdfGpuError):
        gpu.display_select_contour_device(0, shape, 3)
    assert (out.cpu().numpy().view(np.uint32) == C.SENTINEL).all(), "a refused call stored results"


def test_pointers_four_bytes_off_alignment(gpu):
    """records and every result array 4 bytes past a 16-byte boundary"""
    rng = np.random.default_rng(11)
    shape = (9, 9, 33)
    occ = _noise(rng, shape, 0.7)
    keys = rng.choice(np.array([1, 3, 300, 2 ** 32 - 1], np.uint32), size=shape)
    for layout in K.LAYOUTS:
        cells = R.cells_of(occ, keys, layout[0], layout[2], layout[1])
        want = K.reference(occ, keys, 3, True)
        total, groups = len(want[0]), len(want[2])
        raw = torch.zeros(cells.nbytes + 32, dtype=torch.uint8, device="cuda")
        off = (-raw.data_ptr()) % 16 + 4
        raw[off:off + cells.nbytes] = torch.from_numpy(cells.view(np.uint8).reshape(-1).copy()).cuda()
        bufs = [torch.full((count + 9,), C.SENTINEL, dtype=torch.int32, device="cuda") for count in (total, total, groups, groups + 1)]
        ptrs = [b.data_ptr() + ((-b.data_ptr()) % 16) + 4 for b in bufs]
        assert all(p % 16 == 4 for p in ptrs) and (raw.data_ptr() + off) % 16 == 4
        t, g = gpu.display_select_contour_device(raw.data_ptr() + off, shape, 3, *layout, grouped=True, d_indices=ptrs[0], d_keys=ptrs[1], capacity=total,
                                                 d_group_keys=ptrs[2], d_group_offsets=ptrs[3], group_capacity=groups)
        assert (t, g) == (total, groups)
        for b, p, w, count in zip(bufs, ptrs, want, (total, total, groups, groups + 1)):
            words = b.cpu().numpy().view(np.uint32)
            first = (p - b.data_ptr()) // 4
            assert np.array_equal(words[first:first + count], w)
            assert (words[:first] == C.SENTINEL).all() and (words[first + count:] == C.SENTINEL).all()


# ---- the reference's recipe on the GPU: per-object SDFs and the literal threshold -----------------------------------------------------
def _accepted_resolutions():
    """0.05 and one resolution per reach value among those sdfgpu_build_tagged_objects accepts (finite and > 0:
    tests/test_gpu_resolution_domain.py)"""
    out = [0.05, 2.0 ** -140, 2.0 ** -149, 1.5 * 2.0 ** 127, 2.0 ** -160]
    assert [CR.reach(r) for r in out] == [3, 3, 2, 1, 0]
    return out


@pytest.mark.parametrize("res", _accepted_resolutions())
def test_cross_check_against_per_object_sdfs(gpu, res):
    shape = (12, 11, 10)
    rng = np.random.default_rng(12)
    occ = _noise(rng, shape, 0.8)
    keys = np.where(np.arange(12)[:, None, None] < 5, 1, np.where(np.arange(11)[None, :, None] < 6, 2, 7)).astype(np.uint32) * np.ones(shape, np.uint32)
    keys[rng.random(shape) < 0.05] = 0
    cells = R.cells_of(occ, keys, 16, 8)
    ids = [1, 2, 7]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        fields, _ = gpu.build_tagged_objects(cells, shape, ids, unknown_is_filled=True, resolution=res, add_virtual_border=False)
        bdy = np.float32(-1.9 * res)
        drawn = np.zeros(shape, bool)
        for o, d in zip(ids, fields):
            drawn |= (keys == o) & (d.astype(np.float64) < 0.0) & (d > bdy)
    want = np.flatnonzero(drawn.reshape(-1)).astype(np.uint32)
    reach = capi.display_contour_reach(res)
    assert reach == CR.reach(res)
    got = gpu.display_select_contour(cells, shape, reach)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], keys.reshape(-1)[want])
    assert np.array_equal(want, CR.by_neighbours(occ, keys, reach)[0])
    assert (len(want) > 0) == (reach > 0)


# ---- the fuzz, under red zones ---------------------------------------------------------------------------------------------------------
_REDZONE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import contour_cases as K
from sdf_tools_amd import capi
ctx = capi.SdfGpu(0)
K.fuzz(ctx, 100, 20251019)
ctx.close()
print("redzone clean")
"""


def test_fuzz_under_redzones(tmp_path):
    script = tmp_path / "contour_redzone.py"
    script.write_text(_REDZONE_CHILD)
    env = dict(os.environ, SDFGPU_REDZONE="1")
    r = subprocess.run([sys.executable, str(script), os.path.dirname(HERE), HERE], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "redzone clean" in r.stdout
