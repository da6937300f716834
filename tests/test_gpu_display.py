"""Display export on the MI355X (sdfgpu_display_*, include/sdfgpu.h "Display export"): every result bit-equal to
the numpy restatement (tests/display_restated.py), through the host and the device entry points.

Chunk sizes of the kernels (sdfgpu_display.hpp, which takes them from sdfgpu_surfaces.hpp): a wave handles 64 voxels a round,
k_dp_select 256, a tile is kDpTile = kSfTile = 4096 voxels or elements, the scan of the tile counts works in segments of
kDpScanSeg = kSfScanSeg = 2048 entries, and the sort takes kSfDigitBits = 8 key bits a pass.  test_more_tiles_than_one_scan_segment
reads the two constants from the headers and runs a grid of just over kDpScanSeg * kDpTile voxels (129 x 256 x 257 with these).
test_long_draw_lists runs key_listed's lower-bound search on lists of 1 to 65 537 entries; test_lines_of_a_word_and_a_tile and
test_drawn_total_on_a_tile_edge put grids and drawn totals on, one short of and one past those chunk sizes.  Record layouts other
than "occupancy at 0, key at 4" are in tests/test_gpu_display_layouts.py, a grid past 2^31 voxels in tests/test_gpu_display_large.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import display_cases as C
import display_restated as R
import scenes
import stream_harness as H
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sdf_tools_amd", "csrc")
ISSUE_SHAPES = [(1, 1, 1), (1, 1, 40), (7, 1, 1), (5, 6, 7), (2, 3, 31), (2, 3, 32), (3, 4, 65), (9, 9, 33), (17, 16, 33)]
OCC, KEY = capi.DISPLAY_OCCUPANCY, capi.DISPLAY_KEY_FIELD


def _constants():
    """the integer constants of sdfgpu_display.hpp and sdfgpu_surfaces.hpp, names resolved"""
    raw = {}
    for name in ("sdfgpu_surfaces.hpp", "sdfgpu_display.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            raw.update(re.findall(r"constexpr int (\w+) = (\w+);", f.read()))
    def value(v):
        return int(v) if v.isdigit() else value(raw[v])
    return {k: value(v) for k, v in raw.items()}


def _occ(rng, shape):
    return rng.choice(C.OCC_VALUES, size=shape)


# ---- the rules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ISSUE_SHAPES)
def test_occupancy_rule(gpu, shape):
    rng = np.random.default_rng(sum(shape))
    occ = _occ(rng, shape)
    keys = np.zeros(shape, np.uint32)
    for mask in range(8):
        for surf in (False, True):
            # (both strides, forms and result forms for two masks; one combination each for the rest, in rotation)
            full = mask in (5, 7)
            C.check(gpu, occ, keys, OCC, class_mask=mask, surface_only=surf,
                    strides=(8, 16) if full else ((8, 16)[mask % 2],), forms=("host", "device") if full else (("host", "device")[surf],))


@pytest.mark.parametrize("shape", ISSUE_SHAPES)
def test_key_field_rule(gpu, shape):
    rng = np.random.default_rng(sum(shape) + 1)
    occ = _occ(rng, shape)
    for p, pool in enumerate(C.KEY_POOLS):                      # a single key (no pass) ... keys near 2^32 - 1 (four passes)
        pool = np.array(pool, np.uint32)
        keys = rng.choice(pool, size=shape)
        draws = [None, [], [int(pool[-1])], sorted({int(k) for k in pool} | {4, 2 ** 32 - 3})]
        for d, draw in enumerate(draws):
            for draw_zero in (False, True):
                full = p == 5 and d in (0, 3)
                C.check(gpu, occ, keys, KEY, draw_keys=draw, draw_zero=draw_zero, class_mask=(7, 7, 5, 2)[(p + d) % 4],
                        strides=(8, 16) if full else ((8, 16)[(p + d) % 2],), forms=("host", "device") if full else (("host", "device")[draw_zero],))


def test_all_four_sort_passes_and_none(gpu):
    rng = np.random.default_rng(3)
    shape = (17, 16, 33)
    occ = _occ(rng, shape)
    keys = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)        # 32 differing bits
    keys.reshape(-1)[:2] = (0, 2 ** 32 - 1)
    idx, k = C.check(gpu, occ, keys, KEY)
    assert len(np.unique(k)) > 8000
    C.check(gpu, occ, np.full(shape, 2 ** 32 - 1, np.uint32), KEY)                          # one key: nothing to sort
    C.check(gpu, occ, np.where(rng.random(shape) < 0.5, 0x80000000, 0x80000001).astype(np.uint32), KEY)   # one differing bit


def test_more_tiles_than_one_scan_segment(gpu):
    k = _constants()
    assert k["kDpTile"] == k["kSfTile"] and k["kDpScanSeg"] == k["kSfScanSeg"]
    shape = (129, 256, 257)
    n = int(np.prod(shape))
    limit = k["kDpScanSeg"] * k["kDpTile"]
    assert limit < n <= limit + limit // 64, "choose a grid just above one scan segment of tiles (%d voxels)" % limit
    rng = np.random.default_rng(9)
    occ = _occ(rng, shape)
    keys = rng.choice(np.array([0, 3, 300, 70000], np.uint32), size=shape)
    C.check(gpu, occ, keys, OCC, class_mask=5, surface_only=True, strides=(8,), forms=("device",), groupings=(True,))
    C.check(gpu, occ, keys, KEY, draw_zero=False, strides=(16,), forms=("device",), groupings=(True,))
    C.check(gpu, occ, keys, KEY, draw_keys=[300], strides=(8,), forms=("host",), groupings=(False,))


# ---- long draw lists: the lower-bound search of key_listed --------------------------------------------------------------------------
DRAW_LENGTHS = [1, 2, 3, 63, 64, 65, 1000, 65537]


def _draw_list(rng, length, with_zero, with_last):
    """ascending uint32 list of `length` entries from a seeded pool in [1000, 2^32 - 1000), 0 and 2^32 - 1 planted on request; with
    duplicates: the first entry twice from 3 entries on (0 twice where it is planted), the last twice from 5 on, the two-entry
    list that holds neither end value, and whatever the draw from a pool of half the length repeats"""
    pool = rng.integers(1000, 2 ** 32 - 1000, size=max(2, length // 2 + 1), dtype=np.uint64)
    draw = np.sort(rng.choice(pool, size=length))
    if with_zero:
        draw[0] = 0
    if with_last:
        draw[-1] = 2 ** 32 - 1
    if length >= 3 or (length == 2 and not (with_zero or with_last)):
        draw[1] = draw[0]
    if length >= 5:
        draw[-2] = draw[-1]
    draw = draw.astype(np.uint32)
    assert len(draw) == length and (np.diff(draw.astype(np.int64)) >= 0).all() and (length < 3 or (np.diff(draw.astype(np.int64)) == 0).any())
    return draw


def _keys_around(rng, draw, shape):
    """a key grid that holds the list's first and last entries, entries in between, values between two entries, values below and
    above the list (where there are any), 0 and 2^32 - 1; -> (keys, the pool by kind)"""
    d = np.unique(draw).astype(np.int64)
    inside = d[rng.integers(0, len(d), size=6)]
    gaps = np.flatnonzero(np.diff(d) > 1)
    between = (d[gaps] + 1 + (np.diff(d)[gaps] - 2) // 2)[rng.integers(0, max(len(gaps), 1), size=6 if len(gaps) else 0)]
    near = np.concatenate([d[:3] + 1, d[-3:] - 1, inside + 1, inside - 1])
    near = near[(near > d[0]) & (near < d[-1]) & ~np.isin(near, d)]
    below = np.array([v for v in (0, d[0] - 1, d[0] // 2) if v < d[0]], np.int64)
    above = np.array([v for v in (2 ** 32 - 1, d[-1] + 1, d[-1] + (2 ** 32 - 1 - d[-1]) // 2) if v > d[-1]], np.int64)
    kinds = dict(first=d[:1], last=d[-1:], inside=inside, between=np.concatenate([between, near]), below=below, above=above,
                 ends=np.array([0, 2 ** 32 - 1], np.int64))
    pool = np.unique(np.concatenate(list(kinds.values()))).astype(np.uint32)
    keys = rng.choice(pool, size=shape)
    keys.reshape(-1)[:len(pool)] = pool                             # every value of the pool at least once
    return keys, kinds


@pytest.mark.parametrize("length", DRAW_LENGTHS)
def test_long_draw_lists(gpu, length):
    shape = (17, 16, 33)
    at = DRAW_LENGTHS.index(length)
    rng = np.random.default_rng(100 + length)
    occ = _occ(rng, shape)
    first = (bool(at & 1), bool(at & 2))
    variants = [first, (not first[0], not first[1])]               # over the lengths: each end value in some lists, absent from others
    if length <= 2:                                                 # the shortest lists in every variant they can have
        variants = [(False, False), (True, False), (False, True)] + [(True, True)] * (length == 2)
    for with_zero, with_last in variants:
        draw = _draw_list(rng, length, with_zero, with_last)
        assert (0 in draw) == with_zero and (2 ** 32 - 1 in draw) == with_last
        keys, kinds = _keys_around(rng, draw, shape)
        listed = np.isin(keys, draw)
        assert listed.any() and not listed.all()
        assert (keys == draw[0]).any() and (keys == draw[-1]).any()
        if not with_zero:
            assert len(kinds["below"]) and (keys < draw[0]).any()
        if not with_last:
            assert len(kinds["above"]) and (keys > draw[-1]).any()
        if length >= 3:
            assert len(kinds["between"]) and ((keys > draw[0]) & (keys < draw[-1]) & ~listed).any()
        for draw_zero in (False, True):
            idx, k = C.check(gpu, occ, keys, KEY, draw_keys=draw, draw_zero=draw_zero, strides=(8,))
            assert len(idx) == int((listed & (draw_zero | (keys != 0))).sum())
            assert set(np.unique(k).tolist()) == set(np.unique(keys[listed & (draw_zero | (keys != 0))]).tolist())
    # the list as the only filter and with a class mask beside it; a list that holds every key of the grid; one that holds none
    C.check(gpu, occ, keys, KEY, draw_keys=draw, class_mask=5, strides=(16,), forms=("device",))
    C.check(gpu, occ, keys, KEY, draw_keys=np.sort(np.concatenate([draw, np.unique(keys)])), strides=(8,), forms=("device",))
    none = np.sort(rng.choice(np.setdiff1d(np.arange(2000, 2000 + 4 * length, dtype=np.uint32), keys), size=length))
    assert len(C.check(gpu, occ, keys, KEY, draw_keys=none, strides=(8,), forms=("host",), groupings=(False,))[0]) == 0


# ---- tile and word edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 4095, 4096, 4097, 8192])
def test_lines_of_a_word_and_a_tile(gpu, n):
    """a wave's ballot is 64 voxels, a tile kDpTile = 4096: lines of those lengths and one more or less, along each axis (the surface
    rule's neighbours then lie along that axis alone)"""
    assert _constants()["kDpTile"] == 4096
    rng = np.random.default_rng(n)
    for shape in ((1, 1, n), (1, n, 1), (n, 1, 1)):
        occ = _occ(rng, shape)
        keys = rng.choice(np.array([0, 3, 300, 2 ** 32 - 1], np.uint32), size=shape)
        C.check(gpu, occ, keys, OCC, class_mask=7, surface_only=True, strides=(8,), forms=("device",))
        C.check(gpu, occ, keys, KEY, draw_zero=False, strides=(16,), forms=("device",))
        idx, _ = C.check(gpu, np.ones(shape, np.float32), keys, KEY, strides=(8,), forms=("device",))     # every voxel drawn: the last lane of the last word
        assert len(idx) == n and idx[-1] == n - 1


@pytest.mark.parametrize("total", [4095, 4096, 4097])
def test_drawn_total_on_a_tile_edge(gpu, total):
    """exactly `total` voxels of 17 x 16 x 33 carry a key: the second stage (group starts over the sorted keys) then has a tile that is
    one short, full, or followed by a tile of one element.  Three groups of 1500, total - 1501 and 1 elements: with 4097 drawn the
    last group starts exactly at element 4096, the first of the second tile; with 4096 that is where the results end."""
    tile = _constants()["kDpTile"]
    assert tile == 4096
    shape = (17, 16, 33)
    rng = np.random.default_rng(total)
    occ = _occ(rng, shape)
    where = rng.permutation(int(np.prod(shape)))[:total]
    keys = np.zeros(shape, np.uint32)
    keys.reshape(-1)[where[:1500]] = 3
    keys.reshape(-1)[where[1500:total - 1]] = 300
    keys.reshape(-1)[where[total - 1:]] = 2 ** 32 - 1
    want = C.reference(occ, keys, KEY, True, draw_zero=False)
    assert len(want[0]) == total and want[2].tolist() == [3, 300, 2 ** 32 - 1] and want[3].tolist() == [0, 1500, total - 1, total]
    assert (total - 1 == tile) == (total == 4097)
    C.check(gpu, occ, keys, KEY, draw_zero=False, strides=(8,), forms=("device",))
    C.check(gpu, occ, keys, KEY, draw_keys=[3, 300, 2 ** 32 - 1], strides=(16,), forms=("device",))
    # the same total in scan order under the occupancy rule: exactly `total` filled voxels
    filled = np.zeros(shape, np.float32)
    filled.reshape(-1)[where] = 1.0
    idx, _ = C.check(gpu, filled, keys, OCC, class_mask=1, strides=(8,), forms=("device",))
    assert len(idx) == total


def _both_sdf_forms(gpu, d):
    want = R.select_sdf(d)[0]
    got = gpu.display_select_sdf(d)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    d_sdf = C.dev(d)
    total = gpu.display_select_sdf_device(d_sdf.data_ptr(), d.shape)
    assert total == len(want)
    buf = C.words(total)
    assert gpu.display_select_sdf_device(d_sdf.data_ptr(), d.shape, buf.data_ptr(), total) == total
    assert np.array_equal(C.host_words(buf, total), want)
    return want


def test_sdf_rule(gpu):
    m, res = scenes.tutorial_scene()
    sdf, _ = gpu.build(m, res)
    assert len(_both_sdf_forms(gpu, sdf)) == 20 ** 3
    rng = np.random.default_rng(2)
    for shape in ISSUE_SHAPES:
        d = rng.choice(np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 1.5, -2.5], np.float32), size=shape)
        _both_sdf_forms(gpu, d)


# ---- capacities, empty and full results, refusals -----------------------------------------------------------------------------------
def test_capacity_and_sentinels(gpu):
    rng = np.random.default_rng(5)
    shape = (9, 9, 33)
    occ = _occ(rng, shape)
    keys = rng.choice(np.array([0, 3, 300, 70000], np.uint32), size=shape)
    cells = R.cells_of(occ, keys, 8)
    want = C.reference(occ, keys, KEY, True)
    total, groups = len(want[0]), len(want[2])
    assert total == occ.size and groups == 4
    d_cells = C.dev(cells)
    for grouped in (False, True):
        for cap in (total - 1, 0):
            idx, k, gk, go = C.words(total), C.words(total), C.words(groups), C.words(groups + 1)
            with pytest.raises(capi.SdfGpuError) as e:
                gpu.display_select_cells_device(d_cells.data_ptr(), shape, KEY, 8, 0, 4, grouped=grouped, d_indices=idx.data_ptr(), d_keys=k.data_ptr(),
                                                capacity=cap, d_group_keys=gk.data_ptr(), d_group_offsets=go.data_ptr(), group_capacity=groups)
            assert e.value.code == -1 and e.value.total == total and "drawn" in str(e.value)
            for t in (idx, k, gk, go):
                assert (t.cpu().numpy().view(np.uint32) == C.SENTINEL).all(), "a refused call stored results"
            with pytest.raises(capi.SdfGpuError) as e:
                gpu.display_select_cells(cells, shape, KEY, 8, 0, 4, grouped=grouped, capacity=cap)
            assert e.value.code == -1 and e.value.total == total
    # a short group capacity: total and groups come back, nothing is stored past it
    idx, k, gk, go = C.words(total), C.words(total), C.words(groups - 1), C.words(groups)
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.display_select_cells_device(d_cells.data_ptr(), shape, KEY, 8, 0, 4, grouped=True, d_indices=idx.data_ptr(), d_keys=k.data_ptr(),
                                        capacity=total, d_group_keys=gk.data_ptr(), d_group_offsets=go.data_ptr(), group_capacity=groups - 1)
    assert e.value.code == -1 and (e.value.total, e.value.groups) == (total, groups)
    assert (gk.cpu().numpy().view(np.uint32) == C.SENTINEL).all() and (go.cpu().numpy().view(np.uint32) == C.SENTINEL).all()
    C.host_words(idx, total), C.host_words(k, total)
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.display_select_cells(cells, shape, KEY, 8, 0, 4, grouped=True, group_capacity=groups - 1)
    assert (e.value.total, e.value.groups) == (total, groups)
    # exactly the total: C.run_device sizes every buffer exactly and checks the word behind it
    C.same("exact capacities", C.run_device(gpu, cells, shape, KEY, 8, True), want)
    d = np.full(shape, -1.0, np.float32)
    for cap in (d.size - 1, 0):
        buf = C.words(d.size)
        with pytest.raises(capi.SdfGpuError) as e:
            gpu.display_select_sdf_device(C.dev(d).data_ptr(), shape, buf.data_ptr(), cap)
        assert e.value.total == d.size and (buf.cpu().numpy().view(np.uint32) == C.SENTINEL).all()
        with pytest.raises(capi.SdfGpuError):
            gpu.display_select_sdf(d, capacity=cap)


def test_empty_and_all_drawn(gpu):
    shape = (17, 16, 33)
    n = int(np.prod(shape))
    filled = np.ones(shape, np.float32)
    keys = np.full(shape, 6, np.uint32)
    assert len(C.check(gpu, filled, keys, OCC, class_mask=1)[0]) == n
    assert len(C.check(gpu, filled, keys, OCC, class_mask=6)[0]) == 0
    assert len(C.check(gpu, filled, keys, OCC, class_mask=1, surface_only=True)[0]) == 0
    assert len(C.check(gpu, filled, keys, KEY)[0]) == n
    assert len(C.check(gpu, filled, keys, KEY, draw_keys=[5, 7])[0]) == 0
    assert len(C.check(gpu, filled, np.zeros(shape, np.uint32), KEY, draw_zero=False)[0]) == 0
    assert len(gpu.display_select_sdf(filled)) == 0 and len(gpu.display_select_sdf(-filled)) == n


def test_refusals(gpu):
    d = torch.zeros(16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for call in (lambda: gpu.display_select_cells_device(d.data_ptr(), (65536, 65536, 1), OCC),     # 2^32 voxels: refused by shape alone
                 lambda: gpu.display_select_sdf_device(d.data_ptr(), (65536, 1, 65536)),
                 lambda: gpu.display_sdf_colors_device(d.data_ptr(), (1, 65536, 65536), 0.5, d.data_ptr()),
                 lambda: gpu.display_expand_device(d.data_ptr(), 1, (65536, 65536, 1), 0.1, d_points=d.data_ptr())):
        with pytest.raises(capi.SdfGpuError) as e:
            call()
        assert e.value.code == -1 and "2^32 - 1 voxels" in str(e.value)
    assert torch.cuda.mem_get_info()[0] == before, "a call refused by its shape allocated device memory"
    sdf = np.ones((2, 3, 4), np.float32)
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.display_sdf_colors(sdf, float("nan"))
    assert e.value.code == -1 and "NaN" in str(e.value)
    out = C.words(24 * 4)
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.display_sdf_colors_device(C.dev(sdf).data_ptr(), sdf.shape, float("nan"), out.data_ptr())
    assert e.value.code == -1 and (out.cpu().numpy().view(np.uint32) == C.SENTINEL).all()
    cells = R.cells_of(np.zeros((2, 3, 4), np.float32), np.zeros((2, 3, 4), np.uint32), 8)
    with pytest.raises(capi.SdfGpuError) as e:
        gpu.display_select_cells(cells, (2, 3, 4), KEY, draw_keys=[3, 2])
    assert e.value.code == -1 and "ascending" in str(e.value)
    for bad in (dict(rule=2), dict(class_mask=8), dict(key_offset=8), dict(key_offset=2)):
        with pytest.raises(capi.SdfGpuError):
            gpu.display_select_cells(cells, (2, 3, 4), **dict(dict(rule=KEY), **bad))


# ---- expand and the SDF colour map -----------------------------------------------------------------------------------------------------
def test_expand_points_and_colors(gpu):
    rng = np.random.default_rng(6)
    shape, cell = (9, 9, 33), (0.1, 0.25, 3.0)
    n = int(np.prod(shape))
    for count in (1, 63, 4097):
        idx = rng.integers(0, n, size=count).astype(np.uint32)
        idx[0] = n - 1
        keys = rng.choice(np.array([0, 1, 2, 3, 4, 2 ** 32 - 1], np.uint32), size=count)
        table = rng.random((3, 4)).astype(np.float32)           # shorter than the largest key: 3, 4 and 2^32 - 1 take the default
        default = (0.5, 0.25, 0.125, 1.0)
        d_idx, d_keys, d_table = C.dev(idx), C.dev(keys), C.dev(table)
        pts, col = C.words(count * 6), C.words(count * 4)
        gpu.display_expand_device(d_idx.data_ptr(), count, shape, cell, d_points=pts.data_ptr(), d_colors=col.data_ptr(), d_keys=d_keys.data_ptr(),
                                  d_color_table=d_table.data_ptr(), table_entries=3, default_color=default)
        torch.cuda.synchronize()
        want = R.points(idx, shape, cell)
        assert C.host_words(pts, count * 6).view(np.float64).reshape(count, 3).tobytes() == want.tobytes()
        assert C.host_words(col, count * 4).view(np.float32).reshape(count, 4).tobytes() == R.table_colors(keys, table, default).tobytes()
        x = idx.astype(np.int64) // (shape[1] * shape[2])
        assert np.array_equal(want[:, 0], (x + 0.5) * 0.1)      # (i + 0.5) * cell in float64
        # points alone; colours alone without keys (every key is 0) and without a table (every colour is the default)
        pts = C.words(count * 6)
        gpu.display_expand_device(d_idx.data_ptr(), count, shape, cell, d_points=pts.data_ptr())
        col = C.words(count * 4)
        gpu.display_expand_device(d_idx.data_ptr(), count, shape, cell, d_colors=col.data_ptr(), d_color_table=d_table.data_ptr(), table_entries=3)
        col2 = C.words(count * 4)
        gpu.display_expand_device(d_idx.data_ptr(), count, shape, cell, d_colors=col2.data_ptr(), d_keys=d_keys.data_ptr(), default_color=default)
        torch.cuda.synchronize()
        assert C.host_words(pts, count * 6).view(np.float64).tobytes() == want.tobytes()
        assert np.array_equal(C.host_words(col, count * 4).view(np.float32).reshape(count, 4), np.tile(table[0], (count, 1)))
        assert np.array_equal(C.host_words(col2, count * 4).view(np.float32).reshape(count, 4), np.tile(np.float32(default), (count, 1)))


def _both_color_forms(gpu, d, alpha):
    want = R.sdf_colors(d, alpha)
    got = gpu.display_sdf_colors(d, alpha)
    assert got.shape == d.shape + (4,) and H.same_or_nan(got, want), "sdfgpu_display_sdf_colors %s" % (d.shape,)
    out = C.words(d.size * 4)
    gpu.display_sdf_colors_device(C.dev(d).data_ptr(), d.shape, alpha, out.data_ptr())
    assert H.same_or_nan(C.host_words(out, d.size * 4).view(np.float32).reshape(want.shape), want), "sdfgpu_display_sdf_colors_device %s" % (d.shape,)


def test_sdf_colors(gpu):
    m, res = scenes.tutorial_scene()
    sdf, _ = gpu.build(m, res)
    for alpha in (0.5, -1.0, 7.0, 0.1):
        _both_color_forms(gpu, sdf, alpha)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0, -3.0, 1e-45, -1e-45], np.float32)
    rng = np.random.default_rng(7)
    for shape in ISSUE_SHAPES:
        _both_color_forms(gpu, rng.choice(special, size=shape), 0.75)
        _both_color_forms(gpu, rng.choice(special[[0, 1, 4, 5, 6]], size=shape), 1.0)     # finite extrema
        _both_color_forms(gpu, (rng.standard_normal(shape) * 3).astype(np.float32), 0.3)
    _both_color_forms(gpu, np.zeros((5, 6, 7), np.float32), 0.5)                          # min = max = 0: no voxel divides
    _both_color_forms(gpu, np.full((5, 6, 7), np.nan, np.float32), 0.5)


# ---- the fuzz, under red zones ---------------------------------------------------------------------------------------------------------
_REDZONE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import numpy as np
import display_cases as C
import display_restated as R
from sdf_tools_amd import capi
ctx = capi.SdfGpu(0)
C.fuzz(ctx, 200, 20250611)
d = np.random.default_rng(1).standard_normal((25, 20, 15)).astype(np.float32)
assert np.array_equal(ctx.display_select_sdf(d), R.select_sdf(d)[0])
assert ctx.display_sdf_colors(d, 0.5).tobytes() == R.sdf_colors(d, 0.5).tobytes()
ctx.close()
print("redzone clean")
"""


def test_fuzz_under_redzones(tmp_path):
    script = tmp_path / "display_redzone.py"
    script.write_text(_REDZONE_CHILD)
    env = dict(os.environ, SDFGPU_REDZONE="1")
    r = subprocess.run([sys.executable, str(script), os.path.dirname(HERE), HERE], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "redzone clean" in r.stdout


def test_display_leaves_sdf_builds_alone(gpu):
    m, res = scenes.tutorial_scene()
    sdf, ext = gpu.build(m, res)
    info = gpu.last_build_info()
    gpu.display_select_sdf(sdf)
    gpu.display_sdf_colors(sdf, 0.5)
    gpu.display_select_cells(R.cells_of(m.astype(np.float32), m.astype(np.uint32), 8), m.shape, OCC, surface_only=True, grouped=True)
    assert gpu.last_build_info() == info
    again, ext2 = gpu.build(m, res)
    assert np.array_equal(sdf, again) and ext == ext2
