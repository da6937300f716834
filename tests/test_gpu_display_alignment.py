"""GPU: every display-export entry point with each caller pointer 4 bytes off a 16-byte boundary (include/sdfgpu.h promises that
4-byte alignment suffices, the points' doubles included; DESIGN.md sections 22 and 23).  Buffers come from tests/alignment_harness.py:
each sits 256 + shift bytes into a 256-byte-aligned arena with 4 KiB of sentinel bytes on either side, both bands are checked after
the call, and the payload is read back from the same offset.  Results are bit-equal to the restatement and to the shift-0 control."""
import numpy as np
import pytest
import torch

import display_cases as C
import display_restated as R
import stream_harness as H
from alignment_harness import Buffers
from sdf_tools_amd import capi

pytestmark = pytest.mark.gpu

SHAPE = (9, 9, 33)
N = int(np.prod(SHAPE))
SHIFTS = [0, 4, 8, 12]


def _shifts(names, shifted, shift):
    return {n: (shift if shifted in (n, "all") else 0) for n in names}


def _scene(seed=11):
    rng = np.random.default_rng(seed)
    occ = rng.choice(C.OCC_VALUES, size=SHAPE)
    keys = rng.choice(np.array([0, 3, 300, 70000, 2 ** 32 - 1], np.uint32), size=SHAPE)
    return occ, keys


SELECT_NAMES = ("cells", "indices", "keys", "group_keys", "group_offsets")


@pytest.mark.parametrize("shifted", SELECT_NAMES + ("all",))
@pytest.mark.parametrize("stride", [8, 16])
def test_select_cells_device_off_alignment(gpu, stride, shifted):
    occ, keys = _scene()
    for rule, opts in ((capi.DISPLAY_OCCUPANCY, dict(class_mask=5, surface_only=True)), (capi.DISPLAY_KEY_FIELD, dict(draw_zero=False))):
        want = C.reference(occ, keys, rule, True, **opts)
        total, groups = len(want[0]), len(want[2])
        for shift in ([0, 4] if shifted != "all" else SHIFTS):
            b = Buffers(_shifts(SELECT_NAMES, shifted, shift))
            cells = b.put("cells", R.cells_of(occ, keys, stride))
            idx, k = b.out("indices", total * 4), b.out("keys", total * 4)
            gk, go = b.out("group_keys", groups * 4), b.out("group_offsets", (groups + 1) * 4)
            assert cells % 16 == (shift if shifted in ("cells", "all") else 0)
            t, g = gpu.display_select_cells_device(cells, SHAPE, rule, stride, 0, 4, grouped=True, d_indices=idx, d_keys=k, capacity=total,
                                                   d_group_keys=gk, d_group_offsets=go, group_capacity=groups, **opts)
            what = "select_cells_device rule %d, %d-byte records, %s + %d" % (rule, stride, shifted, shift)
            b.check(what)
            assert (t, g) == (total, groups), what
            C.same(what, tuple(b.get(n, np.uint32) for n in SELECT_NAMES[1:]), want)
            # scan order, without keys
            b2 = Buffers(_shifts(SELECT_NAMES, shifted, shift))
            cells = b2.put("cells", R.cells_of(occ, keys, stride))
            idx = b2.out("indices", total * 4)
            gpu.display_select_cells_device(cells, SHAPE, rule, stride, 0, 4, d_indices=idx, capacity=total, **opts)
            b2.check(what + ", scan order")
            assert np.array_equal(b2.get("indices", np.uint32), C.reference(occ, keys, rule, False, **opts)[0]), what


@pytest.mark.parametrize("shifted", ["sdf", "indices", "colors", "all"])
def test_sdf_entries_off_alignment(gpu, shifted):
    rng = np.random.default_rng(12)
    d = (rng.standard_normal(SHAPE) * 2).astype(np.float32)
    d.reshape(-1)[:5] = (0.0, -0.0, np.nan, 3.0, -4.0)
    want_idx, want_col = R.select_sdf(d)[0], R.sdf_colors(d, 0.5)
    for shift in ([0, 4] if shifted != "all" else SHIFTS):
        b = Buffers(_shifts(("sdf", "indices", "colors"), shifted, shift))
        sdf = b.put("sdf", d)
        idx, col = b.out("indices", len(want_idx) * 4), b.out("colors", N * 16)
        what = "sdf entries, %s + %d" % (shifted, shift)
        assert gpu.display_select_sdf_device(sdf, SHAPE, idx, len(want_idx)) == len(want_idx)
        gpu.display_sdf_colors_device(sdf, SHAPE, 0.5, col)
        b.check(what)
        assert np.array_equal(b.get("indices", np.uint32), want_idx), what
        assert H.same_or_nan(b.get("colors", np.float32, SHAPE + (4,)), want_col), what


EXPAND_NAMES = ("indices", "keys", "table", "points", "colors")


@pytest.mark.parametrize("shifted", EXPAND_NAMES + ("all",))
def test_expand_device_off_alignment(gpu, shifted):
    rng = np.random.default_rng(13)
    count, cell, default = 4099, (0.1, 0.25, 3.0), (0.5, 0.25, 0.125, 1.0)
    idx = rng.integers(0, N, size=count).astype(np.uint32)
    keys = rng.integers(0, 6, size=count).astype(np.uint32)
    table = rng.random((4, 4)).astype(np.float32)
    for shift in ([0, 4] if shifted != "all" else SHIFTS):
        b = Buffers(_shifts(EXPAND_NAMES, shifted, shift))
        d_idx, d_keys, d_table = b.put("indices", idx), b.put("keys", keys), b.put("table", table)
        pts, col = b.out("points", count * 24), b.out("colors", count * 16)
        gpu.display_expand_device(d_idx, count, SHAPE, cell, d_points=pts, d_colors=col, d_keys=d_keys, d_color_table=d_table, table_entries=4,
                                  default_color=default)
        torch.cuda.synchronize()
        what = "expand_device, %s + %d" % (shifted, shift)
        b.check(what)
        assert b.get("points", np.uint8).tobytes() == R.points(idx, SHAPE, cell).tobytes(), what
        assert b.get("colors", np.uint8).tobytes() == R.table_colors(keys, table, default).tobytes(), what


def test_host_entries_off_alignment(gpu):
    """the host forms with every host pointer 4 bytes off a 16-byte boundary"""
    occ, keys = _scene(14)

    def off(a):
        a = np.ascontiguousarray(a)
        raw = np.empty(a.nbytes + 32, np.uint8)
        start = (-raw.ctypes.data) % 16 + 4
        v = raw[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
        v[...] = a
        assert v.ctypes.data % 16 == 4
        return v
    for stride in (8, 16):
        cells = off(R.cells_of(occ, keys, stride))
        for rule, opts in ((capi.DISPLAY_OCCUPANCY, dict(class_mask=3, surface_only=True)), (capi.DISPLAY_KEY_FIELD, dict(draw_keys=off(np.array([3, 70000], np.uint32))))):
            for grouped in (False, True):
                C.same("host form", gpu.display_select_cells(cells, SHAPE, rule, stride, 0, 4, grouped=grouped, **opts),
                       C.reference(occ, keys, rule, grouped, **opts))
    d = off((np.random.default_rng(15).standard_normal(SHAPE) * 2).astype(np.float32))
    assert np.array_equal(gpu.display_select_sdf(d), R.select_sdf(d)[0])
    assert H.same_or_nan(gpu.display_sdf_colors(d, 0.25), R.sdf_colors(d, 0.25))
