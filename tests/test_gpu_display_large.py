"""GPU: the display export's device forms on a grid just past 2^31 voxels (1290 x 1290 x 1291 = 2 148 353 100; 869 452 voxels lie past
linear index 2^31, all in the last x plane), the test that catches signed or 32-bit index arithmetic in sdfgpu_display.hip.

The scene (built on the device, no host copy).  The box B is x in [1280, 1290), y in [600, 1290), every z: 8 907 900 voxels, more
than one scan segment of tiles (kDpScanSeg * kDpTile = 8 388 608), on both sides of index 2^31, against the x, y and both z faces of the
grid.  Records of 8 bytes, occupancy at 0 and key at 4: occupancy 0.0 outside B and 1.0 inside, one NaN inside B, 0.5 at the last
voxel (index n - 1, the corner of B); keys 0 outside B, inside B one of 7, 2^31 + 5, 2^32 - 1 by (y + z) % 3 -- a 32-bit sort of
four passes -- and 9 at the last voxel.  The SDF tests use a float field of the same shape whose value depends on x alone,
(x - 1280) / 4, with a NaN, a -0.0 and a +inf planted.

Totals, from the scene (integers): the last voxel is a voxel OF the box, so
    occupancy rule, class_mask 7: n;  3 (F | E): n - 2;  2 (E): n - |B|;  5 (F | U): |B| (the NaN voxel has key 2 and is drawn under U)
    key rule, draw_zero = 0: |B| in four groups 7, 9, 2^31 + 5, 2^32 - 1 (key 9 replaces the last voxel's box key)
Of these n and n - 2 lie above 2^31; no total of a selection that must also exceed one scan segment INSIDE the box can.

Every closed form is a function of a Scene and is first pinned without a GPU on a 9 x 10 x 11 scene of the same kind against
tests/display_restated.py, where a corrupted result must make the comparison raise.  The surface rule's expectation is no closed
form: it is the 26-neighbour rule restated with torch on x chunks with a one-plane halo (class planes, a 3 x 3 x 3 max-pool per
class, the WANTS table of the restatement).  At a grid face the display rule differs from the component-surface rule: a face
alone makes no surface.  The GPU tests skip when the device has too little free memory.  Host forms are not run at this size: they
would push 17 GB through the staging, and their index arithmetic is the device forms' own."""
import math
import os
import re

import numpy as np
import pytest
import torch

import display_restated as R

gpu_test = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sdf_tools_amd", "csrc")
SENTINEL = 0x5A5A5A5A
KEYS = (7, 2 ** 31 + 5, 2 ** 32 - 1)                                # inside the box, by (y + z) % 3
LAST_KEY = 9
ONE, HALF, NAN = 0x3F800000, 0x3F000000, 0x7FC00000                 # float32 bits
SLACK = 3 << 30
ALPHA = 0.75


class Scene:
    def __init__(self, shape, box, nan_at, neg_zero_at, inf_at):
        self.shape, self.box = shape, box                           # box: x0, x1, y0, y1, half open, every z
        self.nan_at, self.neg_zero_at, self.inf_at = nan_at, neg_zero_at, inf_at
        self.n = math.prod(shape)
        self.volume = (box[1] - box[0]) * (box[3] - box[2]) * shape[2]

    def lin(self, at):
        return (at[0] * self.shape[1] + at[1]) * self.shape[2] + at[2]

    def inside(self, at):
        x0, x1, y0, y1 = self.box
        return x0 <= at[0] < x1 and y0 <= at[1] < y1

    @property
    def last(self):
        return tuple(s - 1 for s in self.shape)


BIG = Scene((1290, 1290, 1291), (1280, 1290, 600, 1290), nan_at=(1284, 900, 77), neg_zero_at=(1285, 700, 5), inf_at=(3, 4, 5))
SMALL = Scene((9, 10, 11), (7, 9, 4, 10), nan_at=(8, 5, 3), neg_zero_at=(8, 2, 3), inf_at=(1, 2, 3))


def _constants():
    """the integer constants of sdfgpu_display.hpp and sdfgpu_surfaces.hpp, names resolved (tests/test_gpu_display.py)"""
    raw = {}
    for name in ("sdfgpu_surfaces.hpp", "sdfgpu_display.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            raw.update(re.findall(r"constexpr int (\w+) = (\w+);", f.read()))
    def value(v):
        return int(v) if v.isdigit() else value(raw[v])
    return {k: value(v) for k, v in raw.items()}


def _i32(v):
    """a uint32 value as the int32 torch stores"""
    return v - (1 << 32) if v >= (1 << 31) else v


def _u32(t):
    """an int32 tensor of uint32 words -> int64 values"""
    return t.to(torch.int64) & 0xFFFFFFFF


# ---- the scene and its closed forms (torch, on `device`) ------------------------------------------------------------------------
def build_cells(S, device):
    """int32 [nx, ny, nz, 2]: the records (occupancy bits, key)"""
    nx, ny, nz = S.shape
    x0, x1, y0, y1 = S.box
    cells = torch.zeros(S.shape + (2,), dtype=torch.int32, device=device)
    y = torch.arange(y0, y1, device=device).view(-1, 1)
    z = torch.arange(nz, device=device).view(1, -1)
    table = torch.tensor([_i32(k) for k in KEYS], dtype=torch.int32, device=device)
    cells[x0:x1, y0:y1, :, 0] = ONE
    cells[x0:x1, y0:y1, :, 1] = table[(y + z) % 3]
    assert S.inside(S.nan_at) and S.inside(S.last) and S.nan_at != S.last
    cells[S.nan_at][0] = NAN
    cells[S.last][0] = HALF
    cells[S.last][1] = LAST_KEY
    return cells


def box_indices(S, device):
    """int64: the linear indices of the box's voxels, ascending"""
    nx, ny, nz = S.shape
    x0, x1, y0, y1 = S.box
    x = torch.arange(x0, x1, dtype=torch.int64, device=device).view(-1, 1, 1)
    y = torch.arange(y0, y1, dtype=torch.int64, device=device).view(1, -1, 1)
    z = torch.arange(nz, dtype=torch.int64, device=device).view(1, 1, -1)
    return ((x * ny + y) * nz + z).reshape(-1)


def occupancy_totals(S):
    """class_mask -> total, in integers"""
    return {7: S.n, 3: S.n - 2, 2: S.n - S.volume, 5: S.volume}


def scan_order_f_u(S, device):
    """occupancy rule, class_mask 5: (indices, keys) -- the box ascending; key 0 (F) but 2 at the NaN voxel and at the last (U)"""
    idx = box_indices(S, device)
    keys = torch.zeros_like(idx)
    keys[(idx == S.lin(S.nan_at)) | (idx == S.n - 1)] = 2
    return idx, keys


def grouped_by_key(S, device, draw=None):
    """key rule, draw_zero = 0, grouped: (indices, keys, group keys, group offsets), the last two as Python lists.  Group by group in
    ascending key order, each the ascending list of that key's voxels."""
    nx, ny, nz = S.shape
    idx = box_indices(S, device)
    j = ((idx // nz) % ny + idx % nz) % 3
    last = idx == S.n - 1
    lists = {LAST_KEY: idx[last]}
    for which, key in enumerate(KEYS):
        lists[key] = idx[(j == which) & ~last]
    gkeys = [k for k in sorted(lists) if lists[k].numel() and (draw is None or k in draw)]
    offs = [0]
    for k in gkeys:
        offs.append(offs[-1] + int(lists[k].numel()))
    indices = torch.cat([lists[k] for k in gkeys]) if gkeys else idx[:0]
    keys = torch.cat([torch.full_like(lists[k], k) for k in gkeys]) if gkeys else idx[:0]
    return indices, keys, gkeys, offs


def surface_chunks(occ, chunk):
    """The 26-neighbour rule on x chunks of a float32 tensor [nx, ny, nz] (a strided view will do): yields (x of the chunk's first
    plane, bool [planes, ny, nz]).  Per chunk with one plane of halo on either side: the class of every cell, one plane set per class,
    "some cell of the 3 x 3 x 3 block has class w" as a max-pool (whose padding never wins: cells outside the grid do not exist), and a
    cell of class c is a surface iff that holds for a w in WANTS[c]."""
    nx = occ.shape[0]
    for xa in range(0, nx, chunk):
        xb = min(nx, xa + chunk)
        ha, hb = max(0, xa - 1), min(nx, xb + 1)
        o = occ[ha:hb]
        cls = torch.full(o.shape, R.N, dtype=torch.uint8, device=o.device)
        cls[o == 0.5] = R.U
        cls[o < 0.5] = R.E
        cls[o > 0.5] = R.F
        planes = torch.stack([cls == c for c in (R.F, R.E, R.U, R.N)]).to(torch.float32)
        has = torch.nn.functional.max_pool3d(planes, kernel_size=3, stride=1, padding=1) > 0
        del planes
        surf = torch.zeros(o.shape, dtype=torch.bool, device=o.device)
        for c, wanted in R.WANTS.items():
            for w in wanted:
                surf |= (cls == c) & has[w]
        yield xa, surf[xa - ha:xa - ha + (xb - xa)]


def same(name, got, want):
    """two int64 tensors: equal in length and in every value, or an AssertionError that names the first differences"""
    if got.numel() != want.numel():
        raise AssertionError("%s: %d elements, %d expected" % (name, got.numel(), want.numel()))
    if not bool(torch.equal(got, want)):
        bad = (got != want).nonzero().reshape(-1)
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %s, expected %s"
                             % (name, bad.numel(), got.numel(), bad[:3].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist()))


def check_surface(name, got, occ, chunk, class_mask=7):
    """got: int64 indices of a surface_only selection over `occ`; compared chunk by chunk with surface_chunks; returns the count"""
    nx, ny, nz = occ.shape
    pos = 0
    for xa, surf in surface_chunks(occ, chunk):
        if class_mask != 7:
            o = occ[xa:xa + surf.shape[0]]
            key = (~(o > 0.5)).to(torch.int64) + (~((o > 0.5) | (o < 0.5))).to(torch.int64)          # F 0, E 1, U and NaN 2
            surf = surf & torch.tensor([bool((class_mask >> b) & 1) for b in range(3)], device=o.device)[key]
        e = surf.reshape(-1).nonzero().reshape(-1) + xa * ny * nz
        k = int(e.numel())
        same("%s, x planes %d..%d" % (name, xa, xa + surf.shape[0]), got[pos:pos + k], e)
        pos += k
    if pos != got.numel():
        raise AssertionError("%s: %d indices, %d expected" % (name, got.numel(), pos))
    return pos


def plane_values(S):
    """float32 [nx]: the field's value in plane x, (x - x0) / 4 (exact)"""
    return ((np.arange(S.shape[0]) - S.box[0]) * 0.25).astype(np.float32)


def build_field(S, device):
    """float32 [nx, ny, nz] that depends on x alone, with NaN at the last voxel, -0.0 and +inf planted"""
    d = torch.empty(S.shape, dtype=torch.float32, device=device)
    d.copy_(torch.from_numpy(plane_values(S)).to(device).view(-1, 1, 1).expand(S.shape))
    assert S.inf_at[0] != S.shape[0] - 1 and S.inf_at[0] <= S.box[0] < S.neg_zero_at[0]
    d[S.last] = float("nan")
    d[S.neg_zero_at] = -0.0
    d[S.inf_at] = float("inf")
    return d


def sdf_total(S):
    """voxels with d <= 0: the planes x <= x0, less the +inf planted in one of them, and the -0.0 planted behind them"""
    return (S.box[0] + 1) * S.shape[1] * S.shape[2] - 1 + 1


def color_table(S, alpha):
    """(rgba per x plane float32 [nx, 4], rgba of +inf, NaN and -0.0), on the CPU by the restatement: a line of the planes' values
    followed by the three planted ones has the field's extrema (-x0 / 4 and +inf)"""
    line = np.concatenate([plane_values(S), np.array([np.inf, np.nan, -0.0], np.float32)]).reshape(-1, 1, 1)
    rgba = R.sdf_colors(line, alpha)[:, 0, 0, :]
    return rgba[:S.shape[0]].copy(), rgba[S.shape[0]:].copy()


def check_colors(name, colors, S, alpha, chunk):
    """colors: int32 [nx, ny, nz, 4] (the words of the float32 result; the three planted voxels are overwritten here once checked)"""
    table, special = color_table(S, alpha)
    for at, want in zip((S.inf_at, S.last, S.neg_zero_at), special):
        got = colors[at].cpu().numpy().view(np.float32)
        if not bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))):   # (NaN payloads: stream_harness.same_or_nan)
            raise AssertionError("%s: voxel %s is %s, expected %s" % (name, at, got.tolist(), want.tolist()))
        colors[at] = torch.from_numpy(table[at[0]].view(np.int32).copy()).to(colors.device)
    rows = torch.from_numpy(table.view(np.int32).copy()).to(colors.device)
    for xa in range(0, S.shape[0], chunk):
        a, b = colors[xa:xa + chunk], rows[xa:xa + chunk].view(-1, 1, 1, 4)
        if not bool((a == b).all()):
            bad = (a != b).any(dim=3).nonzero()
            raise AssertionError("%s: planes %d..%d: %d voxels differ, first %s" % (name, xa, xa + a.shape[0], bad.shape[0],
                                                                                     [[v[0] + xa] + v[1:] for v in bad[:3].tolist()]))


# ---- the closed forms against the restatement, no GPU ---------------------------------------------------------------------------
def _small_arrays():
    cells = build_cells(SMALL, "cpu").numpy().view(np.uint32)
    return np.ascontiguousarray(cells[..., 0]).view(np.float32), np.ascontiguousarray(cells[..., 1])


def _t(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64))


def test_the_box_is_where_the_issue_puts_it():
    k = _constants()
    S = BIG
    assert 2 ** 31 < S.n < 2 ** 32 and S.n == 2148353100 and S.n - 2 ** 31 == 869452
    x0, x1, y0, y1 = S.box
    assert S.lin((x0, y0, 0)) < 2 ** 31 < S.lin((x1 - 1, y1 - 1, S.shape[2] - 1)) == S.n - 1      # indices on both sides of 2^31
    assert S.volume == 8907900 > k["kDpScanSeg"] * k["kDpTile"] == 8388608
    assert S.inside((2 ** 31 // (S.shape[1] * S.shape[2]), (2 ** 31 // S.shape[2]) % S.shape[1]))    # voxel 2^31 itself is in the box
    assert (2 ** 31 // (S.shape[1] * S.shape[2])) == S.shape[0] - 1                                 # ... in the last x plane
    totals = occupancy_totals(S)
    assert totals[7] > 2 ** 31 and totals[3] > 2 ** 31 and totals[5] > k["kDpScanSeg"] * k["kDpTile"]
    assert sdf_total(S) == 1281 * 1290 * 1291 == 2133364590
    # the replica has the same relations where they can hold at its size
    s = SMALL
    assert s.box[1] == s.shape[0] and s.box[3] == s.shape[1] and s.inside(s.last) and s.inside(s.nan_at)


def test_scan_order_closed_forms_are_the_restatement():
    occ, keys = _small_arrays()
    S = SMALL
    assert sorted(np.unique(keys).tolist()) == [0, 7, 9, 2 ** 31 + 5, 2 ** 32 - 1] and np.isnan(occ).sum() == 1 and (occ == 0.5).sum() == 1
    for mask, total in occupancy_totals(S).items():
        assert len(R.select_occupancy(occ, mask)[0]) == total, mask
    idx, k = R.select_occupancy(occ, 5)
    want_idx, want_k = scan_order_f_u(S, "cpu")
    same("scan order", _t(idx), want_idx)
    same("scan order keys", _t(k), want_k)
    assert int(want_idx[-1]) == S.n - 1 and sorted(want_idx[want_k == 2].tolist()) == [S.lin(S.nan_at), S.n - 1]
    bad = idx.copy()
    bad[len(bad) // 2] ^= 1
    with pytest.raises(AssertionError):
        same("scan order", _t(bad), want_idx)
    with pytest.raises(AssertionError):
        same("scan order", _t(idx[:-1]), want_idx)
    with pytest.raises(AssertionError):
        same("scan order keys", _t(np.zeros_like(k)), want_k)


def test_grouped_closed_form_is_the_restatement():
    occ, keys = _small_arrays()
    S = SMALL
    for draw in (None, [7, 2 ** 32 - 1], [9], [8]):
        gi, gk, group_keys, group_offsets = R.grouped(*R.select_key_field(keys, occ, draw, draw_zero=False))
        wi, wk, wkeys, woffs = grouped_by_key(S, "cpu", draw)
        same("grouped indices", _t(gi), wi)
        same("grouped keys", _t(gk), wk)
        assert group_keys.tolist() == wkeys and group_offsets.tolist() == woffs and woffs[-1] == len(gi)
        if draw is None:
            assert wkeys == [7, 9, 2 ** 31 + 5, 2 ** 32 - 1] and woffs[-1] == S.volume
            bad = gi.copy()
            bad[[woffs[2], woffs[2] + 1]] = bad[[woffs[2] + 1, woffs[2]]]      # two neighbours of one group swapped
            with pytest.raises(AssertionError):
                same("grouped indices", _t(bad), wi)
    assert grouped_by_key(S, "cpu", [7, 2 ** 32 - 1])[2] == [7, 2 ** 32 - 1] and grouped_by_key(S, "cpu", [8])[3] == [0]


def test_chunked_surface_rule_is_the_restatement():
    occ, _ = _small_arrays()
    S = SMALL
    t = torch.from_numpy(occ)
    for mask in (7, 5, 2):
        want = R.select_occupancy(occ, mask, surface_only=True)[0]
        assert 0 < len(want) < S.n
        for chunk in (1, 4, S.shape[0]):
            assert check_surface("surface", _t(want), t, chunk, mask) == len(want)
            flipped = want.copy()
            flipped[len(want) // 3] ^= 1
            for bad in (np.delete(want, len(want) // 2), flipped, want[:-1], np.append(want, S.n)):
                with pytest.raises(AssertionError):
                    check_surface("surface", _t(bad), t, chunk, mask)
    # what the scene must show: the box's cells on a grid face are no surface by that face alone, the U corner and its F neighbours are
    surf = torch.cat([s for _, s in surface_chunks(t, 4)]).numpy()
    assert np.array_equal(surf, R.occ_surface(occ))
    x0, x1, y0, y1 = S.box
    assert not surf[x1 - 1, y1 - 2, 5] and not surf[x1 - 1, y0 + 2, 0] and surf[x0, y0 + 2, 5] and surf[x0 - 1, y0 + 2, 5]
    assert surf[S.last] and surf[S.last[0], S.last[1], S.last[2] - 1] and not surf[S.nan_at]
    # on random classes as well, every chunk size
    rng = np.random.default_rng(4)
    noise = rng.choice(np.array([0.0, 0.5, 1.0, np.nan, 0.50000006, -3.0], np.float32), size=(7, 5, 6))
    for chunk in (1, 2, 3, 7):
        assert np.array_equal(torch.cat([s for _, s in surface_chunks(torch.from_numpy(noise), chunk)]).numpy(), R.occ_surface(noise))


def test_plane_table_is_the_restatement_on_the_full_field():
    S = SMALL
    d = build_field(S, "cpu").numpy()
    assert np.isnan(d[S.last]) and np.signbit(d[S.neg_zero_at]) and d[S.neg_zero_at] == 0 and np.isinf(d[S.inf_at])
    assert R.sdf_extrema(d) == (-S.box[0] * 0.25, float("inf"))
    full = R.sdf_colors(d, ALPHA)
    words = torch.from_numpy(full.view(np.int32).copy())
    for chunk in (1, 4, S.shape[0]):
        check_colors("colours", words.clone(), S, ALPHA, chunk)
    for at in ((0, 0, 0), (S.box[0], 3, 3), S.last, S.neg_zero_at, S.inf_at, (S.shape[0] - 1, 0, 1)):
        bad = words.clone()
        bad[at][1] ^= 1 << 22
        with pytest.raises(AssertionError):
            check_colors("colours", bad, S, ALPHA, 4)
    table, special = color_table(S, ALPHA)
    assert table[0].tolist() == [1.0, 0.0, 0.0, ALPHA] and table[S.box[0]].tolist() == [0.0, 0.0, 1.0, ALPHA]
    assert table[-1, 1] == np.float32(0.2) and np.isnan(special[0, 1]) and special[1].tolist() == special[2].tolist() == [0.0, 0.0, 1.0, ALPHA]
    # the SDF rule's totals and indices on the same field, and on the one that is negative only inside the box
    assert len(R.select_sdf(d)[0]) == sdf_total(S)
    inside = np.ones(S.shape, np.float32)
    inside[S.box[0]:S.box[1], S.box[2]:S.box[3]] = -1.0
    same("sdf rule", _t(R.select_sdf(inside)[0]), box_indices(S, "cpu"))


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """A context of its own for the largest grid: its scratch goes when the module ends."""
    from sdf_tools_amd import capi
    ctx = capi.SdfGpu(0)
    yield ctx
    ctx.close()
    torch.cuda.empty_cache()


def _need(nbytes):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip("needs %.1f GB of free device memory, %.1f GB are free" % (nbytes / 1e9, free / 1e9))


def _scratch(S):
    """the library's scratch for one selection over the grid: a bit per voxel, a count per tile"""
    return S.n // 8 + S.n // 1024 + (1 << 20)


@pytest.fixture(scope="module")
def records(big):
    """The 17 GB of records, shared by the cell tests (none of them writes to it)."""
    _need(BIG.n * 8 + _scratch(BIG) + SLACK)
    cells = build_cells(BIG, torch.device("cuda", 0))
    torch.cuda.synchronize()
    yield cells
    del cells
    torch.cuda.empty_cache()


def _words(count):
    """`count` words of sentinel on the device and one more behind them"""
    return torch.full((int(count) + 1,), SENTINEL, dtype=torch.int32, device="cuda")


def _taken(buf, count):
    """the first `count` words as int64 values; the word behind them must be intact"""
    assert int(buf[count]) == SENTINEL, "a word behind an output was written"
    return _u32(buf[:count])


def _untouched(*bufs):
    for b in bufs:
        assert bool((b == SENTINEL).all()), "a refused call stored results"


@gpu_test
def test_totals_above_2_31(big, records):
    from sdf_tools_amd import capi
    S = BIG
    want = occupancy_totals(S)
    assert want[7] > 2 ** 31 and want[3] > 2 ** 31
    for mask in (7, 3, 2):
        total, _ = big.display_select_cells_device(records.data_ptr(), S.shape, capi.DISPLAY_OCCUPANCY, 8, 0, 4, class_mask=mask)
        print("\n[display-large] class_mask %d: total %d, expected %d" % (mask, total, want[mask]))
        assert isinstance(total, int) and total == want[mask]
    total, _ = big.display_select_cells_device(records.data_ptr(), S.shape, capi.DISPLAY_KEY_FIELD, 8, 0, 4)     # every key, zero included
    assert total == S.n
    for mask in (7, 2):                                             # a capacity below the total: refused with the total, nothing stored
        for cap in (16, 0):
            idx, keys = _words(16), _words(16)
            with pytest.raises(capi.SdfGpuError) as e:
                big.display_select_cells_device(records.data_ptr(), S.shape, capi.DISPLAY_OCCUPANCY, 8, 0, 4, class_mask=mask,
                                                d_indices=idx.data_ptr(), d_keys=keys.data_ptr(), capacity=cap)
            assert e.value.code == -1 and e.value.total == want[mask]
            _untouched(idx, keys)
    torch.cuda.empty_cache()


@gpu_test
def test_scan_order_with_indices_past_2_31(big, records):
    from sdf_tools_amd import capi
    S = BIG
    _need(S.volume * 8 * 6 + SLACK)
    total, _ = big.display_select_cells_device(records.data_ptr(), S.shape, capi.DISPLAY_OCCUPANCY, 8, 0, 4, class_mask=5)
    assert total == S.volume
    idx, keys = _words(total), _words(total)
    t, _ = big.display_select_cells_device(records.data_ptr(), S.shape, capi.DISPLAY_OCCUPANCY, 8, 0, 4, class_mask=5, d_indices=idx.data_ptr(),
                                           d_keys=keys.data_ptr(), capacity=total)
    assert t == total
    want_idx, want_keys = scan_order_f_u(S, records.device)
    got = _taken(idx, total)
    same("scan order indices", got, want_idx)
    same("scan order keys", _taken(keys, total), want_keys)
    assert int(got[-1]) == S.n - 1 and int((got >= 2 ** 31).sum()) == S.n - 2 ** 31 and int(got[0]) == S.lin((S.box[0], S.box[2], 0))
    del idx, keys, got, want_idx, want_keys
    torch.cuda.empty_cache()


@gpu_test
def test_surface_rule_at_large_indices(big, records):
    from sdf_tools_amd import capi
    S = BIG
    chunk = 16
    _need((chunk + 2) * S.shape[1] * S.shape[2] * 64 + SLACK)       # the chunk's class planes, the pool's result and its indices
    total, _ = big.display_select_cells_device(records.data_ptr(), S.shape, capi.DISPLAY_OCCUPANCY, 8, 0, 4, class_mask=7, surface_only=True)
    print("\n[display-large] surface voxels: %d" % total)
    assert 0 < total < S.volume
    idx = _words(total)
    t, _ = big.display_select_cells_device(records.data_ptr(), S.shape, capi.DISPLAY_OCCUPANCY, 8, 0, 4, class_mask=7, surface_only=True,
                                           d_indices=idx.data_ptr(), capacity=total)
    assert t == total
    got = _taken(idx, total)
    occ = records.view(torch.float32)[..., 0]
    assert check_surface("surface rule", got, occ, chunk) == total
    assert int(got[-1]) == S.n - 1 and int((got >= 2 ** 31).sum()) > 0
    del idx, got, occ
    torch.cuda.empty_cache()


def _grouped_call(big, records, S, draw, draw_zero):
    """count, the refusal with a group capacity of 0 (which returns the group count), then exact buffers with sentinels"""
    from sdf_tools_amd import capi
    opts = dict(draw_keys=draw, draw_zero=draw_zero)
    args = (records.data_ptr(), S.shape, capi.DISPLAY_KEY_FIELD, 8, 0, 4)
    total, _ = big.display_select_cells_device(*args, **opts)
    idx, keys = _words(total), _words(total)
    gk0, go0 = _words(0), _words(1)
    with pytest.raises(capi.SdfGpuError) as e:
        big.display_select_cells_device(*args, grouped=True, d_indices=idx.data_ptr(), capacity=total, d_group_keys=gk0.data_ptr(),
                                        d_group_offsets=go0.data_ptr(), group_capacity=0, **opts)
    assert e.value.code == -1 and e.value.total == total and e.value.groups > 0
    _untouched(gk0, go0)
    groups = e.value.groups
    idx = _words(total)
    gk, go = _words(groups), _words(groups + 1)
    t, g = big.display_select_cells_device(*args, grouped=True, d_indices=idx.data_ptr(), d_keys=keys.data_ptr(), capacity=total,
                                           d_group_keys=gk.data_ptr(), d_group_offsets=go.data_ptr(), group_capacity=groups, **opts)
    assert (t, g) == (total, groups)
    return _taken(idx, total), _taken(keys, total), _taken(gk, groups).tolist(), _taken(go, groups + 1).tolist()


@gpu_test
def test_grouped_past_one_scan_segment_in_both_stages(big, records):
    S = BIG
    k = _constants()
    _need(S.volume * 8 * 10 + SLACK)                                # indices, keys, the sort's pair buffers, the closed form
    for draw, draw_zero, want_keys in ((None, False, [7, LAST_KEY, 2 ** 31 + 5, 2 ** 32 - 1]), ([7, 2 ** 32 - 1], True, [7, 2 ** 32 - 1])):
        gi, gk, group_keys, group_offsets = _grouped_call(big, records, S, draw, draw_zero)
        wi, wk, wkeys, woffs = grouped_by_key(S, records.device, draw)
        print("\n[display-large] grouped, draw %s: groups %s offsets %s" % (draw, group_keys, group_offsets))
        assert wkeys == want_keys and group_keys == wkeys and group_offsets == woffs and group_offsets[len(group_keys)] == gi.numel()
        if draw is None:
            assert gi.numel() == S.volume > k["kDpScanSeg"] * k["kDpTile"]     # the second stage spans more than one scan segment
        for g, key in enumerate(wkeys):
            a, b = woffs[g], woffs[g + 1]
            same("group %d (key %d) indices" % (g, key), gi[a:b], wi[a:b])
            assert bool((gk[a:b] == key).all()), "group %d: keys" % g
        same("grouped keys", gk, wk)
        del gi, gk, wi, wk
        torch.cuda.empty_cache()


@gpu_test
def test_sdf_rule_past_2_31(big):
    from sdf_tools_amd import capi
    S = BIG
    _need(S.n * 4 + _scratch(S) + S.volume * 8 * 3 + SLACK)
    d = build_field(S, torch.device("cuda", 0))
    torch.cuda.synchronize()
    total = big.display_select_sdf_device(d.data_ptr(), S.shape)
    print("\n[display-large] sdf rule: total %d, expected %d" % (total, sdf_total(S)))
    assert total == sdf_total(S)
    for cap in (16, 0):
        buf = _words(16)
        with pytest.raises(capi.SdfGpuError) as e:
            big.display_select_sdf_device(d.data_ptr(), S.shape, buf.data_ptr(), cap)
        assert e.value.code == -1 and e.value.total == sdf_total(S)
        _untouched(buf)
    # indices: a field that is negative only inside the box (which holds the last voxel)
    x0, x1, y0, y1 = S.box
    d.fill_(1.0)
    d[x0:x1, y0:y1] = -1.0
    torch.cuda.synchronize()
    total = big.display_select_sdf_device(d.data_ptr(), S.shape)
    assert total == S.volume
    buf = _words(total)
    assert big.display_select_sdf_device(d.data_ptr(), S.shape, buf.data_ptr(), total) == total
    got = _taken(buf, total)
    same("sdf rule indices", got, box_indices(S, d.device))
    assert int(got[-1]) == S.n - 1
    del d, buf, got
    torch.cuda.empty_cache()


@gpu_test
def test_sdf_colour_map_past_2_31(big):
    S = BIG
    _need(S.n * 4 + S.n * 16 + SLACK)
    dev = torch.device("cuda", 0)
    d = build_field(S, dev)
    out = torch.full((S.n * 4 + 1,), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    big.display_sdf_colors_device(d.data_ptr(), S.shape, ALPHA, out.data_ptr())
    torch.cuda.synchronize()
    assert int(out[S.n * 4]) == SENTINEL, "a word behind the colours was written"
    check_colors("colour map", out[:S.n * 4].view(S.shape + (4,)), S, ALPHA, 30)
    del d, out
    torch.cuda.empty_cache()


@gpu_test
def test_expand_with_indices_past_2_31(big):
    S = BIG
    count = 4097
    rng = np.random.default_rng(8)
    idx = np.concatenate([rng.integers(0, 2 ** 31, size=count // 2), rng.integers(2 ** 31, S.n, size=count - count // 2)]).astype(np.uint32)
    rng.shuffle(idx)
    idx[[0, 1, 2, 3, 4, count - 1]] = (0, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, S.n - 1, S.n - 1)
    keys = rng.choice(np.array([0, 1, 2, 3, 2 ** 31, 2 ** 32 - 1], np.uint32), size=count)
    table = rng.random((3, 4)).astype(np.float32)
    default, cell = (0.5, 0.25, 0.125, 1.0), (0.1, 0.25, 3.0)
    d_idx, d_keys, d_table = (torch.from_numpy(a.view(np.int32).reshape(-1).copy()).cuda() for a in (idx, keys, table))
    pts, col = _words(count * 6), _words(count * 4)
    big.display_expand_device(d_idx.data_ptr(), count, S.shape, cell, d_points=pts.data_ptr(), d_colors=col.data_ptr(), d_keys=d_keys.data_ptr(),
                              d_color_table=d_table.data_ptr(), table_entries=3, default_color=default)
    torch.cuda.synchronize()
    assert int(pts[count * 6]) == SENTINEL and int(col[count * 4]) == SENTINEL
    want = R.points(idx, S.shape, cell)
    got = pts[:count * 6].cpu().numpy().view(np.float64).reshape(count, 3)
    assert got.tobytes() == want.tobytes(), "points differ at elements %s" % np.flatnonzero((got != want).any(axis=1))[:5].tolist()
    assert want[4].tolist() == [0.1 * 1289.5, 0.25 * 1289.5, 3.0 * 1290.5] and want[2, 0] == 0.1 * 1289.5
    assert col[:count * 4].cpu().numpy().view(np.float32).reshape(count, 4).tobytes() == R.table_colors(keys, table, default).tobytes()
