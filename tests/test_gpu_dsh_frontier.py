"""GPU: frontier cells of the dynamic spatial hashed map (sdfgpu_dsh_frontier_window*, sdfgpu_dsh_frontier_cells*) and the component
statistics (sdfgpu_component_stats_device), include/sdfgpu.h "Frontier cells" and "Component statistics", DESIGN.md section 34, against
the restatement of their contract (tests/dsh_frontier_restated.py on a tests/dsh_restated.py map).  Every expected result is the
restatement's, byte for byte; the map's export and info are compared around every call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dsh_frontier_restated as F
import dsh_restated as R
from sdf_tools_amd import capi
from test_gpu_dsh import Pair
from test_gpu_dsh_rays import FRAMES, to_world

pytestmark = pytest.mark.gpu

FREE, FILLED, UNKNOWN = R.record(0.0, 0x10), R.record(1.0, 0x20), R.record(0.5, 0x30)
NAN_CELL = R.record_bits(0x7FC00001, 5)
BELOW, ABOVE = R.record_bits(0x3EFFFFFF, 6), R.record_bits(0x3F000001, 7)     # the two float neighbours of 0.5f
DEFAULTS = {"unknown": R.record(0.5, 0xABCD), "free": R.record(0.0, 0xABCE), "filled": R.record(1.0, 0xABCF)}
RULES = (0, capi.DSH_FRONTIER_26)
SHAPES = [(1, 1, 1), (3, 2, 5), (4, 4, 4), (8, 8, 32), (32768, 1, 1)]
WINDOWS = [(5, 3, 33), (7, 6, 31), (4, 4, 64), (3, 3, 3), (1, 1, 1)]
# chunks per axis of a scene, and the cells along x that it sprinkles single cells into and lists (None: all of them)
LATTICE = {(1, 1, 1): ((20, 20, 20), None), (3, 2, 5): ((4, 5, 3), None), (4, 4, 4): ((4, 4, 4), None), (8, 8, 32): ((2, 2, 2), None),
           (32768, 1, 1): ((2, 7, 7), (-48, 48))}
CANARY = 0x5A5A5A5A5A5A5A5A


def cells_of(a):
    return [tuple(int(v) for v in row) for row in a]


def unpack(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(np.asarray(bits, np.uint32).view(np.uint8), bitorder="little")[:n].reshape(shape).astype(bool)


class FrontierPair(Pair):
    """the map on the GPU and its restatement; every frontier call is compared with the restatement's and must leave the map as it was"""

    def snapshot(self):
        chunks, cells = self.gpu.export()
        return chunks.tobytes(), cells.tobytes(), self.gpu.info()

    def unchanged(self, before, what):
        after = self.snapshot()
        assert after[:2] == before[:2], what + ": the call changed the map's export"
        drop = lambda info: {k: v for k, v in info.items() if k != "scratch_bytes"}
        assert drop(after[2]) == drop(before[2]), what + ": info"

    def window(self, lower, shape, flags, what=""):
        """both forms of the window call against the restatement; returns the restatement's bool [shape]"""
        before = self.snapshot()
        bits = self.gpu.frontier_window(lower, shape, flags)
        n = int(np.prod(shape))
        d_bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device="cuda")     # (every word is written whole: no clearing)
        self.gpu.frontier_window_device(lower, shape, flags, d_bits.data_ptr())
        torch.cuda.synchronize()
        self.unchanged(before, what)
        want = F.frontier_window(self.ref, lower, shape, flags)
        want_bits = R.pack_bits(want)
        assert bits.tobytes() == want_bits.tobytes(), "%s: window %s at %s, flags %d: %d voxels differ" % (
            what, shape, tuple(lower), flags, (unpack(bits, shape) != want).sum())
        assert d_bits.cpu().numpy().view(np.uint32).tobytes() == want_bits.tobytes(), what + ": the device form's words"
        return want

    def cells(self, box, flags, what=""):
        """both forms of the list call against the restatement, the device form at capacity 0, one short and exact; returns the list"""
        lower, extent = (None, None) if box is None else box
        before = self.snapshot()
        got = self.gpu.frontier_cells(lower, extent, flags)
        want = F.frontier_cells(self.ref, box, flags)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), "%s: list of box %s, flags %d: got %d cells, want %d" % (
            what, box, flags, len(got), len(want))
        total = len(want)
        assert self.gpu.frontier_cells_device(lower, extent, flags, 0, 0) == total
        d_cells = torch.full((total + 1, 3), CANARY, dtype=torch.int64, device="cuda")
        if total:
            assert self.gpu.frontier_cells_device(lower, extent, flags, d_cells.data_ptr(), total - 1) == total
            torch.cuda.synchronize()
            assert (d_cells == CANARY).all(), what + ": a list one cell short of its total is not written"
        assert self.gpu.frontier_cells_device(lower, extent, flags, d_cells.data_ptr(), total) == total
        torch.cuda.synchronize()
        back = d_cells.cpu().numpy()
        assert back[:total].tobytes() == want.tobytes() and (back[total:] == CANARY).all(), what + ": the device form's list and the cell behind it"
        self.unchanged(before, what)
        return want


@pytest.fixture
def pair(gpu):
    made = []

    def make(**kw):
        made.append(FrontierPair(gpu, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


def build_scene(p, rng, origin, cell, dims):
    """Chunks of all four kinds on a small lattice around the grid's origin (three in eight chunk-filled free, two unknown, one
    filled, two absent), then single cells of every class in every second chunk of each kind, which makes cell-filled chunks out of
    all four.  Returns the cells the scene touched as (lower, extent)."""
    n = np.array(dims)
    lattice, xspan = LATTICE[tuple(dims)]
    first = -(np.array(lattice) // 2)
    coords = np.stack(np.meshgrid(*[np.arange(f, f + k) for f, k in zip(first, lattice)], indexing="ij"), -1).reshape(-1, 3)
    kind = rng.permutation(len(coords)) % 8
    centre = lambda c: to_world(origin, (c + 0.5) * n, cell)
    p.set_chunks(centre(coords[kind < 3]), FREE)
    p.set_chunks(centre(coords[(kind == 3) | (kind == 4)]), UNKNOWN)
    p.set_chunks(centre(coords[kind == 5]), np.array([R.record(0.75 + 0.01 * (k % 20), k) for k in range((kind == 5).sum())], np.uint64))
    lo, hi = first * n, (first + np.array(lattice)) * n
    if xspan:
        lo[0], hi[0] = xspan
    into = coords[kind % 2 == 0]                                               # free, free, unknown and absent chunks
    k = max(len(into) // 2, 40) if max(dims) < 8 else 400
    chunks = into[rng.integers(0, len(into), k)]
    local = rng.integers(0, n, (k, 3))
    if xspan:                                                                  # (within the span: the chunk's last cells below zero, its first above)
        local[:, 0] = np.where(chunks[:, 0] < 0, n[0] - 1 - rng.integers(0, -xspan[0], k), rng.integers(0, xspan[1], k))
    values = [UNKNOWN, FREE, FILLED, UNKNOWN, NAN_CELL, FREE, BELOW, ABOVE]
    p.set_cells(to_world(origin, chunks * n + local + 0.5, cell), np.array([values[j % 8] for j in range(k)], np.uint64))
    return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo)


def kinds_seen(ref, six, all_26):
    """how many frontier cells have an unknown neighbour (under the 26-rule) in their own chunk, in another live chunk, in an absent
    chunk; and how many are found under 26 but not under 6"""
    seen = {"same": 0, "live": 0, "absent": 0}
    for i in cells_of(all_26):
        for k in F.deciding_kinds(ref, i, capi.DSH_FRONTIER_26):
            seen[k] += 1
    seen["only_26"] = len(set(cells_of(all_26)) - set(cells_of(six)))
    return seen


# ---- shapes, frames, defaults -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("default", list(DEFAULTS))
def test_random_maps_in_every_chunk_shape(pair, dims, frame, default):
    origin, inverse, cell = FRAMES[frame]
    p = pair(inverse=inverse, cell_size=cell, chunk_dims=dims, default=DEFAULTS[default])
    rng = np.random.default_rng(341 + len(default))
    lower, extent = build_scene(p, rng, origin, cell, dims)
    p.check("the scene")
    assert min(p.ref.counts()) > 0, "chunk-filled and cell-filled chunks"
    # the list: over the whole map, or (the chunk of 32768 cells) over the box of the cells the scene touched
    box = (lower, extent) if LATTICE[dims][1] else None
    lists = [p.cells(box, flags, "the scene") for flags in RULES]
    seen = kinds_seen(p.ref, *lists)
    # the kinds a case can hold: a neighbour in the cell's own chunk needs a chunk of more than one cell, and an absent chunk is
    # unknown only under the unknown default
    want_kinds = ["live", "only_26"] + (["same"] if max(dims) > 1 else []) + (["absent"] if default == "unknown" else [])
    for k in want_kinds:
        assert seen[k] >= 20, "%d frontier cells of kind %s: %s" % (seen[k], k, seen)
    if default != "unknown":
        assert seen["absent"] == 0
    # windows that cut chunks, ragged last words; the two forms against each other on every window
    set_bits = on_face = 0
    for shape in WINDOWS:
        for flags in RULES:
            at = tuple(int(v) for v in rng.integers(np.array(lower), np.array(lower) + np.maximum(np.array(extent) - np.array(shape) // 2, 1)))
            want = p.window(at, shape, flags, "the scene")
            listed = p.cells((at, shape), flags, "the window as a box")
            assert int(want.sum()) == len(listed) and set(cells_of(np.argwhere(want) + np.array(at))) == set(cells_of(listed))
            set_bits += len(listed)
            for i in cells_of(listed):                                         # on the window's face, decided from outside it
                nb = [tuple(np.add(i, d)) for d in F.offsets(flags) if F.is_unknown(p.ref.get_cell(tuple(int(v) for v in np.add(i, d)))[0])]
                on_face += all(any(not at[a] <= j[a] < at[a] + shape[a] for a in range(3)) for j in nb)
    assert set_bits >= 20 and on_face >= 3, (set_bits, on_face)


# ---- boxes -------------------------------------------------------------------------------------------------------------------------------------
def test_boxes_that_cut_chunks_hold_no_live_chunk_or_equal_one_cell(pair):
    dims = (3, 2, 5)
    p = pair(chunk_dims=dims, default=DEFAULTS["unknown"])
    rng = np.random.default_rng(343)
    lower, extent = build_scene(p, rng, np.eye(4), 1.0, dims)
    whole = [p.cells(None, flags, "whole") for flags in RULES]
    for flags, everything in zip(RULES, whole):
        assert len(everything) > 100
        assert len(p.cells(((1000, 1000, 1000), (7, 7, 7)), flags, "no live chunk")) == 0
        assert len(p.cells(((-(1 << 62), -(1 << 62), -(1 << 62)), (5, 5, 5)), flags, "beyond the chunk range")) == 0
        big = ((-(1 << 62), -(1 << 62), -(1 << 62)), ((1 << 63) - 1, (1 << 63) - 1, (1 << 63) - 1))
        assert p.cells(big, flags, "a box of almost all int64").tobytes() == everything.tobytes()
        cut = p.cells(((-4, -3, -2), (8, 5, 9)), flags, "cuts chunks")
        assert 0 < len(cut) < len(everything)
        for i in cells_of(everything[:: max(len(everything) // 12, 1)]):
            assert cells_of(p.cells((i, (1, 1, 1)), flags, "one cell")) == [i]
            beside = (i[0], i[1], i[2] + 1)
            assert len(p.cells((beside, (1, 1, 1)), flags, "one cell")) == int(F.is_frontier(p.ref, beside, flags))
    assert len(whole[0]) < len(whole[1])


def test_chunks_at_both_ends_of_the_key_range(pair):
    dims = (3, 2, 5)
    n = np.array(dims)
    ends = np.array([[-(1 << 20)] * 3, [(1 << 20) - 1] * 3])
    for name, default in DEFAULTS.items():
        p = pair(chunk_dims=dims, default=default)
        p.set_chunks((ends + 0.5) * n, FREE)
        p.set_cells((ends * n + np.array([[1, 0, 2], [1, 1, 2]])) + 0.5, UNKNOWN)
        for flags in RULES:
            listed = cells_of(p.cells(None, flags, "the two end chunks"))
            # the outermost cell of each chunk: every neighbour beyond it is out of range and reads the default
            for c, step in zip(ends, (-1, 1)):
                corner = tuple(int(v) for v in c * n + (0 if step < 0 else n - 1))
                assert p.ref.get_cell(tuple(v + step for v in corner)) == (default, R.NOT_FOUND)
                assert (corner in listed) == (name == "unknown")
                at = tuple(int(v) for v in c * n - 1)
                want = p.window(at, (5, 4, 7), flags, "around an end chunk")
                inside = [i for i in listed if all(at[a] <= i[a] < at[a] + (5, 4, 7)[a] for a in range(3))]
                assert want.sum() == len(inside) == len(listed) // 2 > 0
            if name == "unknown":
                assert len(listed) == 2 * 29, "n_y = 2: every free cell of the chunks lies on a face with an absent chunk behind it"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_map_alone(pair):
    p = pair(chunk_dims=(4, 4, 4), default=DEFAULTS["unknown"])
    p.set_cells(np.array([[0.5, 0.5, 0.5]]), FREE)
    before = p.snapshot()
    m, lib = p.gpu, p.gpu._lib
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    lo, ext = np.zeros(3, np.int64), np.ones(3, np.int64)
    total = capi.ctypes.c_int64(-7)
    bad = capi.SdfGpuError

    def refused(call, *args):
        with pytest.raises(bad) as e:
            m._check(call(m._m, *args))
        assert e.value.code == -1
    refused(lib.sdfgpu_dsh_frontier_window_device, lo.ctypes.data, 2, 2, 2, 2, d.data_ptr(), None)           # an unknown flag bit
    refused(lib.sdfgpu_dsh_frontier_window_device, lo.ctypes.data, 2, 2, 2, 0, None, None)                   # no bits
    refused(lib.sdfgpu_dsh_frontier_window_device, lo.ctypes.data, 2, 2, 2, 0, d.data_ptr() + 2, None)       # misaligned
    refused(lib.sdfgpu_dsh_frontier_window_device, None, 2, 2, 2, 0, d.data_ptr(), None)
    refused(lib.sdfgpu_dsh_frontier_window_device, lo.ctypes.data, 0, 2, 2, 0, d.data_ptr(), None)
    refused(lib.sdfgpu_dsh_frontier_window_device, lo.ctypes.data, 1 << 16, 1 << 16, 1, 0, d.data_ptr(), None)   # 2^32 voxels
    refused(lib.sdfgpu_dsh_frontier_window, lo.ctypes.data, 2, 2, 2, 4, np.zeros(1, np.uint32).ctypes.data)
    by_ref = capi.ctypes.byref(total)
    refused(lib.sdfgpu_dsh_frontier_cells_device, lo.ctypes.data, ext.ctypes.data, 2, d.data_ptr(), 4, by_ref, None)
    refused(lib.sdfgpu_dsh_frontier_cells_device, lo.ctypes.data, ext.ctypes.data, 0, d.data_ptr(), 4, None, None)      # out_total is required
    refused(lib.sdfgpu_dsh_frontier_cells_device, lo.ctypes.data, ext.ctypes.data, 0, None, 4, by_ref, None)           # a capacity without a buffer
    refused(lib.sdfgpu_dsh_frontier_cells_device, lo.ctypes.data, ext.ctypes.data, 0, d.data_ptr(), -1, by_ref, None)
    refused(lib.sdfgpu_dsh_frontier_cells_device, lo.ctypes.data, ext.ctypes.data, 0, d.data_ptr() + 4, 4, by_ref, None)
    refused(lib.sdfgpu_dsh_frontier_cells_device, lo.ctypes.data, None, 0, d.data_ptr(), 4, by_ref, None)              # half a box
    refused(lib.sdfgpu_dsh_frontier_cells_device, lo.ctypes.data, np.array([1, 0, 1], np.int64).ctypes.data, 0, d.data_ptr(), 4, by_ref, None)
    far = np.array([(1 << 63) - 2, 0, 0], np.int64)
    refused(lib.sdfgpu_dsh_frontier_cells_device, far.ctypes.data, np.array([3, 1, 1], np.int64).ctypes.data, 0, d.data_ptr(), 4, by_ref, None)
    refused(lib.sdfgpu_dsh_frontier_cells, lo.ctypes.data, ext.ctypes.data, 8, np.zeros(3, np.int64).ctypes.data, 1, by_ref)
    assert (d == 0).all()
    p.unchanged(before, "refusals")
    assert cells_of(p.cells(None, 0)) == [(0, 0, 0)]


# ---- many small maps on one handle -------------------------------------------------------------------------------------------------------------
def small_maps_on(ctx, count):
    rng = np.random.default_rng(344)
    values = [FREE, FREE, UNKNOWN, FILLED, NAN_CELL, FREE, UNKNOWN, BELOW]
    listed = 0
    for k in range(count):
        dims = tuple(int(v) for v in rng.integers(1, 5, 3))
        p = FrontierPair(ctx, chunk_dims=dims, default=list(DEFAULTS.values())[k % 3], initial_chunks=int(rng.integers(0, 3)))
        try:
            p.set_chunks(rng.integers(-6, 6, (6, 3)) + 0.5, np.array([values[int(v)] for v in rng.integers(0, 8, 6)], np.uint64))
            p.set_cells(rng.integers(-6, 6, (30, 3)) + 0.5, np.array([values[int(v)] for v in rng.integers(0, 8, 30)], np.uint64))
            flags = RULES[k % 2]
            got = p.gpu.frontier_cells(None, None, flags)
            want = F.frontier_cells(p.ref, None, flags)
            assert got.tobytes() == want.tobytes(), "map %d" % k
            at, shape = tuple(int(v) for v in rng.integers(-8, 2, 3)), tuple(int(v) for v in rng.integers(1, 12, 3))
            assert p.gpu.frontier_window(at, shape, flags).tobytes() == F.frontier_window_bits(p.ref, at, shape, flags).tobytes(), "map %d" % k
            listed += len(want)
        finally:
            p.close()
    return listed


def test_two_hundred_random_small_maps_on_one_handle(gpu):
    assert small_maps_on(gpu, 200) > 2000


def core_cases_on(ctx):
    """what the red-zone child runs: small maps, a scene of big chunks, the statistics"""
    small_maps_on(ctx, 30)
    for dims in [(3, 2, 5), (8, 8, 32)]:
        p = FrontierPair(ctx, chunk_dims=dims, default=DEFAULTS["unknown"])
        try:
            lower, extent = build_scene(p, np.random.default_rng(345), np.eye(4), 1.0, dims)
            for flags in RULES:
                p.cells(None, flags, "red zones")
                p.window(tuple(v - 1 for v in lower), (5, 3, 33), flags, "red zones")
        finally:
            p.close()
    for shape in STATS_SHAPES:
        stats_case(ctx, shape, 0.5, 346)


def test_the_core_cases_in_a_child_process_with_red_zones_from_the_environment():
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from sdf_tools_amd import capi\nimport test_gpu_dsh_frontier as T\n"
            "ctx = capi.SdfGpu(0)\nT.core_cases_on(ctx)\nctx.redzone_check()\nctx.close()\nprint('core cases clean')\n") % (tests, os.path.dirname(tests))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SDFGPU_REDZONE="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "core cases clean" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- component statistics -------------------------------------------------------------------------------------------------------------------
STATS_SHAPES = [(1, 1, 1), (5, 3, 33), (40, 40, 40)]


def stats_case(ctx, shape, density, seed):
    """labels from sdfgpu_components_bits_device on a random bit field, then the statistics against the restatement: at capacity 0,
    one short and exact, and with label_count cut short.  Returns the number of labels."""
    rng = np.random.default_rng(seed)
    filled = rng.random(shape) < density
    n = int(np.prod(shape))
    d_bits = torch.from_numpy(R.pack_bits(filled).view(np.int32)).cuda()
    d_labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    count = ctx.components_bits_device(d_bits.data_ptr(), shape, d_labels.data_ptr())
    labels = d_labels.cpu().numpy().view(np.uint32).reshape(shape)
    for label_count in sorted({count, max(count // 2, 1)}):
        want = F.component_stats_records(F.component_stats(filled, labels, shape, label_count), capi.COMPONENT_STATS_DTYPE)
        total = len(want)
        assert ctx.component_stats_device(d_bits.data_ptr(), d_labels.data_ptr(), shape, label_count) == total
        d_stats = torch.full((total + 1, 8), CANARY, dtype=torch.int64, device="cuda")
        if total:
            assert ctx.component_stats_device(d_bits.data_ptr(), d_labels.data_ptr(), shape, label_count, d_stats.data_ptr(), total - 1) == total
            torch.cuda.synchronize()
            assert (d_stats == CANARY).all(), "a list one record short of its total is not written"
        assert ctx.component_stats_device(d_bits.data_ptr(), d_labels.data_ptr(), shape, label_count, d_stats.data_ptr(), total) == total
        torch.cuda.synchronize()
        back = d_stats.cpu().numpy()
        assert back[:total].tobytes() == want.tobytes(), "%s, label_count %d: %d records" % (shape, label_count, total)
        assert (back[total:] == CANARY).all()
        if label_count == count:
            assert int(want["count"].sum()) == int(filled.sum()), "every set voxel is in one record"
    assert torch.equal(d_labels.cpu(), torch.from_numpy(labels.reshape(-1).view(np.int32))), "the labels are read only"
    return count


@pytest.mark.parametrize("shape", STATS_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("density", [0.5, 0.999], ids=["half", "dense"])
def test_component_stats_on_labels_of_the_components_call(gpu, shape, density):
    count = stats_case(gpu, shape, density, 347)
    if shape == (40, 40, 40):
        assert (count > 256) == (density == 0.5), "label counts on both sides of 256 (%d)" % count


def test_component_stats_refusals(gpu):
    lib = gpu._lib
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    total = capi.ctypes.c_int64(-7)
    by_ref = capi.ctypes.byref(total)
    ok = (d.data_ptr(), d.data_ptr() + 64, 2, 2, 2, 3, d.data_ptr() + 128, 3, by_ref, None)
    assert lib.sdfgpu_component_stats_device(gpu._h, *ok) == 0

    def refused(k, value):
        args = list(ok)
        args[k] = value
        with pytest.raises(capi.SdfGpuError) as e:
            gpu._check(lib.sdfgpu_component_stats_device(gpu._h, *args))
        assert e.value.code == -1
    refused(0, None)
    refused(1, None)
    refused(8, None)
    refused(0, d.data_ptr() + 2)
    refused(1, d.data_ptr() + 66)
    refused(6, d.data_ptr() + 132)
    refused(6, None)
    refused(7, -1)
    refused(2, 0)
    refused(2, 1 << 32)
    with pytest.raises(capi.SdfGpuError) as e:                                 # 2^31 voxels in a row: the bounding box is int32
        gpu._check(lib.sdfgpu_component_stats_device(gpu._h, d.data_ptr(), d.data_ptr() + 64, 1, 1 << 31, 1, 3, d.data_ptr() + 128, 3, by_ref, None))
    assert e.value.code == -1
    assert (d == 0).all()
