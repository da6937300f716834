"""Helpers of the display-export GPU tests: one selection through the host and the device entry points with sentinel words
behind every output, its reference from tests/display_restated.py, and the seeded random cases of the fuzz, half of them on the scenes
of tests/analysis_scenes.py and tests/scenes.py (which a child process runs under SDFGPU_REDZONE=1, so they live in a module of their
own)."""
import numpy as np
import torch

import analysis_scenes as A
import display_restated as R
import scenes
import stream_harness as H
from sdf_tools_amd import capi

SENTINEL = 0x5A5A5A5A
OCC_VALUES = np.array([0.0, 0.25, 0.5, 0.50000006, 0.75, 1.0, -10000.0, np.nan], np.float32)   # (tests/test_gpu_component_surfaces.py)
DEFAULTS = dict(class_mask=7, surface_only=False, draw_keys=None, draw_zero=True)


def dev(a):
    """numpy array -> device bytes"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def words(count):
    """`count` uint32 words of sentinel on the device, and one more behind them"""
    return torch.full((int(count) + 1,), SENTINEL, dtype=torch.int32, device="cuda")


def host_words(t, count):
    """the first `count` words of such a buffer; the words behind them must be intact"""
    w = t.cpu().numpy().view(np.uint32)
    assert (w[count:] == SENTINEL).all(), "a word behind an output was written"
    return w[:count].copy()


def reference(occ, keys, rule, grouped, **opts):
    o = dict(DEFAULTS, **opts)
    if rule == capi.DISPLAY_OCCUPANCY:
        idx, k = R.select_occupancy(occ, o["class_mask"], o["surface_only"])
    else:
        idx, k = R.select_key_field(keys, occ, o["draw_keys"], o["draw_zero"], o["class_mask"])
    return R.grouped(idx, k) if grouped else (idx, k)


def run_host(ctx, cells, shape, rule, stride, grouped, offsets=(0, 4), **opts):
    """offsets: (occupancy_offset, key_offset) of the records"""
    before = cells.copy()
    got = ctx.display_select_cells(cells, shape, rule, stride, offsets[0], offsets[1], grouped=grouped, **dict(DEFAULTS, **opts))
    assert np.array_equal(cells, before), "the records are read only"
    return got


def run_device(ctx, cells, shape, rule, stride, grouped, stream=0, offsets=(0, 4), **opts):
    """count first, then buffers of exactly the total (and the group count) with a sentinel word behind each"""
    o = dict(DEFAULTS, **opts)
    occ_off, key_off = offsets
    d_cells = dev(cells)
    total, _ = ctx.display_select_cells_device(d_cells.data_ptr(), shape, rule, stride, occ_off, key_off, stream=stream, **o)
    idx, keys = words(total), words(total)
    if not grouped:
        t, _ = ctx.display_select_cells_device(d_cells.data_ptr(), shape, rule, stride, occ_off, key_off, d_indices=idx.data_ptr(), d_keys=keys.data_ptr(),
                                               capacity=total, stream=stream, **o)
        assert t == total
        return host_words(idx, total), host_words(keys, total)
    groups = None
    try:                                                        # group capacity 0: the count of groups comes back with the refusal
        ctx.display_select_cells_device(d_cells.data_ptr(), shape, rule, stride, occ_off, key_off, grouped=True, d_indices=idx.data_ptr(), capacity=total,
                                        d_group_keys=words(0).data_ptr(), d_group_offsets=words(1).data_ptr(), group_capacity=0,
                                        stream=stream, **o)
        groups = 0
    except capi.SdfGpuError as e:
        assert e.code == -1 and e.total == total and e.groups > 0, str(e)
        groups = e.groups
    idx = words(total)
    gk, go = words(groups), words(groups + 1)
    t, g = ctx.display_select_cells_device(d_cells.data_ptr(), shape, rule, stride, occ_off, key_off, grouped=True, d_indices=idx.data_ptr(),
                                           d_keys=keys.data_ptr(), capacity=total, d_group_keys=gk.data_ptr(), d_group_offsets=go.data_ptr(),
                                           group_capacity=groups, stream=stream, **o)
    assert (t, g) == (total, groups)
    return host_words(idx, total), host_words(keys, total), host_words(gk, groups), host_words(go, groups + 1)


def same(what, got, want):
    assert len(got) == len(want), what
    for name, g, w in zip(("indices", "keys", "group_keys", "group_offsets"), got, want):
        assert g.dtype == np.uint32 and np.array_equal(g, w), "%s: %s differ (%d got, %d expected)" % (what, name, len(g), len(w))


def check(ctx, occ, keys, rule, strides=(8, 16), forms=("host", "device"), groupings=(False, True), layouts=None, filler=None, **opts):
    """every stride, form and result form of one selection against the restatement; returns the scan-order reference.
    layouts: (stride, occupancy_offset, key_offset) triples in place of `strides` (which puts the occupancy at 0 and the key at 4);
    filler: filler(stride) -> the words of R.cells_of that are neither field"""
    shape = occ.shape
    if layouts is None:
        layouts = [(stride, 0, 4) for stride in strides]
    for grouped in groupings:
        want = reference(occ, keys, rule, grouped, **opts)
        for stride, occ_off, key_off in layouts:
            cells = R.cells_of(occ, keys, stride, key_off, occ_off, None if filler is None else filler(stride))
            for form in forms:
                got = (run_host if form == "host" else run_device)(ctx, cells, shape, rule, stride, grouped, offsets=(occ_off, key_off), **opts)
                same("%s form, %d-byte records (occupancy at %d, key at %d), grouped %s, shape %s, rule %d, %s"
                     % (form, stride, occ_off, key_off, grouped, shape, rule, describe(opts)), got, want)
    return reference(occ, keys, rule, False, **opts)


def describe(opts):
    """the options of a case for a message: a long draw list by its length and ends"""
    d = opts.get("draw_keys")
    if d is None or len(d) <= 8:
        return opts
    return dict(opts, draw_keys="%d keys %d .. %d" % (len(d), int(d[0]), int(d[-1])))


KEY_POOLS = [[0], [5], [0, 1, 2, 3], [0, 1, 255, 256, 300], [0, 7, 65536, 70000, 2 ** 24 + 3], [0, 2 ** 31, 2 ** 32 - 1, 2 ** 32 - 2, 9],
             [2 ** 32 - 1], [2 ** 32 - 256, 2 ** 32 - 1, 2 ** 32 - 17]]


STRUCTURED = ("serpentine", "comb", "stripes", "checkerboard", "nested_shells", "tori_chain", "tutorial", "bindings")


def structured_mask(rng, name):
    """a mask from the generators of tests/analysis_scenes.py and tests/scenes.py, at a random shape <= 40^3 (the two reference scenes at
    their own shape or a crop of it)"""
    if name == "tutorial":
        lo = int(rng.integers(0, 12))
        return scenes.tutorial_scene()[0][lo:lo + int(rng.integers(8, 29)), lo:, :int(rng.integers(21, 41))]
    if name == "bindings":
        return scenes.test_bindings_scene()[0]
    shape = tuple(int(v) for v in rng.integers(17, 41, size=3))
    return np.asarray(getattr(A, name)(shape)) != 0


def random_case(rng, max_axis=40):
    """-> (occ, keys, rule, opts): a random rule and random options on either voxel noise (a random shape <= max_axis^3, i.i.d. occupancy
    values and keys) or a structured scene (large uniform regions: filled 1.0 / free 0.0 from a scene generator, one slab of unknown and
    NaN cells through it, keys that follow the scene's regions)"""
    if rng.random() < 0.5:
        mask = np.ascontiguousarray(structured_mask(rng, STRUCTURED[int(rng.integers(len(STRUCTURED)))]))
        shape = mask.shape
        occ = np.where(mask, np.float32(1.0), np.float32(0.0)).astype(np.float32)
        axis = int(rng.integers(3))
        at = int(rng.integers(shape[axis]))
        slab = [slice(None)] * 3
        slab[axis] = slice(at, at + 1 + int(rng.integers(2)))
        occ[tuple(slab)] = rng.choice(np.array([0.5, np.nan, 0.5, 0.50000006], np.float32), size=occ[tuple(slab)].shape)
        pool = np.array(KEY_POOLS[int(rng.integers(len(KEY_POOLS)))], np.uint32)
        x = np.arange(shape[0])[:, None, None] * len(pool) // shape[0]
        keys = np.where(mask, pool[(x + 1) % len(pool)], pool[x % len(pool)]).astype(np.uint32)      # slabs along x, shifted inside the filled region
    else:
        shape = tuple(int(v) for v in rng.integers(1, max_axis + 1, size=3))
        occ = rng.choice(OCC_VALUES, size=shape, p=rng.dirichlet(np.ones(len(OCC_VALUES))))
        pool = np.array(KEY_POOLS[int(rng.integers(len(KEY_POOLS)))], np.uint32)
        keys = rng.choice(pool, size=shape)
    if rng.random() < 0.5:
        return occ, keys, capi.DISPLAY_OCCUPANCY, dict(class_mask=int(rng.integers(8)), surface_only=bool(rng.integers(2)))
    kind = int(rng.integers(4))
    draw = None if kind == 0 else [] if kind == 1 else np.unique(rng.choice(np.concatenate([pool, [4, 2 ** 32 - 3]]).astype(np.uint32),
                                                                                   size=1 if kind == 2 else 4))
    return occ, keys, capi.DISPLAY_KEY_FIELD, dict(draw_keys=draw, draw_zero=bool(rng.integers(2)),
                                                   class_mask=7 if rng.random() < 0.6 else int(rng.integers(8)))


def check_sdf(ctx, d, alpha):
    """the SDF rule and the colour map of one field, host and device forms"""
    want_idx, want_col = R.select_sdf(d)[0], R.sdf_colors(d, alpha)
    assert np.array_equal(ctx.display_select_sdf(d), want_idx), "sdfgpu_display_select_sdf"
    got = ctx.display_sdf_colors(d, alpha)
    assert H.same_or_nan(got, want_col), "sdfgpu_display_sdf_colors"
    d_sdf = dev(d)
    total = ctx.display_select_sdf_device(d_sdf.data_ptr(), d.shape)
    buf, col = words(total), words(d.size * 4)
    assert ctx.display_select_sdf_device(d_sdf.data_ptr(), d.shape, buf.data_ptr(), total) == total == len(want_idx)
    ctx.display_sdf_colors_device(d_sdf.data_ptr(), d.shape, alpha, col.data_ptr())
    assert np.array_equal(host_words(buf, total), want_idx), "sdfgpu_display_select_sdf_device"
    assert H.same_or_nan(host_words(col, d.size * 4).view(np.float32).reshape(want_col.shape), want_col), "sdfgpu_display_sdf_colors_device"


def fuzz(ctx, cases, seed):
    """`cases` seeded random cases, each through one stride, one form and both result forms; every fourth also builds the SDF of its
    scene (and every eighth plants special values in it) and runs the SDF rule and the colour map on it"""
    master = np.random.default_rng(seed)
    for case in range(cases):
        s = int(master.integers(1 << 31))
        rng = np.random.default_rng(s)
        occ, keys, rule, opts = random_case(rng)
        try:
            check(ctx, occ, keys, rule, strides=(8 if case % 2 else 16,), forms=("host" if case % 4 == 0 else "device",), **opts)
            if case % 4 == 1:
                with np.errstate(invalid="ignore"):
                    d, _ = ctx.build((occ > 0.5).astype(np.uint8), 0.1)
                if case % 8 == 1:
                    d = d.copy()
                    where = rng.random(d.shape) < 0.05
                    d[where] = rng.choice(np.array([0.0, -0.0, np.nan, np.inf, -np.inf], np.float32), size=int(where.sum()))
                check_sdf(ctx, d, float(rng.choice([0.5, -1.0, 3.0, 0.01])))
        except Exception as e:                                  # noqa: BLE001
            raise AssertionError("fuzz case %d (seed %d, shape %s, rule %d, %s): %s" % (case, s, occ.shape, rule, opts, e))
