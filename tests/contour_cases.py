"""Helpers of the contour GPU tests (tests/test_gpu_contour.py and its kin): one contour selection through the host and the device
entry points with a sentinel word behind every output, its reference from tests/contour_restated.py::by_neighbours, and the seeded
random cases of the fuzz (which a child process runs under SDFGPU_REDZONE=1, so they live in a module of their own)."""
import numpy as np

import contour_restated as CR
import display_cases as C
import display_restated as R
from sdf_tools_amd import capi

DEFAULTS = dict(unknown_is_filled=True, draw_keys=None, draw_zero=False)
LAYOUTS = [(8, 0, 4), (16, 0, 8), (12, 8, 0)]                  # (stride, occupancy offset, key offset); the last: key ahead of the occupancy


def reference(occ, keys, reach, grouped, **opts):
    o = dict(DEFAULTS, **opts)
    idx, k = CR.by_neighbours(occ, keys, reach, o["unknown_is_filled"], o["draw_keys"], o["draw_zero"])
    return R.grouped(idx, k) if grouped else (idx, k)


def run_host(ctx, cells, shape, reach, layout, grouped, **opts):
    stride, occ_off, key_off = layout
    before = cells.copy()
    got = ctx.display_select_contour(cells, shape, reach, stride, occ_off, key_off, grouped=grouped, **dict(DEFAULTS, **opts))
    assert np.array_equal(cells, before), "the records are read only"
    return got


def run_device(ctx, cells, shape, reach, layout, grouped, stream=0, d_cells=None, **opts):
    """count first, then buffers of exactly the total (and the group count) with a sentinel word behind each"""
    o = dict(DEFAULTS, **opts)
    stride, occ_off, key_off = layout
    if d_cells is None:
        keep = C.dev(cells)
        d_cells = keep.data_ptr()
    call = lambda **kw: ctx.display_select_contour_device(d_cells, shape, reach, stride, occ_off, key_off, stream=stream, **dict(o, **kw))
    total, _ = call()
    idx, keys = C.words(total), C.words(total)
    if not grouped:
        t, _ = call(d_indices=idx.data_ptr(), d_keys=keys.data_ptr(), capacity=total)
        assert t == total
        return C.host_words(idx, total), C.host_words(keys, total)
    try:                                                        # group capacity 0: the count of groups comes back with the refusal
        call(grouped=True, d_indices=idx.data_ptr(), capacity=total, d_group_keys=C.words(0).data_ptr(), d_group_offsets=C.words(1).data_ptr(),
             group_capacity=0)
        groups = 0
    except capi.SdfGpuError as e:
        assert e.code == -1 and e.total == total and e.groups > 0, str(e)
        groups = e.groups
    idx = C.words(total)
    gk, go = C.words(groups), C.words(groups + 1)
    t, g = call(grouped=True, d_indices=idx.data_ptr(), d_keys=keys.data_ptr(), capacity=total, d_group_keys=gk.data_ptr(),
                d_group_offsets=go.data_ptr(), group_capacity=groups)
    assert (t, g) == (total, groups)
    return C.host_words(idx, total), C.host_words(keys, total), C.host_words(gk, groups), C.host_words(go, groups + 1)


def check(ctx, occ, keys, reach, layouts=LAYOUTS[:2], forms=("host", "device"), groupings=(False, True), **opts):
    """every layout, form and result form of one selection against by_neighbours; returns the scan-order reference"""
    shape = occ.shape
    for grouped in groupings:
        want = reference(occ, keys, reach, grouped, **opts)
        for layout in layouts:
            cells = R.cells_of(occ, keys, layout[0], layout[2], layout[1])
            for form in forms:
                got = (run_host if form == "host" else run_device)(ctx, cells, shape, reach, layout, grouped, **opts)
                C.same("%s form, layout %s, grouped %s, shape %s, reach %d, %s" % (form, layout, grouped, shape, reach, C.describe(opts)), got, want)
    return reference(occ, keys, reach, False, **opts)


def random_case(rng, max_axis=24):
    """-> (occ, keys, reach, opts): voxel noise, mostly-filled noise (interiors beyond the reach), or slabs of ids"""
    shape = tuple(int(v) for v in rng.integers(1, max_axis + 1, size=3))
    if rng.random() < 0.3:
        shape = (shape[0], shape[1], int(rng.choice([1, 2, 5, 63, 64, 65, 128])))      # rows around a wave
    occ = rng.choice(C.OCC_VALUES, size=shape, p=rng.dirichlet(np.ones(len(C.OCC_VALUES))))
    kind = int(rng.integers(3))
    if kind >= 1:
        occ = np.where(rng.random(shape) < 0.92, np.float32(1.0), occ).astype(np.float32)
    pool = np.array(C.KEY_POOLS[int(rng.integers(len(C.KEY_POOLS)))], np.uint32)
    keys = rng.choice(pool, size=shape)
    if kind == 2:
        axis = int(rng.integers(3))
        along = pool[np.arange(shape[axis]) * len(pool) // shape[axis]]
        keys = np.broadcast_to(along.reshape([-1 if a == axis else 1 for a in range(3)]), shape).copy()
    d = int(rng.integers(4))
    draw = None if d == 0 else [] if d == 1 else np.unique(rng.choice(np.concatenate([pool, [4, 2 ** 32 - 3]]).astype(np.uint32), size=1 if d == 2 else 4))
    return occ, keys, int(rng.integers(4)), dict(unknown_is_filled=bool(rng.integers(2)), draw_keys=draw, draw_zero=bool(rng.integers(2)))


def fuzz(ctx, cases, seed):
    master = np.random.default_rng(seed)
    for case in range(cases):
        s = int(master.integers(1 << 31))
        rng = np.random.default_rng(s)
        occ, keys, reach, opts = random_case(rng)
        try:
            check(ctx, occ, keys, reach, layouts=(LAYOUTS[case % 3],), forms=("host" if case % 4 == 0 else "device",), **opts)
        except Exception as e:                                  # noqa: BLE001
            raise AssertionError("fuzz case %d (seed %d, shape %s, reach %d, %s): %s" % (case, s, occ.shape, reach, opts, e))
