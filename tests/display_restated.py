"""The display export restated in numpy, from the rules of include/sdfgpu.h "Display export"  -- the
reference for tests/test_display_cpu.py (which checks it against a triple loop) and tests/test_gpu_display.py.

Rules, per voxel in scan order (x -> y -> z, z fastest): drawn? and a uint32 key.
  occupancy   class F occ > 0.5, E occ < 0.5, U occ == 0.5, N (NaN) none of them; key 0 / 1 / 2 / 2; drawn iff bit `key` of class_mask
              and, with surface_only, some in-bounds cell of the 26 around it is in the set its class asks for
              (E: F or U; F: E or U; U: F, E or N; N: nothing)
  key field   key = the record's uint32; drawn iff (draw_keys is None or holds it) and (draw_zero or key != 0) and the class bit
  sdf         drawn iff d <= 0 (NaN is not); key 0
Results: scan order (indices ascending, keys beside them); grouped (the same pairs by (key, index), group keys, group offsets);
points cell * (i + 0.5); table colours; the SDF colour map in float64 with the product and the sum rounded separately.
cells_of builds the records of a layout (stride, occupancy offset, key offset); filler_words fills their other words with values that
would change an answer if read by mistake (tests/test_gpu_display_layouts.py pins both against records built by hand)."""
import numpy as np

F, E, U, N = 0, 1, 2, 3
WANTS = {E: (F, U), F: (E, U), U: (F, E, N), N: ()}


def occ_class(occ):
    """class per voxel (uint8): the literal comparisons on the float32"""
    occ = np.asarray(occ, np.float32)
    half = np.float32(0.5)
    cls = np.full(occ.shape, N, np.uint8)
    cls[occ == half] = U
    cls[occ < half] = E
    cls[occ > half] = F
    return cls


def class_key(cls):
    return np.minimum(cls, 2).astype(np.uint32)


def _neighbour_has(cls, which):
    """[nx, ny, nz] bool: some in-bounds cell of the 3 x 3 x 3 block around the voxel (the voxel included) has class `which`"""
    nx, ny, nz = cls.shape
    pad = np.zeros((nx + 2, ny + 2, nz + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = cls == which
    out = np.zeros(cls.shape, bool)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                out |= pad[dx:dx + nx, dy:dy + ny, dz:dz + nz]
    return out


def occ_surface(occ):
    """the 26-neighbour rule (no class asks for itself, so the voxel may stay in the block)"""
    cls = occ_class(occ)
    has = {c: _neighbour_has(cls, c) for c in (F, E, U, N)}
    out = np.zeros(cls.shape, bool)
    for c, wanted in WANTS.items():
        for w in wanted:
            out |= (cls == c) & has[w]
    return out


def _scan(drawn, key):
    idx = np.flatnonzero(drawn.reshape(-1)).astype(np.uint32)
    return idx, np.ascontiguousarray(key, np.uint32).reshape(-1)[idx]


def select_occupancy(occ, class_mask=7, surface_only=False):
    """-> (indices uint32 ascending, keys uint32)"""
    cls = occ_class(occ)
    key = class_key(cls)
    drawn = ((int(class_mask) >> key) & 1).astype(bool)
    if surface_only:
        drawn &= occ_surface(occ)
    return _scan(drawn, key)


def select_key_field(keys, occ=None, draw_keys=None, draw_zero=True, class_mask=7):
    key = np.ascontiguousarray(keys, np.uint32)
    drawn = np.ones(key.shape, bool)
    if draw_keys is not None:
        drawn &= np.isin(key, np.asarray(draw_keys, np.uint32))
    if not draw_zero:
        drawn &= key != 0
    if int(class_mask) != 7:
        drawn &= ((int(class_mask) >> class_key(occ_class(occ))) & 1).astype(bool)
    return _scan(drawn, key)


def select_sdf(sdf):
    d = np.asarray(sdf, np.float32)
    with np.errstate(invalid="ignore"):
        drawn = d <= np.float32(0.0)
    return _scan(drawn, np.zeros(d.shape, np.uint32))


def grouped(idx, keys):
    """scan-order pairs -> (indices, keys, group_keys, group_offsets): stably by (key, index)"""
    order = np.argsort(keys, kind="stable")                     # (the indices already ascend)
    gi, gk = idx[order], keys[order]
    if len(gk) == 0:
        return gi, gk, np.zeros(0, np.uint32), np.zeros(1, np.uint32)
    starts = np.flatnonzero(np.concatenate([[True], gk[1:] != gk[:-1]]))
    return gi, gk, gk[starts].astype(np.uint32), np.concatenate([starts, [len(gk)]]).astype(np.uint32)


def points(idx, shape, cell_sizes):
    """float64 [n, 3]: cell * (i + 0.5) per axis, one rounding"""
    nx, ny, nz = shape
    i = np.asarray(idx, np.int64)
    xyz = np.stack([i // (ny * nz), (i // nz) % ny, i % nz], axis=1).astype(np.float64)
    return np.asarray(cell_sizes, np.float64)[None, :] * (xyz + 0.5)


def table_colors(keys, table, default):
    """float32 [n, 4]: table[key], or `default` for keys at or past the table's end"""
    table = np.asarray(table, np.float32).reshape(-1, 4)
    k = np.asarray(keys, np.int64)
    out = np.tile(np.asarray(default, np.float32).reshape(1, 4), (len(k), 1))
    inside = k < len(table)
    out[inside] = table[k[inside]]
    return out


def sdf_extrema(sdf):
    """(min_distance, max_distance): doubles from 0.0, moved by d < min / d > max (NaN moves neither)"""
    d = np.asarray(sdf, np.float32).astype(np.float64).reshape(-1)
    d = d[~np.isnan(d)]
    return (min(0.0, float(d.min())) if d.size else 0.0), (max(0.0, float(d.max())) if d.size else 0.0)


def sdf_colors(sdf, alpha):
    """float32 [..., 4] rgba; float64 arithmetic, the product and the sum rounded separately (numpy never fuses them)"""
    d = np.asarray(sdf, np.float32)
    d64 = d.astype(np.float64)
    mn, mx = sdf_extrema(d)
    out = np.zeros(d.shape + (4,), np.float32)
    out[..., 3] = np.float32(min(max(np.float32(alpha), np.float32(0.0)), np.float32(1.0)))
    with np.errstate(invalid="ignore", divide="ignore"):
        pos, neg = d > 0, d < 0
        g = np.abs(d64[pos] / mx) * 0.8
        out[..., 1][pos] = (g + 0.2).astype(np.float32)
        r = np.abs(d64[neg] / mn) * 0.8
        out[..., 0][neg] = (r + 0.2).astype(np.float32)
    out[..., 2][~(pos | neg)] = 1.0
    return out


FILLER_WORD = 0x7B7B7B7B


def cells_of(occ, key, stride, key_offset=4, occupancy_offset=0, filler=None):
    """records of `stride` bytes: occupancy at occupancy_offset, the key word at key_offset, the other words from `filler` (uint32,
    broadcast to [..., stride / 4]; a fixed pattern without one).  With both fields at one offset the key is stored last."""
    occ = np.asarray(occ, np.float32)
    words = stride // 4
    assert stride == words * 4 and 0 <= occupancy_offset < stride and 0 <= key_offset < stride and occupancy_offset % 4 == 0 and key_offset % 4 == 0
    c = np.empty(occ.shape + (words,), np.uint32)
    c[...] = FILLER_WORD if filler is None else np.asarray(filler, np.uint32)
    c[..., occupancy_offset // 4] = occ.view(np.uint32)
    c[..., key_offset // 4] = np.asarray(key, np.uint32)
    return np.ascontiguousarray(c)


def filler_words(rng, shape, stride, key_pool):
    """uint32 [shape..., stride / 4] for cells_of: every word drawn from values that would change an answer if a kernel read them for a
    field -- the floats 0.0, 0.5, 1.0 and NaN as bits (one of each occupancy class), the keys of the case's own pool, and the fixed pattern"""
    pool = np.concatenate([np.array([0.0, 0.5, 1.0, np.nan], np.float32).view(np.uint32), np.asarray(key_pool, np.uint32).reshape(-1),
                           np.array([FILLER_WORD], np.uint32)])
    return rng.choice(pool, size=tuple(shape) + (stride // 4,))
