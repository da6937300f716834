"""The object contours (include/sdfgpu.h "Display export: contours") restated in numpy, three ways:

  literal()        the reference's recipe (tagged_object_collision_map.cpp:917-1180): per object o an exact squared distance D, by brute
                   force over all pairs of cells, from every cell that is filled for o to the nearest cell that is not; the field
                   -float32(sqrt(float64(D)) * res) of tests/resolution_domain.py::finish; drawn iff `dist < 0.0 && dist > bdy` with
                   bdy = float32(-1.9 * res)
  reach(res)       the largest D in {1, 2, 3} that those comparisons admit at this resolution, else 0
  by_neighbours()  the device rule: a cell filled for its own key is drawn iff some in-bounds cell of the 26 around it is not filled
                   for that key at a squared offset <= reach

Filled for o: key == o and (occ > 0.5 or (unknown_is_filled and occ == 0.5)); NaN never.  Cells outside the grid do not exist.
tests/test_contour_cpu.py proves literal == by_neighbours(reach(res)); tests/test_gpu_contour.py holds the GPU to by_neighbours."""
import numpy as np

import resolution_domain as RD

BIG = np.iinfo(np.int64).max


def filled_cells(occ, unknown_is_filled=True):
    occ = np.asarray(occ, np.float32)
    with np.errstate(invalid="ignore"):
        f = occ > np.float32(0.5)
        if unknown_is_filled:
            f |= occ == np.float32(0.5)
    return f


def listed(keys, draw_keys=None, draw_zero=False):
    keys = np.ascontiguousarray(keys, np.uint32)
    ok = np.ones(keys.shape, bool)
    if draw_keys is not None:
        ok &= np.isin(keys, np.asarray(draw_keys, np.uint32))
    if not draw_zero:
        ok &= keys != 0
    return ok


def object_dsq(mask):
    """int64 [shape]: -D at the cells of `mask` (D = exact squared distance in cells to the nearest cell outside it, INT64_MAX when
    there is none), +1 elsewhere (those cells are never drawn: their distance is positive).  All pairs: small grids only."""
    mask = np.asarray(mask, bool)
    assert mask.size <= 4096
    pts = np.stack(np.meshgrid(*[np.arange(s) for s in mask.shape], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    inside = mask.reshape(-1)
    out = np.ones(mask.size, np.int64)
    if inside.any():
        if (~inside).any():
            d = ((pts[inside][:, None, :] - pts[~inside][None, :, :]) ** 2).sum(axis=2).min(axis=1)
        else:
            d = np.full(int(inside.sum()), BIG, np.int64)
        out[inside] = -d
    return out.reshape(mask.shape)


def literal(occ, keys, res, unknown_is_filled=True, draw_keys=None, draw_zero=False):
    """-> (indices uint32 ascending, keys uint32): the reference's loop, one field per object that has an SDF"""
    keys = np.ascontiguousarray(keys, np.uint32)
    filled = filled_cells(occ, unknown_is_filled)
    drawn = np.zeros(keys.shape, bool)
    with np.errstate(over="ignore", under="ignore"):
        bdy = np.float32(-1.9 * res)
    objects = np.unique(keys[listed(keys, draw_keys, draw_zero)])
    for o in objects:
        dist = RD.finish(object_dsq(filled & (keys == o)), res)
        with np.errstate(invalid="ignore"):
            drawn |= (keys == o) & (dist.astype(np.float64) < 0.0) & (dist > bdy)
    idx = np.flatnonzero(drawn.reshape(-1)).astype(np.uint32)
    return idx, keys.reshape(-1)[idx]


def f(D, res):
    """the magnitude of the finished field at squared distance D: float32(sqrt(float64(D)) * res)"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return (np.sqrt(np.float64(D)) * np.float64(res)).astype(np.float32)


def admits(D, res):
    """the reference's comparisons on a filled cell at squared distance D"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        bdy = np.float32(np.float64(-1.9) * np.float64(res))
        dist = -f(D, res)
        return bool(np.float64(dist) < 0.0 and dist > bdy)


def reach(res):
    r = 0
    for D in (1, 2, 3):
        if admits(D, res):
            r = D
    return r


def by_neighbours(occ, keys, reach, unknown_is_filled=True, draw_keys=None, draw_zero=False):
    """-> (indices uint32 ascending, keys uint32): the device rule"""
    keys = np.ascontiguousarray(keys, np.uint32)
    nx, ny, nz = keys.shape
    filled = filled_cells(occ, unknown_is_filled)
    pk = np.zeros((nx + 2, ny + 2, nz + 2), np.uint32)
    pf = np.zeros((nx + 2, ny + 2, nz + 2), bool)
    inb = np.zeros((nx + 2, ny + 2, nz + 2), bool)
    pk[1:-1, 1:-1, 1:-1] = keys
    pf[1:-1, 1:-1, 1:-1] = filled
    inb[1:-1, 1:-1, 1:-1] = True
    foreign = np.zeros(keys.shape, bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                d2 = dx * dx + dy * dy + dz * dz
                if d2 == 0 or d2 > reach:
                    continue
                s = (slice(1 + dx, 1 + dx + nx), slice(1 + dy, 1 + dy + ny), slice(1 + dz, 1 + dz + nz))
                foreign |= inb[s] & ~(pf[s] & (pk[s] == keys))
    drawn = filled & listed(keys, draw_keys, draw_zero) & foreign
    idx = np.flatnonzero(drawn.reshape(-1)).astype(np.uint32)
    return idx, keys.reshape(-1)[idx]


# the reach table of DESIGN.md section 25
REACH_TABLE = [(1.0 / 3.0, 3), (0.037, 3), (2.0 ** -3, 3), (2.0 ** -140, 3), (2.0 ** -128 * (1.0 + 2.0 ** -30), 3), (2.0 ** 125, 3), (2.0 ** 127, 3),
               (2.0 ** -149, 2), (1.2 * 2.0 ** 127, 2), (1.5 * 2.0 ** 127, 1), (2.0 ** -160, 0), (1.2 * 2.0 ** -150, 0), (2.0 ** 128, 0), (1e308, 0)]


# ---- the closed-form scene of the large cases: solid boxes on a lattice ------------------------------------------------------------
def lattice_box_axis(n, period, size):
    """per axis index: (inside a box?, the box's number along the axis, on the box's first or last plane?)"""
    i = np.arange(n, dtype=np.int64)
    r = i % period
    return r < size, i // period, (r == 0) | (r == size - 1)


def lattice_scene(shape, period, size):
    """(occ float32, keys uint32): boxes of size^3 cells, one per period^3 cell of a lattice (clipped by the grid's far faces), each
    with its own id 1 + its lattice number; free cells carry id 0 and occupancy 0"""
    ax = [lattice_box_axis(n, period, size) for n in shape]
    counts = [int(-(-n // period)) for n in shape]
    inside = ax[0][0][:, None, None] & ax[1][0][None, :, None] & ax[2][0][None, None, :]
    number = (ax[0][1][:, None, None] * counts[1] + ax[1][1][None, :, None]) * counts[2] + ax[2][1][None, None, :]
    return np.where(inside, np.float32(1.0), np.float32(0.0)).astype(np.float32), np.where(inside, number + 1, 0).astype(np.uint32)


def lattice_contour_count(shape, period, size):
    """the number of drawn cells at reach >= 1 with size <= period - 1 (every box has free cells all around it, or the grid's face):
    a cell of a box is drawn iff along some axis it has an in-grid neighbour outside the box.  Per axis the box cells split into
    `edge` cells (with such a neighbour) and `core` cells; the drawn cells are all box cells minus the all-core ones."""
    assert 1 <= size <= period - 1
    total_cells, total_core = 1, 1
    for n in shape:
        i = np.arange(n, dtype=np.int64)
        r = i % period
        inside = r < size
        # the neighbour below is outside the box iff r == 0 and i > 0; the one above iff r == size - 1 and i + 1 < n
        edge = inside & (((r == 0) & (i > 0)) | ((r == size - 1) & (i + 1 < n)))
        total_cells *= int(inside.sum())
        total_core *= int((inside & ~edge).sum())
    return total_cells - total_core


def lattice_drawn(shape, period, size, index):
    """the closed form at single cells: is the cell at scan index `index` drawn at reach >= 1?  `index`: an int64 numpy array or
    torch tensor (only operators that both have are used)"""
    nx, ny, nz = shape
    coords = (index // (ny * nz), (index // nz) % ny, index % nz)
    inside = index >= 0
    edge = index < 0
    for i, n in zip(coords, shape):
        r = i % period
        inside = inside & (r < size)
        edge = edge | ((r == 0) & (i > 0)) | ((r == size - 1) & (i + 1 < n))
    return inside & edge


def lattice_key(shape, period, index):
    """the id of the box that holds the cell at scan index `index` (a cell of a box): 1 + its lattice number; numpy or torch int64"""
    nx, ny, nz = shape
    cy, cz = -(-ny // period), -(-nz // period)
    return ((index // (ny * nz) // period) * cy + ((index // nz) % ny) // period) * cz + (index % nz) // period + 1
