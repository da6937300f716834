"""The contract of removal from the dynamic spatial hashed map (include/sdfgpu.h "Removal") restated in Python
as plain functions on a dsh_restated.Map: removals one operation at a time in list order, and the box test on every chunk's cell
range with Python ints (no chunk-range shortcut, so it is a statement of its own).  Nothing here runs on a GPU."""
import numpy as np

import dsh_restated as R

CHUNK_NOT_REMOVED, CHUNK_REMOVED = 0, 1
MAX_BOX_CELL = 1 << 40


class Refused(ValueError):
    """what SDFGPU_ERR_INVALID_ARGUMENT stands for"""


def remove_chunk(m, p):
    i = m.global_cell(p)
    if i is None:
        return CHUNK_NOT_REMOVED
    c = m.split(i)[0]
    if c not in m.chunks:
        return CHUNK_NOT_REMOVED
    del m.chunks[c]
    m.components_valid = False
    return CHUNK_REMOVED


def remove_chunks(m, locations):
    loc = np.asarray(locations, np.float64).reshape(-1, 3)
    return np.array([remove_chunk(m, p) for p in loc], np.uint8)


def box_ok(lower, extent):
    return all(abs(int(l)) <= MAX_BOX_CELL and 0 <= int(e) <= MAX_BOX_CELL for l, e in zip(lower, extent))


def chunk_holds_a_cell_of(m, c, lower, extent):
    """whether the chunk's cells c n .. c n + n - 1 and the box's cells lower .. lower + extent - 1 share a cell on every axis"""
    for a in range(3):
        first, last = c[a] * m.n[a], c[a] * m.n[a] + m.n[a] - 1
        box_first, box_last = int(lower[a]), int(lower[a]) + int(extent[a]) - 1          # (an extent of 0: last < first, no cell)
        if box_last < box_first or last < box_first or first > box_last:
            return False
    return True


def retain_box(m, lower, extent, invert=False):
    """removes the chunks that hold no cell of the box (invert: those that hold at least one); returns how many"""
    if not box_ok(lower, extent):
        raise Refused("box out of range")
    gone = [c for c in m.chunks if chunk_holds_a_cell_of(m, c, lower, extent) == bool(invert)]
    for c in gone:
        del m.chunks[c]
    if gone:
        m.components_valid = False
    return len(gone)


def shrink_plan(live, spare, capacity_chunks, table_capacity, cells_per_chunk):
    """(capacity_chunks, table_capacity, bytes_held) after shrink"""
    pool = min(capacity_chunks, max(live + spare, 1))
    want = 16
    while want < 2 * (live + spare):
        want *= 2
    table = min(table_capacity, want)
    return pool, table, table * 12 + pool * (24 + 8 * cells_per_chunk)
