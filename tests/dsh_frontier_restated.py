"""The contract of the frontier calls (include/sdfgpu.h "Frontier cells" and "Component statistics") restated in
Python, cell by cell on dsh_restated.Map.get_cell with plain loops: no vectorised stencil, so that the numpy route of
tests/test_dsh_frontier_cpu.py is a second, independent one.  It is the judge of tests/test_gpu_dsh_frontier*.py; nothing here
runs on a GPU.

A cell is a frontier cell iff its chunk is live, it is free (occupancy < 0.5f) and at least one of its 6 face neighbours (all 26
under FRONTIER_26) is unknown (occupancy == 0.5f).  Neighbours are read wherever they lie; a NaN is neither free nor unknown."""
import numpy as np

import dsh_restated as R

FRONTIER_26 = 1
HALF = np.float32(0.5)

OFFSETS_6 = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
OFFSETS_26 = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def _occupancy(record):
    return np.array([int(record) & 0xFFFFFFFF], np.uint32).view(np.float32)[0]


def is_free(record):
    return bool(_occupancy(record) < HALF)


def is_unknown(record):
    return bool(_occupancy(record) == HALF)


def offsets(flags):
    assert flags in (0, FRONTIER_26)
    return OFFSETS_26 if flags & FRONTIER_26 else OFFSETS_6


def is_frontier(m, i, flags=0):
    """whether global cell i (three Python ints) of the dsh_restated.Map m is a frontier cell"""
    record, found = m.get_cell(i)
    if found == R.NOT_FOUND or not is_free(record):
        return False
    for d in offsets(flags):
        if is_unknown(m.get_cell((i[0] + d[0], i[1] + d[1], i[2] + d[2]))[0]):
            return True
    return False


def deciding_kinds(m, i, flags=0):
    """For a frontier cell: where its unknown neighbours lie, as a set of 'same' (its own chunk), 'live' (another live chunk) and
    'absent' (an absent or out-of-range chunk).  Empty for a cell that is no frontier cell."""
    kinds = set()
    if not is_frontier(m, i, flags):
        return kinds
    own = m.split(i)[0]
    for d in offsets(flags):
        j = (i[0] + d[0], i[1] + d[1], i[2] + d[2])
        record, found = m.get_cell(j)
        if is_unknown(record):
            kinds.add("absent" if found == R.NOT_FOUND else "same" if m.split(j)[0] == own else "live")
    return kinds


def frontier_cells(m, box=None, flags=0):
    """The frontier cells among the cells of live chunks in box = (lower, extent) (the whole map for None), int64 [total, 3]: chunks
    in ascending (c_x, c_y, c_z) order, cells in ascending cell slot order (l_x n_y + l_y) n_z + l_z inside a chunk."""
    out = []
    for c in sorted(m.chunks):
        # the chunk's cells along each axis, cut to the box
        span = []
        for a in range(3):
            first, last = c[a] * m.n[a], c[a] * m.n[a] + m.n[a] - 1
            if box is not None:
                first, last = max(first, int(box[0][a])), min(last, int(box[0][a]) + int(box[1][a]) - 1)
            span.append(range(first, last + 1))
        for x in span[0]:
            for y in span[1]:
                for z in span[2]:
                    if is_frontier(m, (x, y, z), flags):
                        out.append((x, y, z))
    return np.array(out, np.int64).reshape(-1, 3)


def frontier_window(m, lower, shape, flags=0):
    """bool [nx, ny, nz]: voxel (x, y, z) is set iff global cell lower + (x, y, z) is a frontier cell"""
    out = np.zeros(shape, bool)
    for x in range(shape[0]):
        for y in range(shape[1]):
            for z in range(shape[2]):
                out[x, y, z] = is_frontier(m, (int(lower[0]) + x, int(lower[1]) + y, int(lower[2]) + z), flags)
    return out


def frontier_window_bits(m, lower, shape, flags=0):
    """the same as the bit field of sdfgpu_build_bits_device: uint32 [ceil(n / 32)], bits behind the last voxel 0"""
    return R.pack_bits(frontier_window(m, lower, shape, flags))


def component_stats(bits, labels, shape, label_count=None):
    """bits: bool [nx, ny, nz] (or anything that reshapes to it), labels: uint32 of the same shape -> a list of dicts
    {label, count, sum (x, y, z), lo, hi}, one per label in 1 .. label_count (None: every label) with a set voxel, in ascending label
    order, over the voxels whose bit is set.  Python ints throughout."""
    b = np.asarray(bits, bool).reshape(shape)
    lab = np.asarray(labels).reshape(shape)
    acc = {}
    for x in range(shape[0]):
        for y in range(shape[1]):
            for z in range(shape[2]):
                k = int(lab[x, y, z])
                if not b[x, y, z] or k < 1 or (label_count is not None and k > label_count):
                    continue
                s = acc.setdefault(k, {"label": k, "count": 0, "sum": [0, 0, 0], "lo": [x, y, z], "hi": [x, y, z]})
                s["count"] += 1
                for a, v in enumerate((x, y, z)):
                    s["sum"][a] += v
                    s["lo"][a] = min(s["lo"][a], v)
                    s["hi"][a] = max(s["hi"][a], v)
    return [acc[k] for k in sorted(acc)]


def component_stats_records(stats, dtype):
    """the list of component_stats as records of `dtype` (capi.COMPONENT_STATS_DTYPE), for a byte-for-byte comparison"""
    out = np.zeros(len(stats), dtype)
    for r, s in zip(out, stats):
        r["label"], r["reserved"], r["count"] = s["label"], 0, s["count"]
        r["sum"], r["lo"], r["hi"] = s["sum"], s["lo"], s["hi"]
    return out
