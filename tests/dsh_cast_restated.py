"""The contract of a ray cast (include/sdfgpu.h "Ray casts") restated in Python on dsh_rays_restated.steps and a
dsh_restated.Map: one ray at a time, the walk in Python floats and ints, the predicate in numpy float32.  It is the judge of
tests/test_gpu_dsh_cast*.py; nothing here runs on a GPU.

The contract is this project's own: UNVERIFIED against octomap's castRay."""
import struct

import numpy as np

import dsh_rays_restated as RR

CAST_SKIPPED, CAST_CLEAR, CAST_CLEAR_IN_RANGE, CAST_BLOCKED = 0, 1, 2, 3
SKIP_FIRST, SKIP_LAST, UNKNOWN_IS_FILLED = 1, 2, 4
HIT_DTYPE = np.dtype([("cell", np.int64, (3,)), ("record", np.uint64), ("t", np.float64), ("step", np.uint32), ("found", np.uint32)])
Refused = RR.Refused


def blocks(record, unknown_is_filled):
    """the window predicate on one record: the low 4 bytes as a float; a NaN fails both comparisons"""
    occ = struct.unpack("<f", struct.pack("<I", int(record) & 0xFFFFFFFF))[0]   # (a float32 widens to a Python float exactly)
    return occ > 0.5 or (bool(unknown_is_filled) and occ == 0.5)


def check_call(m, max_range, flags, outputs=True):
    if int(flags) & ~(SKIP_FIRST | SKIP_LAST | UNKNOWN_IS_FILLED):
        raise Refused("flags 0x%x" % int(flags))
    if not outputs:
        raise Refused("no output")
    return RR.range_in_cells(m, max_range)


def trace(m, gs, ge, range_cells, i0=None, i1=None):
    """(is_long, N, W): W is the walk's cells (all of them, or the in-range prefix of a long ray) as (cell, record, t_k, k, found)"""
    len2, r2 = RR.length2(gs, ge), range_cells * range_cells
    is_long = len2 > r2
    i0 = [int(np.floor(v)) for v in gs] if i0 is None else i0
    i1 = [int(np.floor(v)) for v in ge] if i1 is None else i1
    cells = []
    for k, (c, tk) in enumerate(RR.steps(gs, ge, i0, i1)):
        if is_long and not (tk * tk) * len2 <= r2:                             # (the in-range cells are a prefix that always holds c_0)
            break
        record, found = m.get_cell(c)
        cells.append((c, record, tk, k, found))
    return is_long, sum(abs(i1[a] - i0[a]) for a in range(3)), cells


def decide(traced, flags):
    """(status, the described cell) of a traced ray under the flags"""
    is_long, n_steps, cells = traced
    for described in cells:
        k = described[3]
        tested = not (k == 0 and flags & SKIP_FIRST) and not (k == n_steps and flags & SKIP_LAST)
        if tested and blocks(described[1], flags & UNKNOWN_IS_FILLED):
            return CAST_BLOCKED, described
    return (CAST_CLEAR_IN_RANGE if is_long else CAST_CLEAR), cells[-1]


def cast(m, gs, ge, range_cells, flags, i0=None, i1=None):
    """(status, (cell, record, t, step, found)) of one ray between two valid locations given in grid coordinates"""
    return decide(trace(m, gs, ge, range_cells, i0, i1), int(flags))


def _result(n):
    return np.zeros(n, np.uint8), np.zeros(n, HIT_DTYPE)


def _store(hits, k, described):
    c, record, t, step, found = described
    hits[k]["cell"] = c
    hits[k]["record"] = np.uint64(record)
    hits[k]["t"] = t
    hits[k]["step"] = step
    hits[k]["found"] = found


def trace_rays(m, sensor, points, max_range):
    """one trace per ray sensor -> point (float32 [n, 3], widened to double), None for a skipped ray"""
    r = RR.range_in_cells(m, max_range)
    s = RR.grid_coordinates(m, sensor)
    if s is None:
        raise Refused("the sensor is not a valid location")
    ends = [RR.grid_coordinates(m, p) for p in np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)]
    return [None if e is None else trace(m, s[0], e[0], r, s[1], e[1]) for e in ends]


def trace_segments(m, starts, ends, max_range):
    """one trace per segment start -> end (float64 [n, 3] each); an invalid start skips its ray only"""
    r = RR.range_in_cells(m, max_range)
    a = np.asarray(starts, np.float64).reshape(-1, 3)
    b = np.asarray(ends, np.float64).reshape(-1, 3)
    assert len(a) == len(b)
    both = [(RR.grid_coordinates(m, p), RR.grid_coordinates(m, q)) for p, q in zip(a, b)]
    return [None if s is None or e is None else trace(m, s[0], e[0], r, s[1], e[1]) for s, e in both]


def decide_all(traces, flags):
    """(statuses uint8 [n], hits HIT_DTYPE [n]) of traced rays under the flags"""
    statuses, hits = _result(len(traces))
    for k, traced in enumerate(traces):
        if traced is not None:
            statuses[k], described = decide(traced, int(flags))
            _store(hits, k, described)
    return statuses, hits


def cast_rays(m, sensor, points, max_range, flags=0):
    check_call(m, max_range, flags)
    return decide_all(trace_rays(m, sensor, points, max_range), flags)


def cast_segments(m, starts, ends, max_range, flags=0):
    check_call(m, max_range, flags)
    return decide_all(trace_segments(m, starts, ends, max_range), flags)


def distance(start, end, t):
    """the wrappers' world distance: t * sqrt((dx dx + dy dy) + dz dz) of end - start, in double"""
    d = [float(np.float64(end[a]) - np.float64(start[a])) for a in range(3)]
    return float(t) * float(np.sqrt(np.float64((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))
