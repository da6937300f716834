"""The contract of a frame of sensor rays (include/sdfgpu.h "Sensor rays") restated in Python: grid coordinates
in numpy float64 with separate products and sums, the walk in IEEE doubles (Python floats: one rounding per operation, nothing fused)
and Python ints, one ray at a time, applied to a dsh_restated.Map through sets of global cell indices.  It is the judge of
tests/test_gpu_dsh_rays*.py; nothing here runs on a GPU.

The contract is this project's own: UNVERIFIED against octomap's insertPointCloud and against arc_utilities."""
import math

import numpy as np

import dsh_restated as R

RAY_SKIPPED, RAY_HIT, RAY_TRUNCATED = 0, 1, 2
MAX_RANGE_CELLS = 65536.0


class Refused(ValueError):
    """the whole call is refused: nothing is written"""


def grid_coordinates(m, p):
    """(g, i): the grid coordinates of a location as three doubles (dsh_locate's expression without the floor) and their floors as
    Python ints; None for a location that is not finite or not valid"""
    p = np.asarray(p, np.float64)
    if not np.all(np.isfinite(p)):
        return None
    g, i = [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            row = m.inverse[a]
            ga = (((row[0] * p[0] + row[1] * p[1]) + row[2] * p[2]) + row[3]) * m.inv_cell
            v = np.floor(ga)
            if not np.isfinite(v) or not R.chunk_in_range(R.floor_div(int(v), m.n[a])):
                return None
            g.append(float(ga))
            i.append(int(v))
    return g, i


def steps(gs, ge, i0=None, i1=None):
    """The walk c_0 .. c_N of the ray gs -> ge (grid coordinates, doubles), one (cell, t_k) at a time: cells are tuples of ints,
    t_0 = 0.0 and t_k is the crossing parameter that step k consumed."""
    i0 = [int(math.floor(v)) for v in gs] if i0 is None else list(i0)
    i1 = [int(math.floor(v)) for v in ge] if i1 is None else list(i1)
    d = [ge[a] - gs[a] for a in range(3)]
    sg = [(i1[a] > i0[a]) - (i1[a] < i0[a]) for a in range(3)]
    rem = [abs(i1[a] - i0[a]) for a in range(3)]
    cur = list(i0)

    def crossing(a):
        if rem[a] == 0:
            return math.inf
        return (float(cur[a] + (1 if sg[a] > 0 else 0)) - gs[a]) / d[a]
    t = [crossing(a) for a in range(3)]
    yield tuple(cur), 0.0
    while rem[0] or rem[1] or rem[2]:
        a, tk = 0, t[0]
        if t[1] < tk:
            a, tk = 1, t[1]
        if t[2] < tk:
            a, tk = 2, t[2]
        cur[a] += sg[a]
        rem[a] -= 1
        t[a] = crossing(a)
        yield tuple(cur), tk


def walk(gs, ge, i0=None, i1=None):
    """the whole walk as a list of (cell, t_k)"""
    return list(steps(gs, ge, i0, i1))


def length2(gs, ge):
    d = [ge[a] - gs[a] for a in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def ray(gs, ge, range_cells, i0=None, i1=None):
    """(status, carved cells in walk order, hit cell or None) of one ray whose ends are valid"""
    len2, r2 = length2(gs, ge), range_cells * range_cells
    if not len2 > r2:
        cells = walk(gs, ge, i0, i1)
        return RAY_HIT, [c for c, _ in cells[:-1]], cells[-1][0]
    carved = []
    for c, tk in steps(gs, ge, i0, i1):                                       # (the in-range cells are a prefix: stop at the first failure)
        if not (tk * tk) * len2 <= r2:
            break
        carved.append(c)
    return RAY_TRUNCATED, carved, None


def range_in_cells(m, max_range):
    with np.errstate(all="ignore"):
        r = float(np.float64(max_range) * m.inv_cell)
    if not (r > 0.0 and r <= MAX_RANGE_CELLS):
        raise Refused("max_range spans %r cells" % r)
    return r


def frame(m, sensor, points, max_range):
    """(statuses uint8 [n], list of carved-cell lists, list of hit cells or None) of a frame, the map untouched"""
    r = range_in_cells(m, max_range)
    s = grid_coordinates(m, sensor)
    if s is None:
        raise Refused("the sensor is not a valid location")
    gs, i0 = s
    pts = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    statuses, carved, hits = np.zeros(len(pts), np.uint8), [], []
    for k, p in enumerate(pts):
        e = grid_coordinates(m, p)
        if e is None:
            carved.append([])
            hits.append(None)
            continue
        statuses[k], c, h = ray(gs, e[0], r, i0, e[1])
        carved.append(c)
        hits.append(h)
    return statuses, carved, hits


def set_cell_index(m, i, value):
    """SetCell at a global cell index (dsh_restated.Map.set_cell behind the location arithmetic); True when the chunk was absent"""
    c, l = m.split(i)
    fresh = c not in m.chunks
    kind, what = m.chunks.get(c, ("chunk", m.default))
    if kind == "chunk":
        what = np.full(m.n, what, np.uint64)
        m.chunks[c] = ("cells", what)
    what[l] = np.uint64(value)
    m.components_valid = False
    return fresh


def insert_rays(m, sensor, points, max_range, free_value, hit_value):
    """The frame applied to the map: every carved cell of every ray, then every hit cell.  Returns (statuses, counts)."""
    statuses, carved, hits = frame(m, sensor, points, max_range)
    new_chunks = 0
    for cells in carved:
        for c in cells:
            new_chunks += set_cell_index(m, c, free_value)
    for h in hits:
        if h is not None:
            new_chunks += set_cell_index(m, h, hit_value)
    counts = {"rays_hit": int((statuses == RAY_HIT).sum()), "rays_truncated": int((statuses == RAY_TRUNCATED).sum()),
              "rays_skipped": int((statuses == RAY_SKIPPED).sum()), "cells_carved": sum(len(c) for c in carved), "new_chunks": new_chunks}
    return statuses, counts
