"""The contract of a fused frame of sensor rays (include/sdfgpu.h "Sensor rays: fusion") restated in Python: the
rays are dsh_rays_restated.frame() unchanged, the sets H (hit cells) and M (carved by at least one ray, not hit) are Python sets of
global cell indices, and fuse() is numpy float32 scalars, one rounding per operation.  Applied to a dsh_restated.Map.  It is the judge
of tests/test_gpu_dsh_fusion*.py; nothing here runs on a GPU.

The contract is this project's own: UNVERIFIED against octomap's insertPointCloud / updateNode and against arc_utilities."""
import numpy as np

import dsh_rays_restated as RR
from dsh_rays_restated import Refused                                          # noqa: F401  (what a refused frame raises)

DEFAULT_MODEL = (0.7, 0.4, 0.12, 0.97)                                         # prob_hit, prob_miss, clamp_min, clamp_max: octomap's numbers
LOW, HIGH = np.float32(0.001), np.float32(0.999)


def model_of(model=None):
    """the four numbers as float32 scalars; Refused unless all lie in [0.001f, 0.999f] and clamp_min <= clamp_max (NaN fails)"""
    m = tuple(np.float32(v) for v in (DEFAULT_MODEL if model is None else model))
    if len(m) != 4 or not all(v >= LOW and v <= HIGH for v in m) or not m[2] <= m[3]:
        raise Refused("sensor model %r" % (m,))
    return m


def fuse(p, m, clamp_min, clamp_max):
    """one measurement m folded into the occupancy p, all float32 scalars"""
    f = np.float32
    p, m, clamp_min, clamp_max = f(p), f(m), f(clamp_min), f(clamp_max)
    with np.errstate(all="ignore"):
        q = p if p >= clamp_min else clamp_min
        q = q if q <= clamp_max else clamp_max
        a = f(q * m)
        b = f(f(f(1.0) - q) * f(f(1.0) - m))
        r = f(a / f(a + b))
        r = r if r >= clamp_min else clamp_min
        r = r if r <= clamp_max else clamp_max
    return f(r)


def fuse_record(record, m, clamp_min, clamp_max):
    """the 8-byte record with its occupancy word (the low one) updated and its component word kept"""
    record = int(record)
    p = np.array([record & 0xFFFFFFFF], np.uint32).view(np.float32)[0]
    r = np.array([fuse(p, m, clamp_min, clamp_max)], np.float32).view(np.uint32)[0]
    return (record & ~0xFFFFFFFF) | int(r)


def get_index(m, i):
    """Get at a global cell index: the record before the frame"""
    c, l = m.split(i)
    kind, what = m.chunks.get(c, ("chunk", m.default))
    return int(what) if kind == "chunk" else int(what[l])


def sets_of(carved, hits):
    """(H, M) of a frame"""
    H = {h for h in hits if h is not None}
    M = {c for cells in carved for c in cells} - H
    return H, M


def fuse_rays(m, sensor, points, max_range, model=None):
    """The frame applied to the map: every cell of H and of M updated once.  Returns (statuses, counts); raises Refused."""
    prob_hit, prob_miss, clamp_min, clamp_max = model_of(model)
    statuses, carved, hits = RR.frame(m, sensor, points, max_range)
    H, M = sets_of(carved, hits)
    new_chunks = 0
    for cells, meas in ((sorted(H), prob_hit), (sorted(M), prob_miss)):
        for c in cells:
            new_chunks += RR.set_cell_index(m, c, fuse_record(get_index(m, c), meas, clamp_min, clamp_max))
    counts = {"rays_hit": int((statuses == RR.RAY_HIT).sum()), "rays_truncated": int((statuses == RR.RAY_TRUNCATED).sum()),
              "rays_skipped": int((statuses == RR.RAY_SKIPPED).sum()), "cells_carved": sum(len(c) for c in carved), "new_chunks": new_chunks}
    return statuses, counts
