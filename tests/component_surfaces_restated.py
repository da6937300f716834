"""Restatement of the component-surface contract (include/sdfgpu.h "Component surfaces") in numpy: the oracle of
test_component_surfaces_cpu.py and test_gpu_component_surfaces.py.

A voxel of label c is a surface voxel iff one of its six face neighbours has another label, out-of-grid voxels being
component -1; it is reported iff it is also selected.  The result is the per-label counts and the reported linear indices
((x ny + y) nz + z) grouped by ascending label, ascending inside each group."""
import numpy as np

FILLED, EMPTY, UNKNOWN = 1, 2, 4


def surface_mask(labels):
    """bool [nx, ny, nz]: some face neighbour (or the outside, -1) has another label."""
    lab = np.asarray(labels).astype(np.int64)
    pad = np.pad(lab, 1, constant_values=-1)
    core = pad[1:-1, 1:-1, 1:-1]
    surf = np.zeros(lab.shape, bool)
    for axis in range(3):
        for shift in (-1, 1):
            surf |= np.roll(pad, shift, axis)[1:-1, 1:-1, 1:-1] != core
    return surf


def class_select(occupancy, class_mask):
    """bool: the voxel's occupancy class (FILLED > 0.5, EMPTY < 0.5, UNKNOWN the rest, NaN included) is in class_mask."""
    occ = np.asarray(occupancy, np.float32)
    with np.errstate(invalid="ignore"):
        cls = np.where(occ > np.float32(0.5), FILLED, np.where(occ < np.float32(0.5), EMPTY, UNKNOWN))
    return (cls & int(class_mask)) != 0


def restated_surfaces(labels, select=None, max_label=None):
    """-> (counts int64 [max_label + 1], indices uint32 [total], reported bool [nx, ny, nz])."""
    lab = np.asarray(labels)
    if max_label is None:
        max_label = int(lab.max()) if lab.size else 0
    rep = surface_mask(lab)
    if select is not None:
        rep &= np.asarray(select) != 0
    idx = np.flatnonzero(rep.reshape(-1))
    key = lab.reshape(-1)[idx].astype(np.int64)
    order = np.argsort(key, kind="stable")
    counts = np.bincount(key, minlength=int(max_label) + 1).astype(np.int64)
    return counts, idx[order].astype(np.uint32), rep


def as_map(counts, indices, shape):
    """{label: set of (x, y, z)}: what ExtractComponentSurfaces returns, as plain Python."""
    ny, nz = int(shape[1]), int(shape[2])
    out, start = {}, 0
    for c, k in enumerate(np.asarray(counts).tolist()):
        if k:
            g = np.asarray(indices[start:start + k]).astype(np.int64)
            out[c] = set(zip((g // (ny * nz)).tolist(), (g // nz % ny).tolist(), (g % nz).tolist()))
        start += k
    return out
