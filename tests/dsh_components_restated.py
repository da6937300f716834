"""The contract of the sparse map's connected components (include/sdfgpu.h "Dynamic spatial hashed map: connected components",
DESIGN.md section 35) restated in Python on the chunk dictionary of dsh_restated.Map: a plain breadth-first search over the nodes
in export order.  It is the judge of tests/test_gpu_dsh_components*.py; nothing here runs on a GPU.

Nodes: every cell of a cell-filled chunk, and every chunk-filled chunk as ONE node; cells of absent chunks are no nodes.  Two nodes
are joined iff they are of the same class and some cell of one is a 6-face neighbour (global cell coordinates) of some cell of the
other.  Classes: filled (occupancy > 0.5f) and everything else; with UNKNOWN_APART filled, free (< 0.5f) and the rest (0.5f, NaN).
Components are numbered 1..K by their first node in export order: chunks in ascending (c_x, c_y, c_z), cells x -> y -> z inside.

The contract is this project's own (the reference has no such method on this class): UNVERIFIED against it."""
from collections import deque

import numpy as np

import dsh_restated as R

UNKNOWN_APART = 1
HALF = np.float32(0.5)
MAX_NODES = (1 << 32) - 1          # N must be below this


def classes(records, flags=0):
    """class codes of records: 1 filled, 0 free (everything else without UNKNOWN_APART), 2 unknown or NaN (UNKNOWN_APART only)"""
    assert flags in (0, UNKNOWN_APART)
    occ = R.occupancy(np.asarray(records, np.uint64).reshape(-1))
    with np.errstate(invalid="ignore"):
        filled, free = occ > HALF, occ < HALF
    if flags & UNKNOWN_APART:
        return np.where(filled, 1, np.where(free, 0, 2)).astype(np.int8)
    return filled.astype(np.int8)


def node_bases(m):
    """(chunks in export order, {chunk: node base}, N)"""
    order, bases, n = sorted(m.chunks), {}, 0
    cpc = int(np.prod(m.n))
    for c in order:
        bases[c] = n
        n += cpc if m.chunks[c][0] == "cells" else 1
    return order, bases, n


def _face_slots(n, axis, high):
    """the cell slots of a chunk's low or high face along `axis`, ascending"""
    idx = np.arange(int(np.prod(n))).reshape(n)
    return idx.take(n[axis] - 1 if high else 0, axis=axis).reshape(-1).tolist()


def components(m, flags=0):
    """(K, labels uint32 [N] by node index, (order, bases, N)): the breadth-first search, one node at a time"""
    order, bases, total = node_bases(m)
    assert total < MAX_NODES
    nx, ny, nz = m.n
    strides = (ny * nz, nz, 1)
    cls = [0] * total                       # class per node
    owner = [0] * total                     # index into `order` of the node's chunk
    has_cells = []
    for ci, c in enumerate(order):
        kind, what = m.chunks[c]
        b = bases[c]
        has_cells.append(kind == "cells")
        if kind == "cells":
            codes = classes(what, flags).tolist()
            cls[b:b + len(codes)] = codes
            owner[b:b + len(codes)] = [ci] * len(codes)
        else:
            cls[b] = int(classes([what], flags)[0])
            owner[b] = ci
    index = {c: ci for ci, c in enumerate(order)}
    # the chunk beyond each of a chunk's six faces: (axis, direction) -> index into `order`, or -1 for an absent one
    beyond = []
    for c in order:
        row = []
        for a in range(3):
            for d in (-1, 1):
                o = list(c)
                o[a] += d
                row.append(index.get(tuple(o), -1) if R.chunk_in_range(o[a]) else -1)
        beyond.append(row)
    faces = {(a, high): _face_slots(m.n, a, high) for a in range(3) for high in (False, True)}
    base_of = [bases[c] for c in order]

    def around_chunk(ci):
        """a chunk-filled chunk's neighbours: every node of the six chunks around it that touches it"""
        out = []
        for a in range(3):
            for d in (0, 1):
                oi = beyond[ci][2 * a + d]
                if oi < 0:
                    continue
                if not has_cells[oi]:
                    out.append(base_of[oi])
                else:                                               # the chunk below shows its high face, the one above its low face
                    out.extend(base_of[oi] + k for k in faces[(a, d == 0)])
        return out

    sx, sy = strides[0], strides[1]
    span = ((nx - 1) * sx, (ny - 1) * sy, nz - 1)                   # from a chunk's low face to its high face along each axis
    labels = [0] * total
    count = 0
    for start in range(total):
        if labels[start]:
            continue
        count += 1
        labels[start] = count
        c0 = cls[start]
        queue = deque([start])
        while queue:
            v = queue.popleft()
            ci = owner[v]
            if not has_cells[ci]:
                near = around_chunk(ci)
            else:
                k = v - base_of[ci]
                lx, r = divmod(k, sx)
                ly, lz = divmod(r, nz)
                row = beyond[ci]
                near = []
                # the six face neighbours: inside the chunk, or the cell across the face (a chunk-filled chunk: its one node)
                for inside, step, oi, across in ((lx > 0, -sx, row[0], span[0]), (lx < nx - 1, sx, row[1], -span[0]),
                                                 (ly > 0, -sy, row[2], span[1]), (ly < ny - 1, sy, row[3], -span[1]),
                                                 (lz > 0, -1, row[4], span[2]), (lz < nz - 1, 1, row[5], -span[2])):
                    if inside:
                        near.append(v + step)
                    elif oi >= 0:
                        near.append(base_of[oi] + k + across if has_cells[oi] else base_of[oi])
            for u in near:
                if not labels[u] and cls[u] == c0:
                    labels[u] = count
                    queue.append(u)
    return count, np.array(labels, np.uint32), (order, bases, total)


def with_label(records, labels):
    """records with their component word replaced"""
    r = np.asarray(records, np.uint64)
    return (r & np.uint64(0xFFFFFFFF)) | (np.asarray(labels, np.uint64).reshape(r.shape) << np.uint64(32))


def apply(m, flags=0):
    """Write the labels into the component words of m's records, as sdfgpu_dsh_update_components does; returns K.  m.export(), m.get()
    and m.window() then answer as the map must after the update."""
    count, labels, (order, bases, _) = components(m, flags)
    cpc = int(np.prod(m.n))
    for c in order:
        kind, what = m.chunks[c]
        b = bases[c]
        if kind == "cells":
            m.chunks[c] = ("cells", with_label(what, labels[b:b + cpc].reshape(m.n)))
        else:
            m.chunks[c] = ("chunk", int(with_label([what], labels[b:b + 1])[0]))
    return count
