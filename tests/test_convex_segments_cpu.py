"""Local extrema and convex segments without a GPU: the C++ restatement of the reference's ComputeLocalExtremaMap and
UpdateConvexSegments (tests/convex_segments_restated.cpp) pinned to hand-derived answers, and a model of the GPU's scheme (pointer
doubling with the cycle test, then the basin-minimum entry walk) checked against a literal memoised walk on random functional
graphs.  tests/test_gpu_convex_segments.py compares the GPU with the same restatement."""
import ctypes
import math
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = []
INF = math.inf
OFF = 0xFFFFFFFF


def _restated_lib():
    if not _LIB:
        out = os.path.join(tempfile.mkdtemp(prefix="convex_restated_"), "convex_segments_restated.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fPIC", "-shared",
                               os.path.join(HERE, "convex_segments_restated.cpp"), "-o", out])
        L = ctypes.CDLL(out)
        L.cx_extrema_restated.restype = ctypes.c_int
        L.cx_extrema_restated.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_double,
                                          ctypes.c_void_p, ctypes.c_void_p]
        L.cx_segments_restated.restype = ctypes.c_uint32
        L.cx_segments_restated.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_int64, ctypes.c_double, ctypes.c_void_p]
        _LIB.append(L)
    return _LIB[0]


def restated_extrema(sdf, res, q=(1.0, 0.0, 0.0, 0.0)):
    """The reference's local extrema map of a float32 [nx, ny, nz] field: float64 [nx, ny, nz, 3]."""
    f = np.ascontiguousarray(sdf, dtype=np.float32)
    out = np.empty(f.shape + (3,), np.float64)
    qq = np.array(q, np.float64)
    _restated_lib().cx_extrema_restated(f.ctypes.data, *f.shape, float(res), qq.ctypes.data, out.ctypes.data)
    return out


def restated_segments(occupancy, object_id, extrema, threshold):
    """The reference's UpdateConvexSegments over given extrema: (labels uint32 [nx, ny, nz], K)."""
    occ = np.ascontiguousarray(occupancy, dtype=np.float32)
    obj = np.ascontiguousarray(object_id, dtype=np.uint32)
    ext = np.ascontiguousarray(extrema, dtype=np.float64)
    labels = np.empty(occ.shape, np.uint32)
    k = _restated_lib().cx_segments_restated(occ.ctypes.data, obj.ctypes.data, ext.ctypes.data, *occ.shape, float(threshold),
                                             labels.ctypes.data)
    return labels, int(k)


def tagged_sdf(occupancy, object_id, res, add_virtual_border, sdf_of):
    """The SDF UpdateConvexSegments walks: sdf_of(filled_mask, border) builds one SDF (the oracle or the GPU); with the border,
    every filled cell (occupancy > 0.5 or == 0.5: unknown is filled); otherwise free space outside, named objects inside."""
    occ = np.asarray(occupancy, np.float32)
    filled = (occ > 0.5) | (occ == 0.5)
    if add_virtual_border:
        return sdf_of(filled, True)
    fr = sdf_of(filled, False)
    nm = sdf_of(filled & (np.asarray(object_id) > 0), False)
    return np.where(fr >= 0.0, fr, np.where(nm <= -0.0, nm, np.float32(0.0))).astype(np.float32)


def loc(i, shape, res):
    _, ny, nz = shape
    return (res * (i // (ny * nz) + 0.5), res * ((i // nz) % ny + 0.5), res * (i % nz + 0.5))


def rot_z(deg):
    t = math.radians(deg)
    return (math.cos(t / 2), 0.0, 0.0, math.sin(t / 2))


# ---- an independent Python next() (same arithmetic as GetGradient(v, true) + GetNextFromGradient) -------------------------------
def _qmul(a, o):
    return (a[0] * o[0] - a[1] * o[1] - a[2] * o[2] - a[3] * o[3], a[0] * o[1] + a[1] * o[0] + a[2] * o[3] - a[3] * o[2],
            a[0] * o[2] - a[1] * o[3] + a[2] * o[0] + a[3] * o[1], a[0] * o[3] + a[1] * o[2] - a[2] * o[1] + a[3] * o[0])


def next_map(sdf, res, q=(1.0, 0.0, 0.0, 0.0)):
    """next(v) for every voxel as a list: v itself at a terminal, -1 for a step out of the grid."""
    f = np.asarray(sdf, np.float32)
    nx, ny, nz = f.shape
    n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    qi = (q[0] / n, -q[1] / n, -q[2] / n, -q[3] / n)
    s = res * 0.06125
    out = []
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                if 0 < x < nx - 1 and 0 < y < ny - 1 and 0 < z < nz - 1:
                    inv = 1.0 / (2.0 * res)
                    g = [float(f[x + 1, y, z] - f[x - 1, y, z]) * inv, float(f[x, y + 1, z] - f[x, y - 1, z]) * inv,
                         float(f[x, y, z + 1] - f[x, y, z - 1]) * inv]
                else:
                    g = []
                    for ax, (c, m) in enumerate(((x, nx), (y, ny), (z, nz))):
                        lo, hi = max(0, c - 1), min(m - 1, c + 1)
                        w = float(hi - lo) * res
                        if w > 0.0:
                            a, b = [x, y, z], [x, y, z]
                            a[ax], b[ax] = hi, lo
                            g.append((float(f[tuple(a)]) - float(f[tuple(b)])) * (1.0 / w))
                        else:
                            g.append(0.0)
                r = _qmul(q, _qmul((0.0, g[0], g[1], g[2]), qi))
                w = [r[1], r[2], r[3]]
                if f[x, y, z] < 0.0:
                    w = [c * -1.0 for c in w]
                d = [1 if c > s else (-1 if c < -s else 0) for c in w]
                X, Y, Z = x + d[0], y + d[1], z + d[2]
                if 0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz:
                    out.append((X * ny + Y) * nz + Z)
                else:
                    out.append(-1)
    return out


def literal_walk(nxt):
    """The reference's memoised walk on a functional graph (nxt[v] = v terminal, -1 OFF): extremum index per node (-1 = OFF)."""
    memo = [None] * len(nxt)
    for v in range(len(nxt)):
        if memo[v] is not None:
            continue
        if nxt[v] == v:
            memo[v] = v
            continue
        path, cur, e = {v}, v, None
        while True:
            cur = nxt[cur]
            if cur in path:
                e = cur
                break
            if cur == -1:
                e = -1
                break
            path.add(cur)
            if memo[cur] is not None:
                e = memo[cur]
                break
            if nxt[cur] == cur:
                e = cur
                break
        for u in path:
            memo[u] = e
    return memo


def doubling_model(nxt):
    """The GPU's scheme, round by round (sdfgpu_convex.hip): (extremum per node, rounds used)."""
    n = len(nxt)
    S = []
    for v in range(n):
        if nxt[v] == v:
            S.append(("T", v))
        elif nxt[v] == -1:
            S.append(("T", -1))
        else:
            S.append((nxt[v], v))                    # (p_0, m_0)
    rounds = 0
    while True:
        rounds += 1
        new, open_ = list(S), 0
        for v in range(n):
            s = S[v]
            if isinstance(s[0], str):
                continue
            p, m = s
            sp = S[p]
            if isinstance(sp[0], str):
                new[v] = sp
                continue
            c = sp[1]
            d = nxt[c]
            if d == -1:
                new[v] = ("T", -1)
                continue
            sd = S[d]
            if isinstance(sd[0], str):
                new[v] = sd
            elif sd[1] == c:
                new[v] = ("C", c)
            else:
                new[v] = (sp[0], min(m, c))
                open_ += 1
        S = new
        if open_ == 0:
            break
        assert rounds <= max(1, math.ceil(math.log2(max(n, 2)))) + 1
    slot = {}
    for v in range(n):
        if S[v][0] == "C":
            slot[S[v][1]] = min(slot.get(S[v][1], n), v)
    entry = {}
    for c, b in slot.items():
        on = set()
        u = c
        while True:
            on.add(u)
            u = nxt[u]
            if u == c:
                break
        u = b
        while u not in on:
            u = nxt[u]
        entry[c] = u
    return [S[v][1] if S[v][0] == "T" else entry[S[v][1]] for v in range(n)], rounds


def random_functional_graph(rng, n):
    kind = rng.random()
    out = []
    for v in range(n):
        r = rng.random()
        if r < 0.08 * kind:
            out.append(v)
        elif r < 0.08 * kind + 0.05:
            out.append(-1)
        else:
            out.append(rng.randrange(n))
    return out


# ---- the GPU's scheme against the literal walk --------------------------------------------------------------------------------
def test_doubling_model_matches_the_memoised_walk_on_random_functional_graphs():
    rng = random.Random(20261015)
    lengths = set()
    for trial in range(3000):
        n = rng.randint(1, 60)
        nxt = random_functional_graph(rng, n)
        got, _ = doubling_model(nxt)
        assert got == literal_walk(nxt), (trial, nxt)
        for v in range(n):                           # (collect the cycle lengths seen)
            u, seen = v, {}
            while u != -1 and u not in seen:
                seen[u] = len(seen)
                u = nxt[u]
            if u != -1:
                lengths.add(len(seen) - seen[u])
    assert {1, 2, 3, 4, 5, 8}.issubset(lengths)


def test_doubling_model_on_long_cycles_and_paths():
    n = 1000
    ring = [(v + 1) % n for v in range(n)]
    got, rounds = doubling_model(ring)
    assert got == [0] * n and rounds <= 11          # the basin minimum 0 is on the ring: it enters at itself
    path = [v + 1 for v in range(n - 1)] + [n - 1]
    got, rounds = doubling_model(path)
    assert got == [n - 1] * n and rounds <= 11


# ---- the restatement on hand-derived fields -------------------------------------------------------------------------------------
def test_corridor_ridge_between_two_voxels_maps_to_the_lower_one():
    """z: 0.5 1.5 2.5 3.5 | 3.5 2.5 1.5 0.5.  Voxels 3 and 4 point at each other; the scan's first walk (from 0) enters the
    2-cycle at 3, so the whole corridor maps to voxel 3."""
    f = np.array([0.5, 1.5, 2.5, 3.5, 3.5, 2.5, 1.5, 0.5], np.float32).reshape(1, 1, 8)
    assert next_map(f, 1.0) == [1, 2, 3, 4, 3, 4, 5, 6]
    e = restated_extrema(f, 1.0)
    assert np.array_equal(e, np.broadcast_to(np.array([0.5, 0.5, 3.5]), (1, 1, 8, 3)))


def _cycles(nxt):
    found = {}
    for v in range(len(nxt)):
        u, seen = v, []
        while u != -1 and u not in seen:
            seen.append(u)
            u = nxt[u]
        if u != -1 and nxt[u] != u:
            cyc = seen[seen.index(u):]
            found[min(cyc)] = cyc
    return found


def _find_scan_rule_fields():
    rng = np.random.default_rng(7)
    want = {3: None, 4: None}
    for _ in range(20000):
        f = rng.random((1, 4, 4)).astype(np.float32)
        nxt = next_map(f, 1.0)
        memo = literal_walk(nxt)
        for cmin, cyc in _cycles(nxt).items():
            L = len(cyc)
            if L not in want or want[L] is not None:
                continue
            basin = [v for v in range(len(nxt)) if memo[v] in cyc]
            b = min(basin)
            u = b
            while u not in cyc:
                u = nxt[u]
            if u != cmin:
                want[L] = (f, cyc, b, u)
        if all(v is not None for v in want.values()):
            return want
    return want


def test_scan_order_rule_for_3_and_4_cycles():
    found = _find_scan_rule_fields()
    for L in (3, 4):
        assert found[L] is not None, "no %d-cycle case in the search" % L
        f, cyc, b, entry = found[L]
        assert entry != min(cyc)
        nxt = next_map(f, 1.0)
        e = restated_extrema(f, 1.0)
        shape = f.shape
        for v in range(len(nxt)):
            if literal_walk(nxt)[v] in cyc:
                assert tuple(e.reshape(-1, 3)[v]) == loc(entry, shape, 1.0), (L, v)
        # ... and not the cycle minimum
        assert tuple(e.reshape(-1, 3)[b]) != loc(min(cyc), shape, 1.0)


def test_edge_gradient_leaving_the_grid_is_off():
    f = np.array([1.0, 2.0, 3.0, 4.0], np.float32).reshape(1, 1, 4)
    assert next_map(f, 1.0) == [1, 2, 3, -1]
    assert np.all(np.isposinf(restated_extrema(f, 1.0)))


def test_field_without_filled_voxels_every_voxel_is_its_own_extremum():
    f = np.full((3, 4, 5), np.inf, np.float32)         # (an SDF with no filled voxel: inf - inf = NaN gradients)
    e = restated_extrema(f, 0.5)
    idx = np.arange(f.size)
    want = np.stack([0.5 * (idx // 20 + 0.5), 0.5 * ((idx // 5) % 4 + 0.5), 0.5 * (idx % 5 + 0.5)], -1).reshape(3, 4, 5, 3)
    assert np.array_equal(e, want)


def test_rotated_frame_changes_the_step():
    """x: 0.5 1.5 1.5 0.5 on a 4 x 1 x 1 grid: unrotated, 1 and 2 form a 2-cycle entered at 1; rotated 30 degrees about z the
    gradient (+-0.5, 0, 0) becomes (+-0.433, +-0.25, 0), which also steps in y and leaves the one-cell-wide grid."""
    f = np.array([0.5, 1.5, 1.5, 0.5], np.float32).reshape(4, 1, 1)
    assert next_map(f, 1.0) == [1, 2, 1, 2]
    assert np.array_equal(restated_extrema(f, 1.0), np.broadcast_to(np.array([1.5, 0.5, 0.5]), (4, 1, 1, 3)))
    q = rot_z(30.0)
    assert next_map(f, 1.0, q) == [-1, -1, -1, -1]
    assert np.all(np.isposinf(restated_extrema(f, 1.0, q)))


def test_restatement_matches_the_python_walk_on_random_fields():
    rng = np.random.default_rng(3)
    for shape, q in (((3, 4, 5), (1.0, 0.0, 0.0, 0.0)), ((4, 4, 4), rot_z(30.0)), ((1, 6, 7), rot_z(-75.0)), ((5, 1, 3), (1.0, 0.0, 0.0, 0.0))):
        f = (rng.random(shape) * 4 - 1).astype(np.float32)
        nxt = next_map(f, 0.7, q)
        memo = literal_walk(nxt)
        want = np.array([loc(m, shape, 0.7) if m >= 0 else (INF, INF, INF) for m in memo]).reshape(shape + (3,))
        assert np.array_equal(restated_extrema(f, 0.7, q), want)


# ---- segments ---------------------------------------------------------------------------------------------------------------------
def _two_cells(e0, e1, occ=(0.0, 0.0), obj=(0, 0)):
    ext = np.array([e0, e1], np.float64).reshape(1, 1, 2, 3)
    return np.array(occ, np.float32).reshape(1, 1, 2), np.array(obj, np.uint32).reshape(1, 1, 2), ext


@pytest.mark.parametrize("d, lo", [(1.0, False), (math.sqrt(2.0), False), (math.sqrt(3.0), False)])
def test_threshold_is_strict(d, lo):
    a = (0.5, 0.5, 0.5)
    b = {1.0: (1.5, 0.5, 0.5), math.sqrt(2.0): (1.5, 1.5, 0.5), math.sqrt(3.0): (1.5, 1.5, 1.5)}[d]
    occ, obj, ext = _two_cells(a, b)
    assert restated_segments(occ, obj, ext, math.nextafter(d, 0.0))[1] == 2
    assert restated_segments(occ, obj, ext, d)[1] == 2                 # distance == threshold: not joined
    labels, k = restated_segments(occ, obj, ext, math.nextafter(d, 3.0))
    assert k == 1 and labels.tolist() == [[[1, 1]]]


def test_same_extremum_joins_for_any_positive_threshold():
    occ, obj, ext = _two_cells((2.5, 0.5, 0.5), (2.5, 0.5, 0.5))
    assert restated_segments(occ, obj, ext, 5e-324)[1] == 1
    assert restated_segments(occ, obj, ext, 0.0)[1] == 2


def test_cells_that_take_no_part():
    # NaN occupancy with object 0, a filled object-0 cell, an OFF extremum: label 0.  A filled named cell takes part.
    ext = np.tile(np.array([0.5, 0.5, 0.5]), (1, 1, 5, 1))
    ext[0, 0, 3] = INF
    occ = np.array([np.nan, 1.0, 0.2, 0.2, 1.0], np.float32).reshape(1, 1, 5)
    obj = np.array([0, 0, 0, 0, 4], np.uint32).reshape(1, 1, 5)
    labels, k = restated_segments(occ, obj, ext, 1.0)
    assert labels.tolist() == [[[0, 0, 1, 0, 2]]] and k == 2
    obj[0, 0, 0] = 9                                                   # NaN occupancy of a named object takes part
    labels, k = restated_segments(occ, obj, ext, 1.0)
    assert labels.tolist() == [[[1, 0, 2, 0, 3]]] and k == 3


def test_object_id_boundaries_split_segments_and_numbering_is_scan_order():
    ext = np.tile(np.array([0.5, 0.5, 0.5]), (2, 3, 1, 1))
    occ = np.zeros((2, 3, 1), np.float32)
    obj = np.array([[[2], [2], [1]], [[1], [2], [1]]], np.uint32)
    labels, k = restated_segments(occ, obj, ext, 1.0)
    assert k == 3
    assert labels[:, :, 0].tolist() == [[1, 1, 2], [3, 1, 2]]
