"""Local extrema and convex segments without a GPU: the C++ restatement of the reference's ComputeLocalExtremaMap and
UpdateConvexSegments (tests/convex_segments_restated.cpp) pinned to hand-derived answers, and a model of the GPU's scheme (pointer
doubling with the cycle test, then the basin-minimum entry walk) checked against a literal memoised walk on random functional
graphs, once with tagged tuples for states and once word by word, markers and all, up to the largest grid the library accepts.
tests/test_gpu_convex_segments.py compares the GPU with the same restatement."""
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


# ---- the five extrema kernels restated on W-bit words ------------------------------------------------------------------------------
# The accepted grid size, in one place: check_convex_args (sdfgpu_convex.hip) refuses n >= 2^32 - 2, so the largest grid it accepts has
# n = 2^32 - 3 voxels.  At word width W that is n = 2^W - CX_N_MARGIN; indices then stay below the three markers.
CX_N_MARGIN = 3


def cx_max_accepted_n(W):
    return (1 << W) - CX_N_MARGIN


def word_model(nxt, W, seed=0):
    """k_cx_next, k_cx_round, k_cx_basin, k_cx_entry and k_cx_final (sdfgpu_convex.hip) on W-bit words: a state packs the high
    word over the low one, kCxOff = kResTerm = 2^W - 1, kResCycle = 2^W - 2, kOnCycle = 2^W - 3, and `resolved` compares the low
    word with kOnCycle, as the kernels do.  nxt[v] = v at a terminal, -1 for OFF.  Each round's lanes run one after another in a
    seeded random order, with the in-place marker writes the kernel makes (one of the interleavings the device may take).  Every
    index a kernel reads is checked against n, every walk against n steps.  Returns (extremum per node, -1 = OFF; rounds)."""
    n = len(nxt)
    assert n <= (1 << W) - 1
    off = term = (1 << W) - 1
    cyc, onc = (1 << W) - 2, (1 << W) - 3
    mask = (1 << W) - 1

    def pack(hi, lo):
        return (hi << W) | lo

    def hi(s):
        return s >> W

    def lo(s):
        return s & mask

    def resolved(s):
        return lo(s) >= onc

    def rd(buf, i):
        assert 0 <= i < n, "read at %d, n = %d" % (i, n)
        assert buf[i] is not None, "read of an unwritten word at %d" % i
        return buf[i]

    rng = random.Random(seed)
    # k_cx_next
    nx_w = [off if t == -1 else t for t in nxt]
    A, B = [None] * n, [None] * n
    for v in range(n):
        t = nxt[v]
        s = pack(v, term) if t == v else (pack(off, term) if t == -1 else pack(t, v))
        A[v] = s
        if resolved(s):
            B[v] = s
    # k_cx_round
    rounds = 0
    for k in range(W + 8):
        src, dst = (B, A) if k & 1 else (A, B)
        order = list(range(n))
        rng.shuffle(order)
        open_ = 0
        for v in order:
            s = rd(src, v)
            if resolved(s):
                continue
            p = hi(s)
            r, done = pack(off, term), True
            if p != off:
                sp = rd(src, p)
                if resolved(sp):
                    r = sp
                else:
                    c = lo(sp)
                    d = nx_w[c] if 0 <= c < n else None
                    assert d is not None, "next read at %d, n = %d" % (c, n)
                    if d != off:
                        sd = rd(src, d)
                        if resolved(sd):
                            r = sd
                        elif lo(sd) == c:
                            r = pack(c, cyc)
                        else:
                            done = False
                            dst[v] = pack(hi(sp), min(lo(s), c))
            if done:
                dst[v] = r
                src[v] = r
            else:
                open_ += 1
        if open_ == 0:
            rounds = k + 1
            break
    else:
        raise AssertionError("no round left every node resolved")
    # k_cx_basin (slot: B's words, all ones)
    slot = [off] * n
    for v in range(n):
        s = A[v]
        if lo(s) == cyc:
            c = hi(s)
            assert c < n
            slot[c] = min(slot[c], v)
    # k_cx_entry
    for v in range(n):
        s = A[v]
        if lo(s) == cyc and hi(s) == v:
            u, steps = v, 0
            while True:
                A[u] = pack(v, onc)
                u = nx_w[u]
                steps += 1
                assert 0 <= u < n and steps <= n, "cycle walk from %d left the graph" % v
                if u == v:
                    break
            w, steps = slot[v], 0
            while True:
                assert 0 <= w < n and steps <= n, "entry walk of cycle %d at %d" % (v, w)
                if lo(A[w]) == onc:
                    break
                w = nx_w[w]
                steps += 1
            slot[v] = w
    # k_cx_final
    ext = []
    for v in range(n):
        s = A[v]
        if lo(s) == term:
            e = hi(s)
        else:
            assert hi(s) < n, "slot read at %d, n = %d" % (hi(s), n)
            e = slot[hi(s)]
        ext.append(-1 if e == off else e)
    return ext, rounds


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


def _last_steps_inward(rng, n):
    """A random functional graph whose last node steps to another node of the graph (not a terminal, not OFF)."""
    g = random_functional_graph(rng, n)
    if n > 1:
        g[n - 1] = rng.randrange(n - 1)
    return g


def _word_graphs(rng, W, n, count):
    """Random graphs at n, half of them with a last node that steps inward, plus a path and a two-cycle through the last node."""
    out = [_last_steps_inward(rng, n) if i % 2 else random_functional_graph(rng, n) for i in range(count)]
    if n < 4:
        return out
    out.append([v + 1 for v in range(n - 1)] + [n - 2])                       # a path ending in the 2-cycle {n-2, n-1}
    out.append([min(v + 1, n - 3) if v < n - 3 else (v + 1 if v < n - 1 else n - 3) for v in range(n)])   # ... {n-3, n-2, n-1}
    return out


@pytest.mark.parametrize("W", [6, 7, 8])
def test_word_model_matches_the_memoised_walk_up_to_the_accepted_bound(W):
    """The kernels' word arithmetic at every n up to the largest grid check_convex_args accepts, scaled to W bits: the same answer
    as the literal walk, every read in bounds, every walk ended."""
    rng = random.Random(1000 + W)
    top = cx_max_accepted_n(W)
    for n in [1, 2, 3, top - 2, top - 1, top] + [rng.randint(4, top) for _ in range(6)]:
        for trial, nxt in enumerate(_word_graphs(rng, W, n, 100 if n == top else 6)):
            got, rounds = word_model(nxt, W, seed=trial)
            assert got == literal_walk(nxt), (W, n, trial, nxt)
            assert rounds <= max(1, math.ceil(math.log2(max(n, 2)))) + 1, (W, n, rounds)


@pytest.mark.parametrize("W", [6, 7, 8])
def test_word_model_sees_the_marker_collision_one_past_the_bound(W):
    """One voxel more than the bound: the last index equals kOnCycle, its round-0 state reads as resolved, and graphs whose last
    node steps inward come back wrong -- the case the bound exists for (the tuple model above cannot see it)."""
    rng = random.Random(2000 + W)
    n = cx_max_accepted_n(W) + 1
    assert n - 1 == (1 << W) - 3
    wrong = 0
    for trial in range(40):
        nxt = _last_steps_inward(rng, n)
        got, _ = word_model(nxt, W, seed=trial)
        want = literal_walk(nxt)
        if got != want:
            wrong += 1
            assert got[n - 1] != want[n - 1]                                   # the last node itself is always among them
    assert wrong > 0
    path = [v + 1 for v in range(n - 1)] + [n - 2]                             # (every node's orbit passes the last one)
    got, _ = word_model(path, W)
    assert got[n - 1] == -1 and literal_walk(path)[n - 1] == n - 2


def test_word_model_agrees_with_the_tuple_model_on_small_graphs():
    rng = random.Random(77)
    for trial in range(400):
        n = rng.randint(1, 40)
        nxt = random_functional_graph(rng, n)
        assert word_model(nxt, 8, seed=trial)[0] == doubling_model(nxt)[0] == literal_walk(nxt), (trial, nxt)


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
