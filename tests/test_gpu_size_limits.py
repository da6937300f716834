"""GPU: exact SDF builds at the edges where the library changes kernels or arithmetic.

* the far-field kernel's 32-bit key limit (envelope_dc_geometry, sdfgpu.hip): for each line length, the in-gate shape
  with the largest finf and the first shape past it, on both swept axes -- the far-field kernel must be exact where it
  is admitted and must not run where it is not;
* 1024^3, inside the gate, and 1024 x 1024 x 1025, one plane past it;
* lines of 1025 .. 16384 voxels (never far-field) and the size refusal at 16385;
* grids of more than 2^31 voxels (linear indices past 2^31) for the SDF and the connected components;
* component topology past 2^31 node ids (512 slabs at 3072 x 1024 x 1024), past 2^32 vertices (one box of 2^32 - 2^17 voxels,
  with and without a selection) and its refusal of more than 2^32 - 1 nodes (the all-even lattice: nothing allocated for them);
* local extrema at n = 2^32 - 3, the largest grid check_convex_args accepts (its last index one below the kOnCycle marker), with
  a basin and doubling windows across index 2^31.

The byte-mask build above runs the point lattice (distances of at most 5 voxels) and Bernoulli(0.5) past 2^31 voxels; the batched
build's launch of 2^32 threads is in test_gpu_batch_edges.py, the projection and gradient-query kernels' 1300 x 1300 x 1272 fields in
test_gpu_projection.py and test_gpu_query_gradients.py.  The other entry points at these sizes -- a far-field scene on the marching
sweeps, bits in, cells in, voxelisation, the full-field gradient, point queries, a host-to-host build -- are in
test_gpu_size_limits_entry_points.py, which imports this module's closed forms.  The closed-form pins of this module carry the gpu
marker with the rest of it (they need no GPU); those of the sibling module do not.

Every reference is independent of the library: the oracle's exact EDT, or a closed form in int64 whose float32 values come
from a table computed on the host like the oracle computes them (sqrt and multiply in float64, one cast), or a closed form
in int64 of the topology counters and extremum indices.  Each closed form is first checked against the oracle (or the C++
restatements of the reference's topology and extrema) on a small grid of the same pattern.  All comparisons are bit for bit."""
import math
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as O
from sdf_tools_amd import capi, synth

pytestmark = pytest.mark.gpu

# ---- envelope_dc_geometry (sdfgpu.hip) and envelope_dc_lds_bytes (sdfgpu_envelope_dc.hpp), restated -----------------------
K_DC_LINES, K_DC_MISC, K_DC_LOCAL_FILLED = 16, 80, 448
K_DC_MAX_DYNAMIC_LDS = 160 * 1024 - 256
K_MAX_DIM, K_INF32 = 16384, 1 << 30


def canonical(shape):
    """canonical_dims: singleton axes move to the front (the layout is unchanged)."""
    nx, ny, nz = shape
    if nz == 1:
        nx, ny, nz = 1, nx, ny
    if nz == 1:
        nx, ny, nz = 1, nx, ny
    if ny == 1:
        nx, ny = 1, nx
    return nx, ny, nz


def dims_ok(shape):
    return all(1 <= s <= K_MAX_DIM for s in shape) and sum(s * s for s in shape) < K_INF32


def dc_lds_bytes(L):
    pitch = ((L + 63) // 64) * 64 + 2
    M = (L + 7) // 8
    return (K_DC_LINES * pitch + (M + 2) * K_DC_LINES + K_DC_MISC + K_DC_LOCAL_FILLED) * 4


def dc_gates(stage, shape):
    """The far-field kernel's gates for one swept axis (stage 2 = y, 3 = x) of a canonical shape."""
    nx, ny, nz = shape
    L = ny if stage == 2 else nx
    B = 1
    while (1 << B) < L:
        B += 1
    finf = (nx - 1) ** 2 + (ny - 1) ** 2 + (nz - 1) ** 2 + 1
    return {
        "L": L, "B": B, "finf": finf,
        "line": 1 <= L <= 2048 and nx * ny * nz < (1 << 31),
        "key": finf + (L + 2) ** 2 < (1 << (32 - B)),
        "mad24": (L + 2) * (2 << B) < (1 << 23),
        "lds": dc_lds_bytes(L) <= K_DC_MAX_DYNAMIC_LDS,
    }


def far_ok(shape):
    """Whether a build of `shape` may take the far-field kernels at all (both swept axes must pass every gate)."""
    c = canonical(shape)
    return all(all(v for k, v in dc_gates(st, c).items() if k in ("line", "key", "mad24", "lds")) for st in (2, 3))


def gated_stage(shape):
    """The swept axis whose gate a key-limit shape probes: the longer of the canonical y and x lines."""
    nx, ny, _ = canonical(shape)
    return 2 if ny >= nx else 3


# ---- key-limit shapes --------------------------------------------------------------------------------------------------------
L_VALUES = (16, 64, 256, 257, 512, 513, 1024)


def _line_shape(L, axis, c, nz):
    return (L, c, nz) if axis == "x" else (c, L, nz)


def key_limit_shapes(L, axis, c):
    """(in, past, wraps) along nz in steps of 16: the in-gate shape with the largest finf, the first shape past it and the
    largest shape whose finf alone still fits the key width (inside a gate without its (L + 2)^2 term; its candidate keys
    wrap).  None where the shape does not exist within the dims limit."""
    def fits(nz):
        s = _line_shape(L, axis, c, nz)
        return dims_ok(s) and far_ok(s)

    nz_in = max(nz for nz in range(16, K_MAX_DIM + 1, 16) if fits(nz))
    out = _line_shape(L, axis, c, nz_in + 16)
    if not dims_ok(out):
        return _line_shape(L, axis, c, nz_in), None, None
    g = dc_gates(gated_stage(out), canonical(out))
    assert not g["key"] and g["line"] and g["mad24"] and g["lds"], (out, g)     # the key gate, and nothing else, turns it away
    wraps = None
    for nz in range(nz_in + 32, K_MAX_DIM + 1, 16):
        s = _line_shape(L, axis, c, nz)
        g = dc_gates(gated_stage(s), canonical(s))
        if not dims_ok(s) or g["finf"] >= (1 << (32 - g["B"])):
            break
        wraps = s
    return _line_shape(L, axis, c, nz_in), out, wraps


def _key_cases():
    cases, seen = [], set()
    for L in L_VALUES:
        for axis, c in (("y", 1), ("y", 3), ("x", 3)):
            sin, sout, swrap = key_limit_shapes(L, axis, c)
            for kind, s in (("in", sin), ("past", sout), ("wraps", swrap if c == 3 else None)):
                if s is not None and canonical(s) not in seen:
                    seen.add(canonical(s))
                    cases.append((kind, s))
    # one nz that is not a multiple of 16, at the exact bound, on each side of it
    cases += [("in", (1024, 3, 1448)), ("past", (1024, 3, 1449))]
    return cases


KEY_CASES = _key_cases()


def test_key_limit_geometry_restated():
    """The restated gates: the shapes the issue names, and which gate decides for lines longer than 1024."""
    assert far_ok((1024, 1, 1440)) and not far_ok((1024, 1, 1456))
    assert far_ok((1, 256, 4080)) and not far_ok((1, 256, 4096))
    assert far_ok((16, 1, 16384))
    assert far_ok((1024, 1024, 1024)) and not far_ok((1024, 1024, 1025))
    g = dc_gates(3, (1024, 1024, 1024))
    assert (1 << 22) - (g["finf"] + 1026 ** 2) == 2040                   # the headline input's headroom
    assert far_ok((1024, 3, 1448)) and not far_ok((1024, 3, 1449))
    # past 1024 the key gate turns every line away, whatever its cross-section: L = 2048 would pass the L <= 2048 test
    # and the LDS test but fails both the key and the 24-bit gate
    for L in (1025, 1500, 2045, 2048):
        g = dc_gates(3, (L, 2, 2))
        assert not g["key"] and g["lds"], (L, g)
    assert not dc_gates(3, (2048, 2, 2))["mad24"] and dc_gates(3, (2045, 2, 2))["mad24"]
    assert not far_ok((3072, 1024, 1024))                                  # 2^31 voxels or more: never
    for kind, s in KEY_CASES:
        assert far_ok(s) == (kind == "in"), (kind, s)
        assert dims_ok(s), s


# ---- scenes --------------------------------------------------------------------------------------------------------------------
def edge_scenes(shape, seed, ax):
    """One filled voxel in a corner (the opposite corner holds d^2 = finf - 1, the largest real key), its inverse, two opposite
    corners, all free, sparse Bernoulli, noisy sheets across both ends of the lines along axis `ax`."""
    nx, ny, nz = shape
    corner = np.zeros(shape, np.uint8)
    corner[0, 0, 0] = 1
    two = corner.copy()
    two[nx - 1, ny - 1, nz - 1] = 1
    rng = np.random.default_rng(seed)
    sheets = np.zeros(shape, np.uint8)
    n_ax = shape[ax]
    for pos in sorted({min(2, n_ax - 1), max(n_ax - 3, 0)}):
        sl = [slice(None)] * 3
        sl[ax] = pos
        sheets[tuple(sl)] = (rng.random(sheets[tuple(sl)].shape) < 0.08).astype(np.uint8)
    sheets[(0,) * 3] = 1                                                  # (never an empty sheet on thin cross-sections)
    return {"corner": corner, "inverse corner": 1 - corner, "two corners": two, "all free": np.zeros(shape, np.uint8),
            "sparse": synth.bernoulli_mask(shape, 0.002, seed), "sheets": sheets}


def _oracles(jobs):
    """O.exact_sdf for several (mask, res, vb) at once (the oracle's ctypes calls release the GIL)."""
    with ThreadPoolExecutor(max_workers=6) as ex:
        return list(ex.map(lambda j: O.exact_sdf(*j), jobs))


def _assert_bits(name, got, want):
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError("%s: %d voxels differ, first at %s got %r want %r" % (
            name, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- 1. the key limit, both swept axes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", KEY_CASES, ids=["%s-%s" % (k, "x".join(map(str, s))) for k, s in KEY_CASES])
def test_far_field_key_limit_is_exact(gpu, kind, shape):
    """Each shape through the library's own tier selection and with the far-field kernel as the only sweep of each axis, under the
    (envelope_dc, i32_handoff) matrix of the divide-and-conquer test: bit for bit against the oracle, virtual border off and on.
    The far-field kernels run on in-gate shapes and never on the others."""
    res = 0.05
    inside = kind == "in"
    st = gated_stage(shape)
    flag = "far_y" if st == 2 else "far_x"
    finf = dc_gates(st, canonical(shape))["finf"]
    sc = edge_scenes(shape, sum(shape) * 7 + len(kind), 1 if st == 2 else 0)
    jobs = [(m, res, vb) for m in sc.values() for vb in (False, True)]
    want = dict(zip([(n, vb) for n in sc for vb in (False, True)], _oracles(jobs)))
    assert want[("corner", False)][2].max() == finf - 1                  # the largest real key is there
    assert -want[("inverse corner", False)][2].min() == finf - 1
    paths = []
    try:
        for name, m in sc.items():
            for vb in (False, True):
                ex, ex_ext, _ = want[(name, vb)]
                tag = "%s %s vb=%d" % (shape, name, vb)
                gpu.set_option("policy_reset", 1)
                sdf, ext = gpu.build(m, res, vb)
                path = gpu.last_path()
                paths.append("%s:%s%s" % (name[:6], "y" if path["far_y"] else "-", "x" if path["far_x"] else "-"))
                _assert_bits(tag + " (tier selection)", sdf, ex)
                assert ext == ex_ext, (tag, ext, ex_ext)
                if not inside:
                    assert not path["far_y"] and not path["far_x"], (tag, path)
                gpu.set_option("dense", 0)
                for dc, ho in ((1, 1), (1, 0), (0, 1)):
                    gpu.set_option("envelope_dc", dc)
                    gpu.set_option("i32_handoff", ho)
                    gpu.set_option("envelope_mode", 1)
                    sdf, ext = gpu.build(m, res, vb)
                    path = gpu.last_path()
                    t = "%s dc=%d handoff=%d" % (tag, dc, ho)
                    _assert_bits(t, sdf, ex)
                    assert ext == ex_ext, (t, ext, ex_ext)
                    if not (inside and dc):
                        assert not path["far_y"] and not path["far_x"], (t, path)
                    elif name != "all free":
                        assert path[flag], (t, path)
                gpu.set_option("envelope_dc", 1)
                gpu.set_option("i32_handoff", 1)
                gpu.set_option("envelope_mode", 0)
                gpu.set_option("dense", 1)
    finally:
        gpu.set_option("envelope_dc", 1)
        gpu.set_option("i32_handoff", 1)
        gpu.set_option("envelope_mode", 0)
        gpu.set_option("dense", 1)
        gpu.set_option("policy_reset", 1)
    print("\n[size-limits] key %-5s %-18s finf=%d tier selection paths: %s" % (kind, "x".join(map(str, shape)), finf, " ".join(paths)))


# ---- closed forms on the device: int64 d^2 -> float32 through a host table --------------------------------------------------------
def _finish_table(dmax, res):
    """float32(sqrt(D) * res) for D = 0 .. dmax, computed like the oracle (float64 sqrt and multiply, one cast)."""
    return (np.sqrt(np.arange(dmax + 1, dtype=np.float64)) * res).astype(np.float32)


def _vb_sq(n, lo, hi, device):
    """Per-axis squared virtual-border distance min(i + 1, n - i)^2 over [lo, hi), or None for a singleton axis."""
    import torch
    if n <= 1:
        return None
    i = torch.arange(lo, hi, dtype=torch.int64, device=device)
    b = torch.minimum(i + 1, n - i)
    return b * b


def _expected_chunk(Dfree, filled, D_filled, table, vb_terms):
    """Signed float32 field of one chunk from the squared distances of free voxels (to the nearest filled one) and of
    filled voxels (to the nearest free one); vb_terms: broadcastable per-axis squared border distances."""
    import torch
    D = torch.where(filled, D_filled, Dfree)
    for t in vb_terms:
        if t is not None:
            D = torch.minimum(D, t)
    v = table[D]
    return torch.where(filled, -v, v), D


class _Extrema:
    def __init__(self):
        self.free, self.filled = -1, -1

    def add(self, D, filled):
        import torch
        if bool((~filled).any()):
            self.free = max(self.free, int(torch.where(filled, torch.zeros_like(D), D).max()))
        if bool(filled.any()):
            self.filled = max(self.filled, int(torch.where(filled, D, torch.zeros_like(D)).max()))

    def value(self, res):
        mx = math.sqrt(self.free) * res if self.free >= 0 else -math.inf
        mn = 0.0 - math.sqrt(self.filled) * res if self.filled >= 0 else math.inf
        return mx, mn


def _used_device_bytes():
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free


def _sites_reference(shape, sites, inverse, res, sdf, chunk=128):
    """Compare a device field with the brute-force exact field of point sites (min over the sites in int64), in x chunks.
    inverse=False: the sites are the filled voxels; True: the sites are the only free voxels.  Returns the extrema."""
    import torch
    nx, ny, nz = shape
    dev = sdf.device
    dmax = max((max(nx - 1 - x, x) ** 2 + max(ny - 1 - y, y) ** 2 + max(nz - 1 - z, z) ** 2) for x, y, z in sites)
    table = torch.from_numpy(_finish_table(dmax, res)).to(dev)
    gy = torch.arange(ny, dtype=torch.int64, device=dev).view(1, ny, 1)
    gz = torch.arange(nz, dtype=torch.int64, device=dev).view(1, 1, nz)
    ext = _Extrema()
    for x0 in range(0, nx, chunk):
        x1 = min(nx, x0 + chunk)
        gx = torch.arange(x0, x1, dtype=torch.int64, device=dev).view(-1, 1, 1)
        D = None
        for sx, sy, sz in sites:
            d = (gx - sx) ** 2 + (gy - sy) ** 2 + (gz - sz) ** 2
            D = d if D is None else torch.minimum(D, d)
        site = D == 0
        filled = ~site if inverse else site
        one = torch.ones_like(D)
        # free voxels: distance to the nearest filled one; filled voxels: to the nearest free one (1 for an isolated site)
        want, Dc = _expected_chunk(one if inverse else D, filled, D if inverse else one, table, [])
        got = sdf[x0:x1]
        if not bool(torch.equal(got.view(torch.int32), want.view(torch.int32))):
            bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()[:3].tolist()
            raise AssertionError("x chunk %d: %d voxels differ, first %s" % (
                x0, int((got.view(torch.int32) != want.view(torch.int32)).sum()), [[b[0] + x0] + b[1:] for b in bad]))
        ext.add(Dc, filled)
        del D, d, site, filled, want, Dc, got
    return ext.value(res)


def _sites_mask(shape, sites, inverse, device):
    import torch
    m = torch.full(shape, 1 if inverse else 0, dtype=torch.uint8, device=device)
    for s in sites:
        m[s] = 0 if inverse else 1
    return m


def test_sites_closed_form_matches_the_oracle():
    import torch
    shape, res = (13, 11, 14), 0.01
    for sites in ([(0, 0, 0)], [(0, 0, 0), (12, 10, 13), (6, 5, 7), (0, 5, 2), (12, 5, 2)]):
        for inverse in (False, True):
            m = _sites_mask(shape, sites, inverse, "cpu").numpy()
            ex, ex_ext, _ = O.exact_sdf(m, res)
            t = torch.from_numpy(ex)
            assert _sites_reference(shape, sites, inverse, res, t, chunk=5) == ex_ext, (sites, inverse)
            t[3, 4, 5] = -t[3, 4, 5]
            with pytest.raises(AssertionError):                       # (and the comparison does compare)
                _sites_reference(shape, sites, inverse, res, t, chunk=5)


@pytest.fixture(scope="module")
def big():
    """A context of its own for the largest grids: its scratch fields go when the module ends."""
    import torch
    ctx = capi.SdfGpu(0)
    ctx.set_option("dense_retry", 0)
    yield ctx
    ctx.close()
    torch.cuda.empty_cache()


# ---- 2. 1024^3 at its edge ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", [1024, 1025])
def test_1024_cube_at_the_key_limit(big, nz):
    """(1024, 1024, 1024) is 2040 below the key bound, (1024, 1024, 1025) one plane past it.  Point sites and their inverses,
    device-resident, against the brute-force minimum over the sites; far-field on the first, marching sweeps on the second."""
    import torch
    shape, res = (1024, 1024, nz), 0.01
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    inside = nz == 1024
    assert far_ok(shape) == inside
    c = (1023, 1023, nz - 1)
    corners = [(x, y, z) for x in (0, c[0]) for y in (0, c[1]) for z in (0, c[2])]
    site_sets = {"corner": [(0, 0, 0)], "8 corners": corners,
                 "interior + line": [(511, 300, 700), (0, 512, 5), (1023, 512, 5), (1023, 0, nz - 1)]}
    base = _used_device_bytes()
    peak = 0
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    times = []
    for name, sites in site_sets.items():
        for inverse in (False, True):
            m_t = _sites_mask(shape, sites, inverse, dev)
            big.set_option("policy_reset", 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            big.build_device(m_t.data_ptr(), shape, out.data_ptr(), res, False, stream)
            torch.cuda.synchronize()
            times.append((name + (" inverse" if inverse else ""), time.perf_counter() - t0))
            peak = max(peak, _used_device_bytes() - base)
            ext = big.get_extrema()
            path = big.last_path()
            del m_t
            want_ext = _sites_reference(shape, sites, inverse, res, out)
            assert ext == want_ext, (name, inverse, ext, want_ext)
            if inside:
                assert path["far_y"] and path["far_x"], (name, inverse, path)
            else:
                assert not path["far_y"] and not path["far_x"], (name, inverse, path)
    del out
    torch.cuda.empty_cache()
    print("\n[size-limits] %s build times (s): %s; device memory in use %.2f GB" % (
        "x".join(map(str, shape)), ", ".join("%s %.3f" % t for t in times), peak / 1e9))


# ---- 3. long lines, the largest extents, the size refusal -----------------------------------------------------------------------
LONG_SHAPES = [(16384, 2, 3), (3, 16384, 2), (2, 3, 16384), (1025, 4, 16), (4, 2049, 32), (8, 8, 4096), (2048, 3, 8),
               (3, 1025, 40), (4096, 5, 3), (1, 1, 16384)]


@pytest.mark.parametrize("shape", LONG_SHAPES, ids=["x".join(map(str, s)) for s in LONG_SHAPES])
def test_long_lines_are_exact(gpu, shape):
    """Lines of 1025 .. 16384 voxels (marching sweeps with unbounded scans, int16 z distances up to 16383, the 16-bit plane
    field with its side table saturated): host and device entry points against the oracle, virtual border off and on."""
    import torch
    res = 0.05
    sc = edge_scenes(shape, sum(shape), int(np.argmax(shape)))
    jobs = [(m, res, vb) for m in sc.values() for vb in (False, True)]
    want = dict(zip([(n, vb) for n in sc for vb in (False, True)], _oracles(jobs)))
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    may_far = far_ok(shape)
    for name, m in sc.items():
        m_t = torch.from_numpy(m).cuda()
        for vb in (False, True):
            ex, ex_ext, _ = want[(name, vb)]
            tag = "%s %s vb=%d" % (shape, name, vb)
            sdf, ext = gpu.build(m, res, vb)
            _assert_bits(tag + " host", sdf, ex)
            assert ext == ex_ext, (tag, ext, ex_ext)
            if not may_far:
                p = gpu.last_path()
                assert not p["far_y"] and not p["far_x"], (tag, p)
            gpu.build_device(m_t.data_ptr(), shape, out.data_ptr(), res, vb, stream)
            torch.cuda.synchronize()
            _assert_bits(tag + " device", out.cpu().numpy(), ex)
            assert gpu.get_extrema() == ex_ext, tag


def test_size_refusal_then_exact(gpu):
    """A dimension of 16385 is refused with SDFGPU_ERR_UNSUPPORTED_SIZE (-3) through the host and the device entry points; the
    context builds exactly afterwards."""
    import torch
    from sdf_tools_amd.capi import SdfGpuError
    for shape in ((16385, 1, 1), (1, 16385, 1), (1, 1, 16385), (2, 16385, 2)):
        m = np.zeros(shape, np.uint8)
        m[0, 0, 0] = 1
        with pytest.raises(SdfGpuError) as ei:
            gpu.build(m, 0.05)
        assert ei.value.code == -3, (shape, ei.value.code)
        m_t = torch.from_numpy(m).cuda()
        out = torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(SdfGpuError) as ei:
            gpu.build_device(m_t.data_ptr(), shape, out.data_ptr(), 0.05, False, torch.cuda.current_stream().cuda_stream)
        assert ei.value.code == -3, (shape, ei.value.code)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())                                   # nothing written
    m = synth.bernoulli_mask((16384, 2, 2), 0.01, 5)
    ex, ex_ext, _ = O.exact_sdf(m, 0.05, True)
    sdf, ext = gpu.build(m, 0.05, True)
    _assert_bits("after the refusal", sdf, ex)
    assert ext == ex_ext


# ---- 4. past 2^31 voxels -------------------------------------------------------------------------------------------------------
BIG = (3072, 1024, 1024)
STRIDES = (5, 7, 11)


def _lattice_axis_dist(n, s, lo, hi, device):
    """Distance from i in [lo, hi) to the nearest multiple of s in [0, n)."""
    import torch
    i = torch.arange(lo, hi, dtype=torch.int64, device=device)
    last = ((n - 1) // s) * s
    r = i % s
    d = torch.minimum(r, s - r)
    return torch.where(i > last, i - last, d)


def _lattice_check(shape, inverse, vb, res, sdf, chunk=128):
    """Point lattice with strides STRIDES (filled iff every coordinate is a multiple of its stride): the exact d^2 of a
    non-lattice voxel is the sum of the per-axis squared distances to the nearest lattice coordinate; a lattice voxel is 1 from
    the other class.  inverse: the lattice voxels are the free ones.  Compared in x chunks; returns the extrema."""
    import torch
    nx, ny, nz = shape
    dev = sdf.device
    dy = _lattice_axis_dist(ny, STRIDES[1], 0, ny, dev).view(1, ny, 1)
    dz = _lattice_axis_dist(nz, STRIDES[2], 0, nz, dev).view(1, 1, nz)
    vby = _vb_sq(ny, 0, ny, dev) if vb else None
    vbz = _vb_sq(nz, 0, nz, dev) if vb else None
    dmax = sum(int(_lattice_axis_dist(n, s, 0, n, "cpu").max()) ** 2 for n, s in zip(shape, STRIDES))
    table = torch.from_numpy(_finish_table(dmax, res)).to(dev)
    ext = _Extrema()
    for x0 in range(0, nx, chunk):
        x1 = min(nx, x0 + chunk)
        dx = _lattice_axis_dist(nx, STRIDES[0], x0, x1, dev).view(-1, 1, 1)
        D = dx * dx + dy * dy + dz * dz
        lattice = D == 0
        filled = ~lattice if inverse else lattice
        one = torch.ones_like(D)
        vbx = _vb_sq(nx, x0, x1, dev) if vb else None
        terms = [t.view(*v) for t, v in ((vbx, (-1, 1, 1)), (vby, (1, -1, 1)), (vbz, (1, 1, -1))) if t is not None]
        want, Dc = _expected_chunk(one if inverse else D, filled, D if inverse else one, table, terms)
        got = sdf[x0:x1]
        eq = got.view(torch.int32) == want.view(torch.int32)
        if not bool(eq.all()):
            bad = (~eq).nonzero()[:3].tolist()
            raise AssertionError("x chunk %d: %d voxels differ, first %s" % (x0, int((~eq).sum()), [[b[0] + x0] + b[1:] for b in bad]))
        ext.add(Dc, filled)
        del D, lattice, filled, one, want, Dc, got, eq
    return ext.value(res)


def _lattice_mask(shape, inverse, device, chunk=256):
    import torch
    nx, ny, nz = shape
    m = torch.empty(shape, dtype=torch.uint8, device=device)
    ly = (torch.arange(ny, device=device) % STRIDES[1] == 0).view(1, ny, 1)
    lz = (torch.arange(nz, device=device) % STRIDES[2] == 0).view(1, 1, nz)
    for x0 in range(0, nx, chunk):
        x1 = min(nx, x0 + chunk)
        lx = (torch.arange(x0, x1, device=device) % STRIDES[0] == 0).view(-1, 1, 1)
        lat = lx & ly & lz
        m[x0:x1] = (~lat if inverse else lat).to(torch.uint8)
    return m


def test_lattice_closed_form_matches_the_oracle():
    import torch
    res = 0.01
    for shape in ((23, 30, 40), (17, 9, 34), (1, 15, 23)):
        for inverse in (False, True):
            for vb in (False, True):
                m = _lattice_mask(shape, inverse, "cpu").numpy()
                ex, ex_ext, _ = O.exact_sdf(m, res, vb)
                t = torch.from_numpy(ex)
                assert _lattice_check(shape, inverse, vb, res, t, chunk=4) == ex_ext, (shape, inverse, vb)
                t[0, 1, 2] = t[0, 1, 2] * 2
                with pytest.raises(AssertionError):
                    _lattice_check(shape, inverse, vb, res, t, chunk=4)


def test_sdf_past_2_31_voxels(big):
    """3 * 2^30 voxels, device-resident (linear indices past 2^31 in every sweep, the pack, the dense tier, the finish and the
    extrema fold): the point lattice and its inverse against the closed form on every voxel; Bernoulli(0.5) through the
    dense tier (certified) against oracle crops at x = 0, across x = 2048 (linear index 2^31) and at the last planes, plus
    the properties of an exact signed EDT."""
    import torch
    shape, res = BIG, 0.01
    nx, ny, nz = shape
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.empty_cache()
    base = _used_device_bytes()
    peak = 0
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    times = []
    for inverse, vb in ((False, False), (True, True)):
        m_t = _lattice_mask(shape, inverse, dev)
        big.set_option("policy_reset", 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        big.build_device(m_t.data_ptr(), shape, out.data_ptr(), res, vb, stream)
        torch.cuda.synchronize()
        times.append(("lattice" + (" inverse vb" if inverse else ""), time.perf_counter() - t0))
        peak = max(peak, _used_device_bytes() - base)
        ext = big.get_extrema()
        path = big.last_path()
        assert not path["far_y"] and not path["far_x"], path
        del m_t
        want_ext = _lattice_check(shape, inverse, vb, res, out)
        assert ext == want_ext, (inverse, vb, ext, want_ext)
    # Bernoulli(0.5): the dense tier
    m_t = torch.empty(shape, dtype=torch.uint8, device=dev)
    for x0 in range(0, nx, 256):
        m_t[x0:x0 + 256] = synth.bernoulli_mask_torch(shape, 0.5, 11, x_range=(x0, min(nx, x0 + 256)), device=dev)
    big.set_option("policy_reset", 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    big.build_device(m_t.data_ptr(), shape, out.data_ptr(), res, False, stream)
    torch.cuda.synchronize()
    times.append(("bernoulli 0.5", time.perf_counter() - t0))
    peak = max(peak, _used_device_bytes() - base)
    ext = big.get_extrema()
    assert big.last_path()["dense_certified"]
    mx, mn = -math.inf, math.inf
    for x0 in range(0, nx, 128):
        s, mk = out[x0:x0 + 128], m_t[x0:x0 + 128]
        assert bool(torch.equal(s < 0, mk != 0)), x0                     # sign == occupancy
        a = s.abs()
        assert float(a.min()) >= res * (1 - 1e-6), x0
        d2 = (a.double() / res) ** 2
        assert float((d2 - d2.round()).abs().max()) < 1e-3, x0           # squared distances are integers
        mx, mn = max(mx, float(s.max())), min(mn, float(s.min()))
        del s, mk, a, d2
    assert ext[0] == pytest.approx(mx, abs=1e-6) and ext[1] == pytest.approx(mn, abs=1e-6)
    maxd = int(round(max(ext[0], -ext[1]) / res)) + 2
    C = 40
    rng = np.random.default_rng(5)
    corners = [[0, 0, 0], [2048 - C // 2, int(rng.integers(0, ny - C)), int(rng.integers(0, nz - C))], [2047 - C, ny - C, 0],
               [2048, 0, nz - C], [nx - C, ny - C, nz - C], [nx - C, 0, int(rng.integers(0, nz - C))]]
    for lo in corners:
        a = [max(0, v - maxd) for v in lo]
        b = [min(n, v + C + maxd) for v, n in zip(lo, shape)]
        sub = m_t[a[0]:b[0], a[1]:b[1], a[2]:b[2]].cpu().numpy()
        want, _, _ = O.exact_sdf(sub, res)
        off = [v - aa for v, aa in zip(lo, a)]
        w = want[off[0]:off[0] + C, off[1]:off[1] + C, off[2]:off[2] + C]
        g = out[lo[0]:lo[0] + C, lo[1]:lo[1] + C, lo[2]:lo[2] + C].cpu().numpy()
        _assert_bits("crop at %s" % lo, g, w)
    del out, m_t
    torch.cuda.empty_cache()
    print("\n[size-limits] %s build times (s): %s; device memory in use %.2f GB" % (
        "x".join(map(str, shape)), ", ".join("%s %.3f" % t for t in times), peak / 1e9))


def _even_lattice_labels(shape, x0, x1, device):
    """Closed form of the labels when a voxel is filled iff x, y and z are all even: every filled voxel is a component of its
    own, numbered by scan order (x -> y -> z); the origin is component 1, the one free component (which starts at (0, 0, 1))
    is 2, and the lattice voxel of 0-based rank r > 0 among the lattice voxels is r + 2."""
    import torch
    nx, ny, nz = shape
    hy, hz = (ny + 1) // 2, (nz + 1) // 2
    x = torch.arange(x0, x1, dtype=torch.int64, device=device).view(-1, 1, 1)
    y = torch.arange(ny, dtype=torch.int64, device=device).view(1, ny, 1)
    z = torch.arange(nz, dtype=torch.int64, device=device).view(1, 1, nz)
    lat = ((x % 2) == 0) & ((y % 2) == 0) & ((z % 2) == 0)
    rank = (x // 2) * (hy * hz) + (y // 2) * hz + (z // 2)
    return torch.where(lat, torch.where(rank == 0, torch.ones_like(rank), rank + 2), torch.full_like(rank, 2))


def _even_lattice_bits(shape, device):
    """The bit field of the all-even lattice, built on the device (nz a multiple of 32: every word holds 32 voxels of one row)."""
    import torch
    nx, ny, nz = shape
    assert nz % 32 == 0
    w = torch.zeros((nx, ny, nz // 32), dtype=torch.int32, device=device)
    w[0::2, 0::2, :] = 0x55555555
    return w


def test_even_lattice_labels_closed_form():
    from test_components_cpu import restated_labels
    shape = (6, 4, 128)
    x, y, z = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    m = ((x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0)).astype(np.uint8)
    ref, k = restated_labels(m)
    assert k == (3 * 2 * 64) + 1
    assert np.array_equal(_even_lattice_labels(shape, 0, 6, "cpu").numpy(), ref.astype(np.int64))
    assert np.array_equal(_even_lattice_bits(shape, "cpu").numpy().view(np.uint32).reshape(-1), capi.pack_bits_host(m))
    for odd in ((5, 3, 7), (1, 3, 9)):                                 # the numbering on odd extents too
        x, y, z = np.meshgrid(*(np.arange(n) for n in odd), indexing="ij")
        mo = ((x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0)).astype(np.uint8)
        ro, _ = restated_labels(mo)
        assert np.array_equal(_even_lattice_labels(odd, 0, odd[0], "cpu").numpy(), ro.astype(np.int64)), odd


def test_components_past_2_31_voxels(big):
    """Connected components of 3 * 2^30 voxels through sdfgpu_components_bits_device: filled iff x, y and z are all even, so
    3 * 2^27 singleton components plus the free one; every label against the closed form (labels past index 2^31 included)."""
    import torch
    shape = BIG
    nx, ny, nz = shape
    dev = torch.device("cuda", 0)
    torch.cuda.empty_cache()
    base = _used_device_bytes()
    bits = _even_lattice_bits(shape, dev)
    labels = torch.full((nx, ny, nz), -1, dtype=torch.int32, device=dev)
    t0 = time.perf_counter()
    k = big.components_bits_device(bits.data_ptr(), shape, labels.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    peak = _used_device_bytes() - base
    assert k == 3 * 2 ** 27 + 1, k
    for x0 in range(0, nx, 128):
        x1 = min(nx, x0 + 128)
        want = _even_lattice_labels(shape, x0, x1, dev)
        got = labels[x0:x1].to(torch.int64) & 0xFFFFFFFF
        eq = got == want
        if not bool(eq.all()):
            bad = (~eq).nonzero()[:3].tolist()
            raise AssertionError("x chunk %d: %d labels differ, first %s got %s" % (
                x0, int((~eq).sum()), [[b[0] + x0] + b[1:] for b in bad], [int(got[tuple(b)]) for b in bad]))
        del want, got, eq
    del bits, labels
    torch.cuda.empty_cache()
    print("\n[size-limits] components %s: %.3f s, K = %d; device memory in use %.2f GB" % ("x".join(map(str, shape)), dt, k, peak / 1e9))


# ---- 5. component topology past 2^31 node ids and 2^32 vertices ------------------------------------------------------------------
def _layer_labels(shape, device):
    """Labels z // 2 (the slabs of a grid filled iff z mod 4 < 2, two voxels thick, alternately filled and free)."""
    import torch
    nx, ny, nz = shape
    lz = (torch.arange(nz, dtype=torch.int32, device=device) // 2).view(1, 1, nz)
    return lz.expand(nx, ny, nz).contiguous()


def _layer_counts(shape):
    """Closed form of the counters of _layer_labels (nz a multiple of 4): every label is a slab spanning x and y with another label
    (or the outside) on each side -- nodes at its two z faces and at the x / y rim of its middle vertex plane; M3 = its 8 corners;
    every other node has 4 exposed edges; one surface."""
    nx, ny, nz = shape
    assert nz % 4 == 0
    per = [2 * (nx + 1) * (ny + 1) + 2 * (nx + ny), 8, 0, 0, 1]
    return np.array([per] * (nz // 2), np.int64)


def _box_counts(shape):
    """Closed form of the counters of one label over the whole grid (label 1; row 0 empty): the boundary vertices, 8 corners."""
    nx, ny, nz = shape
    nodes = (nx + 1) * (ny + 1) * (nz + 1) - (nx - 1) * (ny - 1) * (nz - 1)
    return np.array([[0] * 5, [nodes, 8, 0, 0, 1]], np.int64)


def _even_lattice_nodes(shape):
    """Closed form of the surface-vertex nodes of _even_lattice_labels: 8 per lattice voxel (each is a component of its own), and
    one of the free component at every vertex except those whose in-grid cube is a lone lattice voxel (a corner of the vertex grid
    on each axis that starts or, for an odd extent, ends with a lattice coordinate)."""
    lattice = math.prod((n + 1) // 2 for n in shape)
    lone = math.prod(1 + n % 2 for n in shape)
    return 8 * lattice + math.prod(n + 1 for n in shape) - lone


def _numpy_nodes(labels):
    """Node count by the header's definition, independent of both restatements: (vertex, c) is a node iff the vertex's cube holds
    a voxel of c with a face neighbour inside the cube whose label is not c (the outside is -1)."""
    lab = np.pad(np.asarray(labels, np.int64), 1, constant_values=-1)
    nx, ny, nz = labels.shape
    cube = [lab[dx:dx + nx + 1, dy:dy + ny + 1, dz:dz + nz + 1] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
    surface = []
    for s in range(8):
        nb = [cube[s ^ b] for b in (1, 2, 4)]
        surface.append((cube[s] >= 0) & ((nb[0] != cube[s]) | (nb[1] != cube[s]) | (nb[2] != cube[s])))
    total = 0
    for s in range(8):
        first = surface[s].copy()
        for t in range(s):
            first &= ~(surface[t] & (cube[t] == cube[s]))
        total += int(first.sum())
    return total


def _tp_scratch_bytes(shape, max_label, select):
    """tp_plan's scratch_bytes (sdfgpu_topology.hip), restated."""
    nx, ny, nz = shape
    chunk, align8 = 8192, (lambda b: (b + 7) & ~7)
    nv = (nx + 1) * (ny + 1) * (nz + 1)
    chunks = (nv + chunk - 1) // chunk
    labels = max_label + 1
    off_flags = align8(labels * 5 * 8) + 24                               # counters | TpStatus (24 bytes)
    off_nm = align8(off_flags + (labels * 4 if select else 0))
    return off_nm + chunks * chunk + chunks * (chunk // 8) * 4 + chunks * 4 * 2


def test_topology_closed_forms_match_the_restatement():
    """The three closed forms on small grids of the same patterns (odd and even extents, thin ones): every counter against
    restated_counts, the node totals against a numpy count by the header's definition."""
    from test_topology_cpu import holes_voids, restated_counts
    for shape in ((5, 3, 8), (2, 7, 12), (1, 1, 4), (6, 4, 16), (3, 1, 8)):
        lab = _layer_labels(shape, "cpu").numpy().view(np.uint32)
        want = _layer_counts(shape)
        assert np.array_equal(restated_counts(lab, max_label=shape[2] // 2 - 1), want), shape
        assert _numpy_nodes(lab) == int(want[:, 0].sum()), shape
        assert holes_voids(want) == {c: (0, 0) for c in range(shape[2] // 2)}
    for shape in ((4, 8, 7), (1, 3, 4), (2, 2, 2), (4, 5, 6), (1, 1, 1)):
        lab = np.ones(shape, np.uint32)
        want = _box_counts(shape)
        assert np.array_equal(restated_counts(lab, max_label=1), want), shape
        assert _numpy_nodes(lab) == int(want[1, 0]), shape
        assert holes_voids(want) == {1: (0, 0)}
    for shape in ((6, 4, 8), (5, 3, 7), (4, 5, 2), (1, 3, 9), (7, 6, 5)):
        lab = _even_lattice_labels(shape, 0, shape[0], "cpu").numpy().astype(np.uint32)
        counts = restated_counts(lab)
        assert int(counts[:, 0].sum()) == _even_lattice_nodes(shape) == _numpy_nodes(lab), shape
    assert _even_lattice_nodes(BIG) == 8 * 3 * 2 ** 27 + 3073 * 1025 * 1025 - 1


def _counts_device(ctx, labels, shape, max_label, select=None):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = ctx.component_topology_device(labels.data_ptr(), shape, max_label, None if select is None else select.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    return got, time.perf_counter() - t0


def test_topology_refuses_more_than_2_32_nodes(big):
    """The all-even lattice at 3072 x 1024 x 1024 has about 6.4e9 surface-vertex nodes: refused with -1 after the counting pass,
    the count in the message equal to the closed form, the node buffer never allocated (device memory grows by the scratch at
    most).  The same handle then answers a small scene exactly."""
    import torch
    from test_components_cpu import restated_labels
    from test_topology_cpu import SHAPES, restated_counts
    from sdf_tools_amd.capi import SdfGpuError
    shape = BIG
    nx = shape[0]
    dev = torch.device("cuda", 0)
    torch.cuda.empty_cache()
    labels = torch.empty(shape, dtype=torch.int32, device=dev)
    for x0 in range(0, nx, 128):
        labels[x0:x0 + 128] = _even_lattice_labels(shape, x0, min(nx, x0 + 128), dev).to(torch.int32)
    max_label = 3 * 2 ** 27 + 1
    nodes = _even_lattice_nodes(shape)
    assert nodes > 2 ** 32 - 1
    scratch = _tp_scratch_bytes(shape, max_label, False)
    torch.cuda.synchronize()
    base = _used_device_bytes()
    t0 = time.perf_counter()
    with pytest.raises(SdfGpuError) as ei:
        big.component_topology_device(labels.data_ptr(), shape, max_label, None, torch.cuda.current_stream().cuda_stream)
    dt = time.perf_counter() - t0
    grew = _used_device_bytes() - base
    msg = str(ei.value)
    assert ei.value.code == -1, msg
    assert ("%d surface-vertex nodes" % nodes) in msg, (nodes, msg)
    assert grew <= scratch + (64 << 20), (grew, scratch, nodes * 4)
    del labels
    torch.cuda.empty_cache()
    m = SHAPES["cube_two_cavities"]()
    lab, k = restated_labels(m)
    d = torch.from_numpy(lab.astype(np.int32)).to(dev)
    got, _ = _counts_device(big, d, m.shape, k)
    assert np.array_equal(got, restated_counts(lab, max_label=k))
    print("\n[size-limits] topology refusal %s: %d nodes, %.3f s, device memory grew %.2f GB (scratch %.2f GB)" % (
        "x".join(map(str, shape)), nodes, dt, grew / 1e9, scratch / 1e9))


def test_topology_layers_past_2_31_node_ids(big):
    """3072 x 1024 x 1024 labelled z // 2: 512 slabs whose surfaces span the whole vertex range, about 3.23e9 nodes, so the
    union-find joins node ids above 2^31 with ids below it.  Every counter against the closed form; (holes, voids) = (0, 0)."""
    import torch
    from test_topology_cpu import holes_voids
    shape = BIG
    dev = torch.device("cuda", 0)
    torch.cuda.empty_cache()
    base = _used_device_bytes()
    labels = _layer_labels(shape, dev)
    want = _layer_counts(shape)
    nodes = int(want[:, 0].sum())
    assert 2 ** 31 < nodes < 2 ** 32 - 1, nodes
    got, dt = _counts_device(big, labels, shape, shape[2] // 2 - 1)
    peak = _used_device_bytes() - base
    assert np.array_equal(got, want), (got[:3], want[:3], np.argwhere(got != want)[:5])
    assert holes_voids(got) == {c: (0, 0) for c in range(shape[2] // 2)}
    del labels
    torch.cuda.empty_cache()
    print("\n[size-limits] topology layers %s: %d nodes, %.3f s; device memory in use %.2f GB" % (
        "x".join(map(str, shape)), nodes, dt, peak / 1e9))


def test_topology_one_box_past_2_32_vertices(big):
    """(4, 32768, 32767): n = 2^32 - 2^17 voxels, 5.37e9 vertices (the 64-bit branch of vertex_of, vertex ids past 2^32), one
    label from the components of an all-filled bit field (K = 1) and 2,147,942,394 nodes on one surface.  Without a selection
    and with an all-ones one: the same counters, equal to the closed form."""
    import torch
    from test_topology_cpu import holes_voids
    shape = (4, 32768, 32767)
    n = math.prod(shape)
    assert n == 2 ** 32 - 2 ** 17 and math.prod(s + 1 for s in shape) > 2 ** 32
    dev = torch.device("cuda", 0)
    torch.cuda.empty_cache()
    base = _used_device_bytes()
    bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)
    labels = torch.zeros(n, dtype=torch.int32, device=dev)
    t0 = time.perf_counter()
    k = big.components_bits_device(bits.data_ptr(), shape, labels.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    t_cc = time.perf_counter() - t0
    assert k == 1, k
    assert bool((labels == 1).all())
    want = _box_counts(shape)
    assert int(want[1, 0]) == 2147942394
    got, t_all = _counts_device(big, labels, shape, 1)
    assert np.array_equal(got, want), (got, want)
    sel, t_sel = _counts_device(big, labels, shape, 1, bits)
    assert np.array_equal(sel, got), (sel, got)
    assert holes_voids(got) == {1: (0, 0)}
    peak = _used_device_bytes() - base
    del bits, labels
    torch.cuda.empty_cache()
    print("\n[size-limits] topology box %s: components %.3f s; %d nodes, %.3f s, selected %.3f s; device memory in use %.2f GB" % (
        "x".join(map(str, shape)), t_cc, int(want[1, 0]), t_all, t_sel, peak / 1e9))


# ---- 6. local extrema at the largest grid check_convex_args accepts -----------------------------------------------------------------
CX_BIG = (9241, 464773, 1)                 # n = 2^32 - 3; index 2^31 is (4620, 232388, 0)
CX_RAMP = (4620, 4100, 1101)               # (split, left, right) of cx_profile


def cx_profile(nx, split, left, right):
    """An x profile (integers >= 0, exact in float32): blocks 0 1 1 0 from x = 0 up to a = split - left, each block a 2-cycle
    entered from its first voxel; a ramp rising over `left` steps from a to the 2-cycle {split - 1, split}; a ramp falling over
    `right` steps after it; blocks 0 1 1 0 anchored at the last x, so that the last plane steps to x - 1 into its block's 2-cycle."""
    a, b = split - left, split + right
    assert a % 4 == 0 and (nx - 1 - b) % 4 == 3 and right <= left
    x = np.arange(nx)
    blk = np.array([0, 1, 1, 0])
    f = np.empty(nx, np.int64)
    f[:a] = blk[x[:a] % 4]
    f[a:split] = left + 1 - (split - 1 - x[a:split])
    f[split:b] = left + 1 - (x[split:b] - split)
    f[b:] = blk[(nx - 1 - x[b:]) % 4]
    return f.astype(np.float32)


def _profile_next(f):
    """next() along x of a field that depends on x alone: the sign of f(x + 1) - f(x - 1), one-sided at both ends."""
    fi = f.astype(np.int64)
    nx = len(f)
    out = []
    for x in range(nx):
        d = fi[min(nx - 1, x + 1)] - fi[max(0, x - 1)]
        out.append(x + 1 if d > 0 else (x - 1 if d < 0 else x))
    return out


def _cx_scratch_bytes(n):
    """cx_plan's scratch_bytes (sdfgpu_convex.hip), restated: A, B (u64), next (u32), CxStats, root bits, word ranks, chunk
    counts and offsets."""
    chunks = (n + 8191) // 8192
    stats = (40 * 64 * 32 + 64 * 32 + 3 * 32) * 4
    off_stats = (20 * n + 7) & ~7
    return off_stats + ((stats + 7) & ~7) + 2 * chunks * 256 * 4 + 2 * chunks * 4


def cx_profile_walk(f):
    """The literal walk along the profile (every step an integer difference of at least 1, far above the step threshold at
    res = 1) and, per cycle, the steps from its basin minimum to its entry: (extremum x or -1 per x, cycles, longest entry walk)."""
    from test_convex_segments_cpu import literal_walk
    nx = len(f)
    nxt = _profile_next(f)
    E = literal_walk(nxt)
    cycles, longest = 0, 0
    for x in range(nx):
        if nxt[x] != x and nxt[nxt[x]] == x and x < nxt[x]:
            cycles += 1
            b = min(u for u in range(nx) if E[u] in (x, nxt[x]))
            steps, u = 0, b
            while u not in (x, nxt[x]):
                u, steps = nxt[u], steps + 1
            longest = max(longest, steps)
    return np.array(E, np.int64), cycles, longest


def cx_expected(E, ny, x0, x1, device):
    """Closed form of the extremum indices of x planes [x0, x1): E[x] ny + y (int64; every walk stays in its row)."""
    import torch
    e = torch.as_tensor(E[x0:x1], device=device).view(-1, 1)
    return torch.where(e < 0, torch.full_like(e, 0xFFFFFFFF), e * ny + torch.arange(ny, dtype=torch.int64, device=device).view(1, -1))


def test_extrema_profile_closed_form_matches_the_restatement():
    """The profile's closed form on small grids whose x pattern matches CX_BIG's at both ends (blocks from x = 0, the two ramps,
    blocks ending at the last plane): the extremum locations against restated_extrema, the cycles and the longest entry walk
    against the walk of the grid's own next()."""
    from test_convex_segments_cpu import _cycles, cx_max_accepted_n, literal_walk, next_map, restated_extrema
    assert math.prod(CX_BIG) == cx_max_accepted_n(32) == 2 ** 32 - 3
    assert 4620 * CX_BIG[1] + 232388 == 2 ** 31
    for nx, ny, ramp in ((37, 5, (24, 12, 9)), (45, 3, (24, 12, 9)), (41, 1, (20, 12, 9)), (61, 4, (32, 16, 13))):
        f = cx_profile(nx, *ramp)
        field = np.broadcast_to(f.reshape(nx, 1, 1), (nx, ny, 1)).copy()
        E, cycles, longest = cx_profile_walk(f)
        idx = cx_expected(E, ny, 0, nx, "cpu").numpy().reshape(nx, ny, 1)
        got = restated_extrema(field, 1.0)
        assert np.array_equal(capi.extremum_locations(idx.astype(np.uint32), field.shape, 1.0), got), (nx, ny, ramp)
        nxt = next_map(field, 1.0)
        assert nxt[-1] == (nx - 2) * ny + ny - 1                            # the last voxel steps to x - 1
        assert len(_cycles(nxt)) == cycles * ny == (ramp[0] - ramp[1]) // 4 * ny + (nx - ramp[0] - ramp[2]) // 4 * ny + ny
        assert longest == ramp[1]
        assert np.array_equal(np.array(literal_walk(nxt)).reshape(nx, ny, 1), idx)
    f = cx_profile(CX_BIG[0], *CX_RAMP)
    assert f.min() >= 0 and f.max() < 2 ** 24
    E, cycles, longest = cx_profile_walk(f)
    ny = CX_BIG[1]
    assert E[4620] == E[4617] == 4619 and E[519] == 4619 and E[4620 + 1100] == 4619        # one basin across index 2^31
    assert E[-1] == CX_BIG[0] - 3 and E[-1] * ny + ny - 1 < 2 ** 32 - 3
    assert cycles == 1011 and longest == 4100


def test_extrema_at_the_largest_accepted_grid(big):
    """n = 2^32 - 3, the largest grid check_convex_args accepts: the last index, 2^32 - 4, is one below kOnCycle, and the last voxel
    steps inward.  A basin of 5202 x planes around index 2^31 (entered at x = 4619 from its minimum at x = 519; a signed minimum
    would pick x = 4620 or 4621 and enter at x = 4620), reached over up to 4100 steps (at least 10 doubling rounds whose windows
    span both sides), blocks with 2-cycles elsewhere.  Past n = 2^32 - 256 a 1-D launch of one lane per voxel would need 2^32
    work-items, which the runtime refuses: the kernels' 2-D grid is exercised here too.  All 4.29e9 extremum indices against the
    closed form, bit for bit, and the doubling statistics."""
    import torch
    from test_convex_segments_cpu import word_model
    shape, res = CX_BIG, 1.0
    nx, ny, _ = shape
    n = math.prod(shape)
    f = cx_profile(nx, *CX_RAMP)
    E, cycles, longest = cx_profile_walk(f)
    dev = torch.device("cuda", 0)
    torch.cuda.empty_cache()
    need = 8 * n + _cx_scratch_bytes(n) + (4 << 30)                        # field, indices, scratch, the comparison's chunks
    free, _ = torch.cuda.mem_get_info()
    assert free >= need, "local extrema at 2^32 - 3 voxels needs about %.1f GB of device memory, %.1f GB are free" % (need / 1e9, free / 1e9)
    base = _used_device_bytes()
    field = torch.empty(shape, dtype=torch.float32, device=dev)
    ft = torch.from_numpy(f).to(dev)
    for x0 in range(0, nx, 512):
        field[x0:x0 + 512] = ft[x0:x0 + 512].view(-1, 1, 1).expand(-1, ny, 1)
    ext = torch.empty(shape, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    big.local_extrema_device(field.data_ptr(), shape, res, ext.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    peak = _used_device_bytes() - base
    info = big.convex_last_info()
    del field
    for x0 in range(0, nx, 128):
        x1 = min(nx, x0 + 128)
        want = cx_expected(E, ny, x0, x1, dev)
        got = ext[x0:x1, :, 0].to(torch.int64) & 0xFFFFFFFF
        eq = got == want
        if not bool(eq.all()):
            bad = (~eq).nonzero()[:3].tolist()
            raise AssertionError("x chunk %d: %d extrema differ, first %s got %s want %s" % (
                x0, int((~eq).sum()), [[b[0] + x0, b[1]] for b in bad], [int(got[tuple(b)]) for b in bad],
                [int(want[tuple(b)]) for b in bad]))
        del want, got, eq
    del ext
    torch.cuda.empty_cache()
    line_rounds = word_model([int(v) for v in _profile_next(f)], 32)[1]
    assert info["cycles"] == cycles * ny, (info, cycles * ny)
    assert info["longest_cycle"] == 2 and info["longest_entry"] == longest, info
    assert 10 <= info["rounds"] <= math.ceil(math.log2(n)) + 1, info
    print("\n[size-limits] extrema %s (n = 2^32 - 3): %.3f s, %d rounds (one row alone in the word model: %d), %d cycles, "
          "longest entry %d; device memory in use %.2f GB" % ("x".join(map(str, shape)), dt, info["rounds"], line_rounds,
                                                               info["cycles"], info["longest_entry"], peak / 1e9))

