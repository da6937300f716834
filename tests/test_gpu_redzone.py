"""GPU: red zones (round 6, VERDICT r5 "next round" 2).  With option "redzone" (or SDFGPU_REDZONE=1 at sdfgpu_create) every device
allocation of the library carries canaries and every entry point ends with a check: a store outside a buffer fails the call
that made it and names the buffer.  The whole `-m gpu` suite and the fuzz are also run with SDFGPU_REDZONE=1 (a script removed
after commit 4eb6a2c, tools/r06_redzone.sh; its log is profiles/r06_redzone_suite_and_fuzz.txt)."""
import numpy as np
import pytest

from oracle import oracle as O
from sdf_tools_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture
def rz():
    ctx = capi.SdfGpu(0)
    ctx.set_option("redzone", 1)
    yield ctx
    ctx.close()


def test_a_store_behind_a_buffer_fails_the_call_and_names_the_buffer(rz):
    shape, res = (40, 48, 64), 0.01
    n = int(np.prod(shape))
    m = synth.bernoulli_mask(shape, 0.5, 1)
    d_in = rz.device_malloc(n)
    rz.copy_from_host(d_in, m)
    short = rz.device_malloc(n * 4 - 256)               # 64 floats too small: the build's last stores land in the canary
    with pytest.raises(capi.SdfGpuError) as e:
        rz.build_device(d_in, shape, short, res, False, 0)
    assert e.value.code == -6 and "sdfgpu_device_malloc" in str(e.value) and "BEHIND its end" in str(e.value) and "256 canary bytes" in str(e.value)
    rz.redzone_check()                                  # (the zone was repaired: the next look is clean)
    good = rz.device_malloc(n * 4)
    for opts in ({}, {"dense": 0}, {"dense": 0, "envelope_mode": 1}):
        rz.set_option("policy_reset", 1)
        for k, v in opts.items():
            rz.set_option(k, v)
        rz.build_device(d_in, shape, good, res, False, 0)
        got = rz.copy_to_host(np.empty(shape, np.float32), good)
        ex, ex_ext, _ = O.exact_sdf(m, res)
        assert np.array_equal(got, ex) and rz.get_extrema() == ex_ext
        rz.set_option("dense", 1)
        rz.set_option("envelope_mode", 0)
    for p in (d_in, short, good):
        rz.device_free(p)


@pytest.mark.parametrize("shape", [(25, 20, 15), (9, 13, 64), (64, 64, 64), (21, 5, 512), (520, 3, 16), (2, 777, 32), (33, 17, 96)], ids=lambda s: "x".join(map(str, s)))
def test_every_tier_and_entry_point_is_clean_under_red_zones(rz, shape):
    """the reference's own demo grid (25 x 20 x 15, scripts/3d_sdf_demo_rviz.py:107-111 -- the shape whose x sweep stored past the field
    for three rounds), shapes 1 .. 6 mod 8, long lines, dense shapes: every tier forced in turn, with and without the virtual border,
    host builds, bits in, tagged cells, gradient, queries -- exact results and no canary touched."""
    res = 0.02
    n = int(np.prod(shape))
    for p in (0.5, 0.03, 0.002):
        m = synth.bernoulli_mask(shape, p, 4)
        for vb in (False, True):
            ex, ex_ext, _ = O.exact_sdf(m, res, vb)
            d_in, d_out = rz.device_malloc(n), rz.device_malloc(n * 4)
            rz.copy_from_host(d_in, m)
            for opts in ({}, {"dense": 0}, {"dense": 0, "envelope_mode": 1}, {"dense": 0, "plane16": 0}, {"expect_dense": 1}, {"far_predict": 2, "dense": 0},
                         {"dense3_mode": 1}, {"fixup_mode": 1}):
                rz.set_option("policy_reset", 1)
                for k, v in opts.items():
                    rz.set_option(k, v)
                rz.build_device(d_in, shape, d_out, res, vb, 0)
                ext = rz.get_extrema()
                got = rz.copy_to_host(np.empty(shape, np.float32), d_out)
                for k in opts:
                    rz.set_option(k, {"dense": 1, "envelope_mode": 0, "plane16": 1, "expect_dense": 0, "far_predict": 1, "dense3_mode": 0, "fixup_mode": 0}[k])
                assert np.array_equal(got, ex) and ext == ex_ext, (p, vb, opts)
            rz.device_free(d_in)
            got, ext = rz.build(m, res, vb)
            assert np.array_equal(got, ex) and ext == ex_ext
            got, ext = rz.build_bits(capi.pack_bits_host(m), shape, res, vb)
            assert np.array_equal(got, ex) and ext == ex_ext
            if not vb:
                d_g = rz.device_malloc(n * 12)
                rz.gradient_device(d_out, shape, d_g, res, True, False, 0)
                pts = np.random.default_rng(0).random((300, 3)) * (np.asarray(shape) * res)
                rz.query_points(d_out, shape, res, pts, enable_edge_gradients=True)
                rz.device_free(d_g)
            rz.device_free(d_out)
    cells = np.zeros(shape + (4,), np.float32)
    cells[..., 0] = synth.bernoulli_mask(shape, 0.3, 9)
    cells.view(np.uint32)[..., 2] = 3
    got, ext = rz.build_tagged_cells(cells, shape, 1, (), False, res)
    ex, ex_ext, _ = O.exact_sdf(cells[..., 0] > 0.5, res)
    assert np.array_equal(got, ex) and ext == ex_ext


def _analysis_scratch_bytes(shape, max_label):
    """What components_bits_device, component_topology_device (no selection), component_surfaces_device and local_extrema_device
    plan for a grid, by the formulas of cc_plan, tp_plan, sf_plan and cx_plan (the scratch_bytes each hands to the handle).  The
    topology's node words and the surfaces' sort scratch depend on the scene and come on top."""
    nx, ny, nz = shape
    n, labels = nx * ny * nz, max_label + 1
    align8 = lambda v: (v + 7) & ~7
    # cc_plan: root bits | word ranks (256 words per chunk of 8192 voxels each) | chunk counts | chunk offsets | K and 3 spare words
    chunks = -(-n // 8192)
    cc = (2 * chunks * 256 + 2 * chunks + 4) * 4
    # tp_plan: counters u64 [labels][5] | status (24 bytes) | node bytes, one per vertex in chunks of 8192 | a u32 per 8 vertices
    # | chunk counts | chunk offsets
    chunks = -(-(nx + 1) * (ny + 1) * (nz + 1) // 8192)
    tp = align8(align8(labels * 5 * 8) + 24) + chunks * 8192 + chunks * 1024 * 4 + 2 * chunks * 4
    # sf_plan: counts u32 [labels] | status (16 bytes) | one surface bit per voxel in tiles of 4096
    sf = align8(align8(labels * 4) + 16) + -(-n // 4096) * 512
    # cx_plan: A u64 [n] | B u64 [n] | next u32 [n] | CxStats (40 rounds x 64 slots + 64 slots + 3 single slots, 32 words per slot)
    # | root bits | word ranks (256 words per chunk of 8192 each) | chunk counts | chunk offsets
    chunks = -(-n // 8192)
    cx = align8(20 * n) + align8((40 * 64 * 32 + 64 * 32 + 3 * 32) * 4) + 2 * chunks * 256 * 4 + 2 * chunks * 4
    return cc + tp + sf + cx


@pytest.fixture
def fresh():
    """A handle of its own, red zones off, that holds no scratch yet."""
    ctx = capi.SdfGpu(0)
    ctx.set_option("redzone", 0)
    yield ctx
    ctx.close()


def test_switching_red_zones_on_releases_the_analysis_scratch(fresh):
    """The analysis counterpart of test_gpu_batch_edges.py::test_switching_red_zones_on_releases_the_batch_scratch.  A handle that
    ran the component, topology, surface and extrema entry points before set_option("redzone", 1) must not keep their scratch
    without canaries: the switch releases it (the device's free memory rises by what the four calls planned at least),
    sdfgpu_convex_last_info asks for a new extrema call instead of reading statistics that went with the scratch, and the same
    four calls, on scratch with zones, give the same results and leave every canary alone.  Device forms on caller-owned buffers
    only: the host forms go through the staging buffers, which the switch has always released."""
    import torch
    side = 128                                          # the smallest cube with nz % 32 == 0 that plans 32 MiB (the amount the
    while _analysis_scratch_bytes((side,) * 3, 0) < (32 << 20):                          # batch test sees in mem_get_info)
        side += 32
    shape, n, res = (side,) * 3, side ** 3, 0.02
    ctx = fresh
    sizes = {"bits": (n + 31) // 32 * 4, "labels": n * 4, "indices": n * 4, "field": n * 4, "extrema": n * 4}
    d = {k: ctx.device_malloc(v) for k, v in sizes.items()}
    ctx.copy_from_host(d["bits"], capi.pack_bits_host(synth.bernoulli_mask(shape, 0.3, 21)))
    ctx.copy_from_host(d["field"], (np.random.default_rng(21).random(shape) * 2 - 1).astype(np.float32))

    def run():
        k = ctx.components_bits_device(d["bits"], shape, d["labels"])
        counters = ctx.component_topology_device(d["labels"], shape, k)
        counts, total = ctx.component_surfaces_device(d["labels"], shape, k, d_indices=d["indices"], capacity=n)
        ctx.local_extrema_device(d["field"], shape, res, d["extrema"])
        info = ctx.convex_last_info()
        torch.cuda.synchronize()
        return (k, ctx.copy_to_host(np.empty(n, np.uint32), d["labels"]), counters, counts, total,
                ctx.copy_to_host(np.empty(n, np.uint32), d["indices"])[:total], ctx.copy_to_host(np.empty(n, np.uint32), d["extrema"]), info)

    first = run()
    assert first[0] > 1 and first[4] > 0 and first[2][:, 4].sum() > 0       # components, reported voxels and surfaces: there was work
    planned = _analysis_scratch_bytes(shape, first[0])
    assert planned >= 32 << 20
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    ctx.set_option("redzone", 1)
    rise = torch.cuda.mem_get_info()[0] - free0
    print("planned %d bytes, free memory rose by %d" % (planned, rise))
    assert rise >= planned - (4 << 20)
    with pytest.raises(capi.SdfGpuError) as e:          # (its statistics lay in the scratch)
        ctx.convex_last_info()
    assert e.value.code == -1
    second = run()
    ctx.redzone_check()
    names = ("component count", "labels", "topology counters", "surface counts", "surface total", "surface indices", "extrema", "extrema info")
    for name, a, b in zip(names, first, second):
        if isinstance(a, np.ndarray):
            assert a.shape == b.shape, (name, a.shape, b.shape)
            differing = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
            assert differing.size == 0, (name, int(differing.size), differing[:4], a.reshape(-1)[differing[:4]], b.reshape(-1)[differing[:4]])
        else:
            assert a == b, (name, a, b)
    for p in d.values():
        ctx.device_free(p)


def test_multi_rank_builds_are_clean_under_red_zones(monkeypatch):
    """libsdfgpu_multi with 1 .. 4 logical ranks (contexts created with SDFGPU_REDZONE=1): slabs, bit planes, halos, the re-partition."""
    monkeypatch.setenv("SDFGPU_REDZONE", "1")
    shape, res = (37, 24, 64), 0.01
    for ranks in (1, 2, 3, 4):
        mg = capi.MultiSdfGpu(ranks, [0] * ranks)
        mg.set_option("dense_retry", 0)
        for p, vb in ((0.5, False), (0.01, False), (0.002, True), (0.3, True)):
            m = synth.bernoulli_mask(shape, p, 6)
            ex, ex_ext, _ = O.exact_sdf(m, res, vb)
            for halo in (1, 8):
                mg.set_option("halo", halo)
                got, ext = mg.build(m, res, vb)
                assert np.array_equal(got, ex) and ext == ex_ext, (ranks, p, vb, halo)
        mg.close()
