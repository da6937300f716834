"""GPU: the SDF build path and its stage entry points on masks and fields that are off their 16-byte alignment.

The build path picks kernels by the alignment of the caller's pointers, and every tensor the rest of the
suite hands over is at least 16-byte aligned.  Here every device buffer lives in an arena of alignment_harness.py: the library
gets arena + 256 + shift, 4 KiB and more of sentinel lie on either side, both bands are checked after every call and the payload
is read back from the same offset.  alignment_cases.py holds the shifts, the shapes, the tier-forcing options and the audit
table (which pointer, how wide an access, behind which predicate) that the cases walk: the control at shift 0, one pointer moved
at a time, then all of them at once.

Every field is compared bit for bit with oracle.exact_sdf (stage fields with test_gpu_parity._exact_stage_fields, bits with
capi.pack_bits_host, masks with oracle.classify_cells, gradients with analysis_scenes.grid_gradient), the extrema for equality,
and with the control's result on the same handle.  Where the library reports which arm ran, the expected bits come from the audit
table: a mask off its alignment leaves the fused bit clear, a field off its alignment the plane16 and KD3 bits, a plane field off
its alignment the tiered bit and the far-field instance of sdfgpu_sweep_x_lines_device.

One parametrised test, its cases ordered by shape: the scalar shapes run first, the widest rows last."""
import functools

import numpy as np
import pytest
import torch

import alignment_cases as C
import alignment_harness as H
import analysis_scenes as A
from oracle import oracle as O
from sdf_tools_amd import capi, synth
from stream_harness import same_or_nan
from test_gpu_parity import _exact_stage_fields

pytestmark = pytest.mark.gpu
RES = 0.05
# row lengths of the tuned dense kernels: 2 words (word-wise staging), 4 (the shortest row staged with 16-byte loads), 16
DENSE_SHAPES = [(9, 12, 64), (5, 6, 128), (3, 8, 512)]


# ---- scenes and references, computed once ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(shape, p, seed=7):
    m = synth.bernoulli_mask(shape, p, seed)
    if not m.any():                                              # (0.002 of a few hundred voxels: one obstacle, so that the scene has two classes)
        m = m.copy()
        m[tuple(s // 2 for s in shape)] = 1
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def exact(shape, p, vb, seed=7, res=RES):
    sdf, ext, dsq = O.exact_sdf(scene(shape, p, seed), res, vb)
    return sdf, tuple(float(v) for v in ext), dsq


@functools.lru_cache(maxsize=None)
def plane_field(shape, p):
    return _exact_stage_fields(scene(shape, p))[1]


def cells8(shape, seed):
    rng = np.random.default_rng(seed)
    c = np.zeros(shape + (2,), np.float32)
    c[..., 0] = rng.choice(np.array([0.0, 0.5, 1.0, 0.50000006, np.nan], np.float32), size=shape, p=[0.5, 0.1, 0.3, 0.05, 0.05])
    c[..., 1] = rng.random(shape).astype(np.float32)
    return c


def cells16(c8, seed):
    n = c8[..., 0].size
    raw = np.random.default_rng(seed).integers(0, 256, (n, 16), dtype=np.uint8)
    raw[:, 4:8] = np.ascontiguousarray(c8[..., 0]).reshape(-1).view(np.uint8).reshape(n, 4)       # occupancy at offset 4
    return raw


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_field(what, got, want):
    if not bits_equal(got, want):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        sentinel = int((got.view(np.uint32) == 0xA5A5A5A5).sum())
        pytest.fail("%s: %d of %d voxels differ (%d still hold the sentinel), the first at %s: got %r, want %r"
                    % (what, len(bad), got.size, sentinel, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- the handle -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle():
    """a handle of this module's own: the options set here never reach another test"""
    h = capi.SdfGpu(0)
    yield h
    h.close()


def configure(h, tier):
    """every option from its default, the tier's on top, the policy forgotten (what the handle learnt from one shift must not
    choose the next one's kernels), then the options that hold for one build"""
    opts = dict(C.OPTION_DEFAULTS)
    opts.update({k: v for k, v in C.TIERS[tier].items() if k != "once"})
    for k, v in opts.items():
        h.set_option(k, v)
    h.set_option("policy_reset", 1)
    for k, v in C.TIERS[tier].get("once", {}).items():
        h.set_option(k, v)
    return opts


def stream():
    return torch.cuda.current_stream().cuda_stream


def moved(shifts):
    return {name for name, s in shifts.items() if s % 16}


# ---- whole builds ---------------------------------------------------------------------------------------------------------------
def run_build_device(h, shape, tier):
    nx, ny, nz = shape
    for p in C.DENSITIES:
        for vb in (False, True):
            want, want_ext, _ = exact(shape, p, vb)
            base = None
            for label, sh in C.moves("build_device"):
                what = "build_device %s p=%g vb=%d tier %s, %s" % (shape, p, vb, tier, label)
                opts = configure(h, tier)
                b = H.Buffers(sh)
                d_mask, d_out = b.put("mask", scene(shape, p) * np.uint8(3)), b.out("out", want.nbytes)
                h.build_device(d_mask, shape, d_out, RES, vb, stream())
                info, ext, path = h.last_build_info(), h.get_extrema(), h.last_path()
                print(what, info, path)
                b.check(what)
                got = b.get("out", np.float32, shape)
                assert_field(what, got, want)
                assert ext == want_ext, (what, ext, want_ext)
                if base is None:
                    base = (got, info, path)
                    # the control takes the wide arms the shape and the options allow (or the moved cases show nothing)
                    assert info["plane16"] == bool(opts["plane16"] and nz % 4 == 0 and (ny * nz) % 8 == 0), (what, info)
                    assert info["dense"] == bool(opts["dense"]), (what, info)
                    if tier.startswith("fused") and nz in (512, 1024):
                        assert info["fused_zy"], (what, info)
                    continue
                assert_field(what + " against the control", got, base[0])
                if "mask" in moved(sh):
                    assert not info["fused_zy"], (what, info)                  # K12 loads 16 mask bytes per lane
                if "out" in moved(sh):
                    # K3/16 and the tuned ball kernels store 16 bytes per lane: int32 plane field, generic dense kernel
                    assert not info["plane16"] and not info["dense3"] and not info["dense3_staged"], (what, info)
                    assert info["dense"] == base[1]["dense"], (what, info)
                else:
                    assert {k: info[k] for k in ("plane16", "dense", "dense3", "dense3_staged")} == \
                           {k: base[1][k] for k in ("plane16", "dense", "dense3", "dense3_staged")}, (what, info, base[1])
                    assert path["dense_certified"] == base[2]["dense_certified"], (what, path, base[2])


def run_build_cells_device(h, shape, tier):
    for stride, off, kind in ((8, 0, "cells8"), (16, 4, "cells16")):
        c8 = cells8(shape, 50)
        raw = c8 if stride == 8 else cells16(c8, 3)
        for unknown, vb in ((True, False), (False, True)):
            want, want_ext, _ = O.exact_sdf(O.classify_cells(c8, unknown), RES, vb)
            want_ext = tuple(float(v) for v in want_ext)
            base = None
            for label, sh in C.moves("build_cells_device", {"cells": kind}):
                what = "build_cells_device %s stride %d unknown=%d vb=%d tier %s, %s" % (shape, stride, unknown, vb, tier, label)
                configure(h, tier)
                b = H.Buffers(sh)
                d_cells, d_out = b.put("cells", raw), b.out("out", want.nbytes)
                h.build_cells_device(d_cells, shape, d_out, stride, off, unknown, RES, vb, stream())
                info, ext = h.last_build_info(), h.get_extrema()
                b.check(what)
                got = b.get("out", np.float32, shape)
                assert_field(what, got, want)
                assert ext == want_ext, (what, ext, want_ext)
                if base is None:
                    base = (got, info)
                    continue
                assert_field(what + " against the control", got, base[0])
                assert not info["fused_zy"]
                if "out" in moved(sh):
                    assert not info["plane16"] and not info["dense3"] and not info["dense3_staged"], (what, info)
                else:
                    assert info == base[1], (what, info, base[1])


def run_build_batch_device(h, shape, fast):
    batch = 3
    n = int(np.prod(shape))
    masks = np.stack([scene(shape, 0.3, 60 + k) for k in range(batch)])
    res = np.array([1.0, 0.25, 0.037])
    for vb in (False, True):
        want = [O.exact_sdf(masks[k], res[k], vb) for k in range(batch)]
        base = None
        for label, sh in C.moves("build_batch_device"):
            what = "build_batch_device %d x %s vb=%d, %s" % (batch, shape, vb, label)
            configure(h, "default")
            b = H.Buffers(sh)
            d_masks, d_out = b.put("masks", masks * np.uint8(255)), b.out("out", batch * n * 4)
            h.build_batch_device(d_masks, batch, shape, d_out, res.copy(), vb, stream())
            ext = h.get_extrema_batch(batch)
            b.check(what)
            assert h.last_batch_info()[0] == fast, what                          # the audit's arm: every axis <= 128 or one build per grid
            got = b.get("out", np.float32, (batch,) + shape)
            for k in range(batch):
                assert_field("%s, grid %d" % (what, k), got[k], want[k][0])
                assert ext[k] == tuple(float(v) for v in want[k][1]), (what, k)
            if base is None:
                base = got
            assert_field(what + " against the control", got, base)


def run_gradient_batch_device(h, shape, f64):
    batch = 3
    res = np.array([0.05, 0.25, 1.0])
    dt = np.float64 if f64 else np.float32
    fields = np.stack([O.exact_sdf(scene(shape, 0.3, 60 + k), res[k], False)[0] for k in range(batch)])
    want = np.stack([A.grid_gradient(fields[k], res[k], True).astype(dt) for k in range(batch)])
    for label, sh in C.moves("gradient_batch_device", {"out": "doubles"} if f64 else None):
        what = "gradient_batch_device %d x %s f64=%d, %s" % (batch, shape, f64, label)
        b = H.Buffers(sh)
        d_sdf, d_out = b.put("sdf", fields), b.out("out", want.nbytes)
        h.gradient_batch_device(d_sdf, batch, shape, d_out, res.copy(), True, f64, stream())
        b.check(what)
        assert same_or_nan(b.get("out", dt, want.shape), want), what


# ---- stage entry points ---------------------------------------------------------------------------------------------------------
def run_sweep_zy_device(h, shape, tier):
    for p in C.DENSITIES:
        want = plane_field(shape, p)
        base = None
        for label, sh in C.moves("sweep_zy_device"):
            what = "sweep_zy_tiered_device %s p=%g tier %s, %s" % (shape, p, tier, label)
            configure(h, tier)
            b = H.Buffers(sh)
            d_mask, d_plane, d_far = b.put("mask", scene(shape, p) * np.uint8(255)), b.out("plane", want.nbytes), b.out("far", 4)
            h.sweep_zy_tiered_device(d_mask, shape, d_plane, d_far, stream())
            b.check(what)
            got, far = b.get("plane", np.int32, shape), int(b.get("far", np.uint32)[0])
            assert bits_equal(got, want), (what, int((got != want).sum()))
            assert far in (0, 1), (what, far)
            # sdfgpu_sweep_zy_device: the same call without the hint
            b2 = H.Buffers(sh)
            d_mask, d_plane = b2.put("mask", scene(shape, p)), b2.out("plane", want.nbytes)
            configure(h, tier)
            h.sweep_zy_device(d_mask, shape, d_plane, stream())
            b2.check(what + " (sweep_zy_device)")
            assert bits_equal(b2.get("plane", np.int32, shape), want), what + " (sweep_zy_device)"
            if base is None:
                base = far
            if "plane" not in moved(sh):                                        # (off its alignment the call is untiered: no probe, the hint is 0)
                assert far == base, (what, far, base)
            else:
                assert far == 0, (what, far)


def run_sweep_x_device(h, shape, halo):
    nx, ny, nz = shape
    a, bx, lo, hi = (3, 6, 2, 2) if halo else (0, nx, 0, 0)
    for p in ((0.3,) if halo else C.DENSITIES):
        plane = np.ascontiguousarray(plane_field(shape, p)[a - lo:bx + hi])
        for vb in (False, True):
            want, want_ext, _ = exact(shape, p, vb)
            want = want[a:bx]
            base = None
            for label, sh in C.moves("sweep_x_device"):
                what = "sweep_x_device %s rows %d..%d halo %d p=%g vb=%d, %s" % (shape, a, bx, lo, p, vb, label)
                configure(h, "default")
                b = H.Buffers(sh)
                d_plane, d_out = b.put("plane", plane), b.out("out", want.nbytes)
                d_max, d_status = b.put("maxdsq", np.zeros(2, np.uint32)), b.put("status", np.zeros(1, np.uint32))
                h.sweep_x_device(d_plane, lo, bx - a, hi, ny, nz, a - lo > 0, bx + hi < nx, a, nx, RES, vb, d_out, d_max, d_status, stream())
                b.check(what)
                got, mx, status = b.get("out", np.float32, want.shape), b.get("maxdsq", np.uint32), int(b.get("status", np.uint32)[0])
                assert status == 0, (what, status)
                assert_field(what, got, want)
                if not halo:
                    assert capi.extrema_from_dsq(int(mx[0]), int(mx[1]), RES) == want_ext, (what, mx)
                if base is None:
                    base = mx
                assert np.array_equal(mx, base), (what, mx, base)


def run_sweep_x_lines_device(h, shape, tier):
    nx, ny, nz = shape
    for p in C.DENSITIES:
        for ya, yb in ((0, ny), (2, ny - 1)):
            plane = np.ascontiguousarray(plane_field(shape, p)[:, ya:yb])
            for vb in (False, True):
                want, want_ext, _ = exact(shape, p, vb)
                want = np.ascontiguousarray(want[:, ya:yb])
                base = None
                for label, sh in C.moves("sweep_x_lines_device"):
                    what = "sweep_x_lines_device %s y %d..%d p=%g vb=%d tier %s, %s" % (shape, ya, yb, p, vb, tier, label)
                    opts = configure(h, tier)
                    b = H.Buffers(sh)
                    d_plane, d_out, d_max = b.put("plane", plane), b.out("out", want.nbytes), b.put("maxdsq", np.zeros(2, np.uint32))
                    h.sweep_x_lines_device(d_plane, nx, yb - ya, nz, ya, ny, RES, vb, d_out, d_max, stream())
                    info = h.last_build_info()
                    b.check(what)
                    got, mx = b.get("out", np.float32, want.shape), b.get("maxdsq", np.uint32)
                    assert_field(what, got, want)
                    if (ya, yb) == (0, ny):
                        assert capi.extrema_from_dsq(int(mx[0]), int(mx[1]), RES) == want_ext, (what, mx)
                    arm = (info["lines_tiered"], info["far_x_instance"])
                    if base is None:
                        base = (mx, arm)
                        assert info["lines_tiered"] == bool(opts["envelope"]), (what, info)   # the control is tiered wherever the option allows
                    assert np.array_equal(mx, base[0]), (what, mx, base[0])
                    if "plane" in moved(sh):
                        # the far-field kernel reads the plane field with 16-byte loads: off its alignment the call is the marching sweep alone
                        assert arm == (False, -1), (what, info)
                    else:
                        assert arm == base[1], (what, info, base[1])


def run_pack_bits_device(h, shape):
    nx, ny, nz = shape
    for p in C.DENSITIES:
        want = capi.pack_bits_host(scene(shape, p))
        for label, sh in C.moves("pack_bits_device"):
            what = "pack_bits_device %s p=%g, %s" % (shape, p, label)
            b = H.Buffers(sh)
            d_mask, d_bits = b.put("mask", scene(shape, p) * np.uint8(7)), b.out("bits", want.nbytes)
            h.pack_bits_device(d_mask, nx * ny, nz, d_bits, stream())
            b.check(what)
            assert bits_equal(b.get("bits", np.uint32), want), what


def check_dense(what, got, rows, mx, uncertified, shape, p, whole):
    """what the dense stages promise: exact wherever the nearest voxel of the other class is within d^2 = 8; with the flag down,
    everywhere, and the maxima are the field's"""
    want, want_ext, dsq = exact(shape, p, False)
    near = np.abs(dsq[rows]) <= 8
    assert bits_equal(got[near], want[rows][near]), (what, "voxels within the ball differ")
    if uncertified == 0:
        assert_field(what, got, want[rows])
        if whole:
            assert capi.extrema_from_dsq(int(mx[0]), int(mx[1]), RES) == want_ext, (what, mx)


def run_dense_ball_device(h, shape):
    nx, ny, nz = shape
    configure(h, "default")
    for p in C.DENSITIES:
        bits = capi.pack_bits_host(scene(shape, p))
        for out_lo, out_hi in [(0, nx)] + ([(2, nx - 2)] if nx >= 5 else []):
            rows = slice(out_lo, out_hi)
            base = None
            for label, sh in C.moves("dense_ball_device"):
                what = "dense_ball_device %s planes %d..%d p=%g, %s" % (shape, out_lo, out_hi, p, label)
                b = H.Buffers(sh)
                d_bits, d_out = b.put("bits", bits), b.out("out", (out_hi - out_lo) * ny * nz * 4)
                d_max, d_unc = b.put("maxdsq", np.zeros(2, np.uint32)), b.put("uncertified", np.zeros(1, np.uint32))
                h.dense_ball_device(d_bits, nx, out_lo, out_hi, ny, nz, RES, d_out, d_max, d_unc, stream())
                b.check(what)
                got = b.get("out", np.float32, (out_hi - out_lo, ny, nz))
                mx, unc = b.get("maxdsq", np.uint32), int(b.get("uncertified", np.uint32)[0])
                assert bits_equal(b.get("bits", np.uint32), bits), what + ": the caller's bit planes changed"
                check_dense(what, got, rows, mx, unc, shape, p, (out_lo, out_hi) == (0, nx))
                if base is None:
                    base = (got, mx, unc)
                assert_field(what + " against the control", got, base[0])
                assert np.array_equal(mx, base[1]) and (unc != 0) == (base[2] != 0), (what, mx, unc, base[1:])


def run_slab_dense_phase(h, shape):
    """phases 0, 1, 2 of one rank without neighbours: phase 0 packs the slab, phase 2 runs the ball kernel and folds"""
    nx, ny, nz = shape
    configure(h, "default")
    for p in C.DENSITIES:
        bits = capi.pack_bits_host(scene(shape, p))
        base = None
        for label, sh in C.moves("slab_dense_phase"):
            what = "slab_dense_phase %s p=%g, %s" % (shape, p, label)
            b = H.Buffers(sh)
            d_mask, d_bits = b.put("mask", scene(shape, p) * np.uint8(255)), b.out("bits", bits.nbytes)
            d_out, d_small = b.out("out", nx * ny * nz * 4), b.put("small", np.full(4, 7, np.uint32))
            for phase in (0, 1, 2):
                h.slab_dense_phase(phase, d_mask, nx, ny, nz, d_bits, 0, 0, RES, d_out, d_small, stream())
                b.check("%s, phase %d" % (what, phase))
            assert bits_equal(b.get("bits", np.uint32), bits), what + ": bit planes"
            got, small = b.get("out", np.float32, shape), b.get("small", np.uint32)
            assert small[2] == 0, (what, small)
            check_dense(what, got, slice(0, nx), small[:2], int(small[3]), shape, p, True)
            if base is None:
                base = (got, small)
            assert_field(what + " against the control", got, base[0])
            assert np.array_equal(small[:2], base[1][:2]) and (small[3] != 0) == (base[1][3] != 0), (what, small, base[1])


def run_classify_cells_device(h, shape):
    c8 = cells8(shape, 52)
    for stride, off, kind in ((8, 0, "cells8"), (16, 4, "cells16")):
        raw = c8 if stride == 8 else cells16(c8, 3)
        for unknown in (False, True):
            want = O.classify_cells(c8, unknown)
            for label, sh in C.moves("classify_cells_device", {"cells": kind}):
                what = "classify_cells_device %s stride %d unknown=%d, %s" % (shape, stride, unknown, label)
                b = H.Buffers(sh)
                d_cells, d_mask = b.put("cells", raw), b.out("mask", want.size)
                h.classify_cells_device(d_cells, want.size, d_mask, stride, off, unknown, stream())
                b.check(what)
                assert bits_equal(b.get("mask", np.uint8, shape), want), what


def run_upload_classified(h, shape):
    src = scene(shape, 0.3) * np.uint8(3)
    want = (src != 0).astype(np.uint8)
    for label, sh in C.moves("upload_classified"):
        what = "upload_classified %s, %s" % (shape, label)
        b = H.Buffers(sh)
        d_mask = b.out("mask", want.size)
        h.upload_classified(d_mask, filled=src, stream=stream())
        b.check(what)
        assert bits_equal(b.get("mask", np.uint8, shape), want), what


# ---- the cases, ordered by shape ------------------------------------------------------------------------------------------------
def _cases():
    tiny, small = (4, 5, 13), (6, 6, 20)
    cases = []
    for shape in (tiny, small):                                    # calls whose kernels are scalar whatever the shape
        cases += [(shape, "classify_cells_device", run_classify_cells_device, ()),
                  (shape, "gradient_batch_device-f32", run_gradient_batch_device, (False,)),
                  (shape, "gradient_batch_device-f64", run_gradient_batch_device, (True,)),
                  (shape, "build_batch_device-fast-path", run_build_batch_device, (True,))]
    cases += [(tiny, "upload_classified", run_upload_classified, ()), ((9, 12, 64), "upload_classified", run_upload_classified, ())]
    # above 128 voxels on an axis a batch is one build per grid: grid k's mask and field start k * n voxels in (n = 393: every
    # alignment class of a byte, two of a float, even in the control)
    cases += [((1, 3, 131), "build_batch_device-per-grid", run_build_batch_device, (False,)),
              ((2, 3, 256), "build_batch_device-per-grid", run_build_batch_device, (False,))]
    for shape in C.SHAPES:
        nx, ny, nz = shape
        for tier in C.TIERS:
            cases.append((shape, "build_device-" + tier, run_build_device, (tier,)))
        for tier in ("default", "sweeps"):
            if shape in (small, (9, 12, 64)):
                cases.append((shape, "build_cells_device-" + tier, run_build_cells_device, (tier,)))
        for tier in ("default", "sweeps-z-workgroup", "sweeps-unbounded", "fused-unbounded", "far-field-only"):
            cases.append((shape, "sweep_zy_device-" + tier, run_sweep_zy_device, (tier,)))
        cases.append((shape, "sweep_x_device", run_sweep_x_device, (False,)))
        if nx >= 9:
            cases.append((shape, "sweep_x_device-halo", run_sweep_x_device, (True,)))
        for tier in ("default", "far-field-only", "far-field-probed-handoff", "sweeps-unbounded"):
            cases.append((shape, "sweep_x_lines_device-" + tier, run_sweep_x_lines_device, (tier,)))
    for shape in DENSE_SHAPES:
        cases += [(shape, "pack_bits_device", run_pack_bits_device, ()), (shape, "dense_ball_device", run_dense_ball_device, ()),
                  (shape, "slab_dense_phase", run_slab_dense_phase, ())]
    order = {s: i for i, s in enumerate(sorted({c[0] for c in cases}, key=lambda s: (s[2], s)))}
    return sorted(cases, key=lambda c: order[c[0]])               # (stable: a shape's cases keep the order above)


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=["%dx%dx%d-%s" % (c[0] + (c[1],)) for c in CASES])
def test_off_alignment(handle, case):
    shape, _, run, args = case
    run(handle, shape, *args)


# ---- under red zones ------------------------------------------------------------------------------------------------------------
def test_under_red_zones(monkeypatch):
    """SDFGPU_REDZONE=1 in the environment of sdfgpu_create: the library's own fields -- the scratch copies of a stage call's bit
    planes and field among them -- carry canaries, and every call here ends in their check.  One shape per tier, mask at +1,
    field at +4."""
    monkeypatch.setenv("SDFGPU_REDZONE", "1")
    h = capi.SdfGpu(0)
    try:
        sh = {"mask": 1, "out": 4, "bits": 4, "maxdsq": 4, "uncertified": 4, "small": 4}
        for shape, p, tier in (((9, 12, 64), 0.3, "default"), ((9, 12, 64), 0.002, "far-field-predicted-plane-skip"),
                               ((6, 6, 20), 0.3, "sweeps"), ((3, 8, 512), 0.002, "fused"), ((3, 8, 512), 0.3, "dense-kd3")):
            nx, ny, nz = shape
            for vb in (False, True):
                what = "red zones: build_device %s p=%g vb=%d tier %s" % (shape, p, vb, tier)
                want, want_ext, _ = exact(shape, p, vb)
                configure(h, tier)
                b = H.Buffers(sh)
                d_mask, d_out = b.put("mask", scene(shape, p)), b.out("out", want.nbytes)
                h.build_device(d_mask, shape, d_out, RES, vb, stream())
                h.redzone_check()
                b.check(what)
                assert_field(what, b.get("out", np.float32, shape), want)
                assert h.get_extrema() == want_ext, what
        for shape in DENSE_SHAPES:
            nx, ny, nz = shape
            configure(h, "default")
            for p in C.DENSITIES:
                what = "red zones: dense stages %s p=%g" % (shape, p)
                bits = capi.pack_bits_host(scene(shape, p))
                b = H.Buffers(sh)
                d_bits, d_out = b.put("bits", bits), b.out("out", nx * ny * nz * 4)
                d_max, d_unc = b.put("maxdsq", np.zeros(2, np.uint32)), b.put("uncertified", np.zeros(1, np.uint32))
                h.dense_ball_device(d_bits, nx, 0, nx, ny, nz, RES, d_out, d_max, d_unc, stream())
                h.redzone_check()
                b.check(what)
                check_dense(what, b.get("out", np.float32, shape), slice(0, nx), b.get("maxdsq", np.uint32),
                            int(b.get("uncertified", np.uint32)[0]), shape, p, True)
                b = H.Buffers(sh)
                d_mask, d_bits = b.put("mask", scene(shape, p)), b.out("bits", bits.nbytes)
                d_out, d_small = b.out("out", nx * ny * nz * 4), b.put("small", np.zeros(4, np.uint32))
                for phase in (0, 1, 2):
                    h.slab_dense_phase(phase, d_mask, nx, ny, nz, d_bits, 0, 0, RES, d_out, d_small, stream())
                    h.redzone_check()
                b.check(what + " (slab phases)")
                small = b.get("small", np.uint32)
                check_dense(what + " (slab phases)", b.get("out", np.float32, shape), slice(0, nx), small[:2], int(small[3]), shape, p, True)
    finally:
        h.close()
