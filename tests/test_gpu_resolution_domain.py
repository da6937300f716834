"""GPU: every place that finishes a squared distance as float(sqrt((double)D) * resolution) and applies the sign, at every class of
resolution (resolution_domain.py: doubles that no float holds, float-exact values, results that are subnormal, straddle FLT_MIN,
underflow to signed zeros, overflow partly or wholly), bit for bit against the exact oracle -- which test_resolution_domain_cpu.py
pins against a plain numpy restatement at the same resolutions.  Then the consumers of the field (full-grid gradient, its batch
form, the per-point queries, the projection) on full-mantissa fields around the gate of the fp32-scaled gradient kernel, and the
one rule for resolutions that are refused.  Tolerance: none; -0.0 != +0.0; NaN == NaN where a gradient has none.

Finishing sites (grep sqrt under sdf_tools_amd/csrc; every line that finishes a distance is here).  `opts` are set after a policy
reset in front of EVERY build; `proof` is what the case asserts so that a build that fell to another tier fails.

  site                                   line(s)                                      opts / scene                                     proof
  KD, 7 host magnitudes (tuned)          sdfgpu.hip launch_ball_dense `a.mag[l] =`    dense3=0; every level 1..8, nz = 64              dense, not dense3 / staged, certified, max D <= 8
  KD, 7 host magnitudes (generic)        sdfgpu.hip launch_dense_generic `a.mag[l] =` dense3=0; same scene, nz = 40 (nz % 32 != 0)     dense, certified (the shape has no tuned form)
  KD3, 13 host magnitudes                sdfgpu.hip launch_ball_dense `a.mag3[l] =`   dense3_mode=1; every level 1..14; also nz = 512  dense3, certified, 8 < max D <= 14
                                                                                      (KD3's fixed-pitch instance)
  KF device sqrt                         sdfgpu_dense.hpp k_ball_fixup `sqrt((double)best)`   dense3=0 fixup_mode=1 (behind KD) and    certified, max D > 8 resp. > 14: only KF
                                                                                      dense3_mode=1 dense_shell=0 (behind KD3)         finishes such a voxel in a certified build
  KD6 shell pass                         sdfgpu_dense6.hpp `__builtin_sqrt(kShellD2`  dense3_mode=1 shell_min_words=0; 6-lattice       dense3, certified -- and NOT certified with
                                                                                      (d^2 = 27 for a third of the voxels)             dense_shell=0 (KF alone refuses the scene)
  K3 marching x sweep                    sdfgpu_kernels.hpp `sqrt((double)D) * a.resolution`  dense=0 envelope=0 plane16=0             no dense, no plane16, no far flags
  K3/16 LDS table / finish_large         sdfgpu_sweep_x16.hpp `lut[i] =`, finish_large        dense=0 envelope=0; noise (window fast   plane16, no dense, no far flags; max D < 16,
                                                                                      path), sparse noise, corner voxel of 48x8x64     < 1024, >= 1024 per scene
  far-field kernel, chunk finish         sdfgpu_envelope_dc.hpp `sqrt_exact_pos((double)D[k])`  dense=0 envelope_mode=1; generic       far_x, no dense, far_x_instance
  far-field kernel, emit_filled          sdfgpu_envelope_dc.hpp emit_filled           instances (vector / scalar loads, 512 lanes),    the sparse scenes' filled voxels are pass 0's
  far-field kernel, fixed instances      same lines, L = 512 / 1024 compile-time      (512, 8, 8) and (1024, 4, 8), dc_fixed 1 / 0;    (few and shallow), the inverse scenes' the
                                                                                      i32_handoff 0, flat_tiles 2                      second pass's
  stand-by pair (LOOP form)              same lines behind a trusted dense tier       certified build, expect_dense=1, far scene;      standby_far, far_y and far_x, not certified
                                                                                      standby_fold 1 / 0
  batched kernel                         sdfgpu_batch.hip `sqrt((double)D) * res`     per-grid resolutions, every class in one batch   last_batch_info() == (True, 2)
  host extrema                           sdfgpu.hip sdfgpu_extrema_from_dsq           get_extrema / get_extrema_batch of every case above, and extrema_from_dsq itself
  slab stages                            sdfgpu_sweep_x_device (K3: the only kernel it has), sdfgpu_sweep_x_lines_device (K3 alone with envelope=0, the far-field
                                         kernel behind a forced decision with envelope_mode=1: lines_tiered and far_x_instance of sdfgpu_last_build_info),
                                         sdfgpu_slab_dense_phase (KD: status word 3 stays 0)
Not a finishing site: sdfgpu_finish.hpp / k_finish_table (a debug kernel, test_gpu_finish.py), sdfgpu_project.hip and
sdfgpu_convex.hip (norms), the integer square root of a search radius in sdfgpu_envelope_dc.hpp.
No site is left out.  Scenes whose D stays below 16 (the dense tiers') get the additional straddle / overflow resolutions that
split them (resolution_domain.class_resolutions)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import analysis_scenes as A
import resolution_domain as R
from oracle import oracle as O
from sdf_tools_amd import capi, synth
from test_gpu_analysis_edges import _device_gradient, _same

pytestmark = pytest.mark.gpu

DEFAULTS = {"dense": 1, "dense3": 1, "dense3_mode": 0, "fixup_mode": 0, "dense_shell": 1, "shell_min_words": -1, "plane16": 1,
            "envelope": 1, "envelope_dc": 1, "envelope_mode": 0, "dc_fixed": 1, "i32_handoff": 1, "flat_tiles": 1, "standby_fold": 1}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set(gpu, opts):
    gpu.set_option("policy_reset", 1)
    for k, v in opts.items():
        gpu.set_option(k, v)


def _restore(gpu, opts):
    for k in opts:
        gpu.set_option(k, DEFAULTS[k])
    gpu.set_option("policy_reset", 1)


def _run_site(gpu, opts, mask, vb, proof, prepare=None):
    """Every class on one (site, scene): the build's bits and extrema against the exact oracle, the site's proof after each build."""
    mask = np.ascontiguousarray(mask, np.uint8)
    _, _, dsq = O.exact_sdf(mask, 1.0, vb)
    classes = R.class_resolutions(dsq)
    assert sorted({c for c, _ in classes}) == list("abcdefg")
    try:
        for cls, res in classes:
            want, want_ext, _ = O.exact_sdf(mask, res, vb)
            _set(gpu, opts)
            if prepare is not None:
                prepare(gpu)
            got, ext = gpu.build(mask, res, vb)
            info, path = gpu.last_build_info(), gpu.last_path()
            proof(info, path, dsq)
            bad = np.argwhere(_bits(got) != _bits(want))
            assert len(bad) == 0, "class %s res %r: %d voxels differ, first %s got %r want %r (%s %s)" % (
                cls, res, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])], info, path)
            assert ext == want_ext and gpu.get_extrema() == want_ext, (cls, res, ext, want_ext)
    finally:
        _restore(gpu, opts)
    return dsq


def _noise(shape, p, seed):
    m = synth.bernoulli_mask(shape, p, seed)
    assert 0 < m.sum() < m.size
    return m


# ---- the dense tier ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(13, 9, 64), (13, 9, 40)], ids=["tuned", "generic"])
def test_dense_ball_magnitudes(gpu, shape):
    def proof(info, path, dsq):
        assert info["dense"] and not info["dense3"] and not info["dense3_staged"] and path["dense_certified"], (info, path)
        assert np.abs(dsq).max() <= 8
    levels = R.ball_levels(shape)
    for vb in (False, True):
        for m in (levels, 1 - levels, _noise(shape, 0.5, 3)):
            dsq = _run_site(gpu, {"dense3": 0}, m, vb, proof)
    assert set(np.unique(np.abs(O.exact_sdf(levels, 1.0)[2])).tolist()) == {1, 2, 3, 4, 5, 6, 8}


@pytest.mark.parametrize("shape", [(13, 13, 64), (13, 5, 512)], ids=["nz64", "nz512-fixed-pitch"])
def test_wide_ball_magnitudes(gpu, shape):
    def proof(info, path, dsq):
        assert info["dense"] and info["dense3"] and path["dense_certified"], (info, path)
        assert 8 < np.abs(dsq).max() <= 14
    m = R.ball3_levels(shape)
    assert set(np.unique(np.abs(O.exact_sdf(m, 1.0)[2])).tolist()) == {1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14}
    for mm in (m, 1 - m):
        _run_site(gpu, {"dense3_mode": 1}, mm, False, proof)


def _cavity(shape, c):
    m = _noise(shape, 0.5, 9)
    m[3:3 + c, 2:2 + c, 20:20 + c] = 0
    return m


def test_fixup_kernel_finish(gpu):
    def behind_kd(info, path, dsq):
        assert info["dense"] and not info["dense3"] and not info["dense3_staged"] and path["dense_certified"], (info, path)
        assert np.abs(dsq).max() > 8                         # beyond KD's ball: in a certified build only KF writes such a voxel
    def behind_kd3(info, path, dsq):
        assert info["dense3"] and path["dense_certified"], (info, path)
        assert np.abs(dsq).max() > 14
    # a c^3 hole in noise (or a c^3 block in it): the voxel in its middle is (c + 1) / 2 from the nearest voxel of the other class
    for m in (_cavity((16, 12, 64), 5), 1 - _cavity((16, 12, 64), 5)):
        _run_site(gpu, {"dense3": 0, "fixup_mode": 1}, m, False, behind_kd)
    for m in (_cavity((16, 12, 64), 9), 1 - _cavity((16, 12, 64), 9)):
        _run_site(gpu, {"dense3_mode": 1, "dense_shell": 0}, m, False, behind_kd3)


def test_shell_pass_finish(gpu):
    def proof(info, path, dsq):
        assert info["dense3"] and path["dense_certified"], (info, path)
        assert np.abs(dsq).max() == 27
    m = np.zeros((13, 13, 64), np.uint8)
    m[::6, ::6, ::6] = 1                                      # (3, 3, 3) away for a third of the voxels: the shell's levels 16 .. 36
    for mm in (m, 1 - m):
        _run_site(gpu, {"dense3_mode": 1, "shell_min_words": 0}, mm, False, proof)
    # the proof that the shell pass, not KF, finished them: without it the same build is not certified
    opts = {"dense3_mode": 1, "dense_shell": 0}
    try:
        _set(gpu, opts)
        got, ext = gpu.build(m, 1.0 / 3.0)
        assert not gpu.last_path()["dense_certified"], gpu.last_path()
        want, want_ext, _ = O.exact_sdf(m, 1.0 / 3.0)
        assert np.array_equal(_bits(got), _bits(want)) and ext == want_ext
    finally:
        _restore(gpu, opts)


# ---- the marching x sweeps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 10, 40), (9, 11, 7)], ids=["vector", "scalar"])
def test_marching_x_sweep_finish(gpu, shape):
    def proof(info, path, dsq):
        assert not info["dense"] and not info["plane16"] and not info["fused_zy"] and not info["standby_far"], info
        assert not path["far_y"] and not path["far_x"] and not path["dense_certified"], path
    for vb in (False, True):
        for m in (_noise(shape, 0.03, 5), 1 - _noise(shape, 0.03, 5), _noise(shape, 0.5, 6), R.corner_voxel(shape)):
            _run_site(gpu, {"dense": 0, "envelope": 0, "plane16": 0}, m, vb, proof)


def test_plane16_x_sweep_table_and_fallback(gpu):
    def proof(lo, hi):
        def check(info, path, dsq):
            assert info["plane16"] and not info["dense"] and not info["fused_zy"] and not info["standby_far"], info
            assert not path["far_y"] and not path["far_x"], path
            assert lo <= np.abs(dsq).max() < hi, np.abs(dsq).max()
        return check
    opts = {"dense": 0, "envelope": 0}
    _run_site(gpu, opts, _noise((9, 10, 40), 0.5, 6), False, proof(2, 16))         # every wave decided by the window: the packed finish
    for vb in (False, True):
        # the exact scan, every distance from the table (the border keeps every voxel of so small a grid within 16: the border form
        # of the kernel has no packed finish, so the general one does the work there as well)
        _run_site(gpu, opts, _noise((9, 10, 40), 0.03, 5), vb, proof(1 if vb else 16, 1024))
        _run_site(gpu, opts, 1 - _noise((9, 10, 40), 0.03, 5), vb, proof(1, 1024))
    _run_site(gpu, opts, R.corner_voxel((48, 8, 64)), False, proof(1024, 1 << 20))  # beyond the table: finish_large
    _run_site(gpu, opts, 1 - R.corner_voxel((48, 8, 64)), False, proof(1024, 1 << 20))


# ---- the far-field kernel -----------------------------------------------------------------------------------------------------------
def _far_proof(instance):
    def proof(info, path, dsq):
        assert not info["dense"] and not info["standby_far"], info
        assert info["far_x_instance"] == instance, info        # WHICH instantiation of the kernel was enqueued for the x sweep ...
        assert path["far_x"] and not path["dense_certified"], path      # ... and that it did the work
    return proof


# far_x_instance (sdfgpu_last_build_info bits 8..12): 1 stage 3 + 2 vector loads + 4 looping form + 8 512 lanes; 13 / 15: the 512- /
# 1024-voxel lines as compile-time constants
FAR = [((9, 10, 40), {}, 3), ((9, 11, 7), {}, 1), ((9, 10, 40), {"i32_handoff": 0}, 3), ((9, 10, 40), {"flat_tiles": 2}, 3),
       ((512, 8, 8), {}, 13), ((512, 8, 8), {"dc_fixed": 0}, 3), ((520, 4, 8), {}, 11), ((1024, 4, 8), {}, 15), ((8, 8, 512), {}, 3)]


@pytest.mark.parametrize("shape,extra,instance", FAR,
                         ids=["%s%s" % ("x".join(map(str, s)), "".join("-%s%d" % kv for kv in e.items())) for s, e, _ in FAR])
def test_far_field_kernel_finish(gpu, shape, extra, instance):
    opts = dict({"dense": 0, "envelope_mode": 1}, **extra)
    sparse = _noise(shape, 0.03, 7)
    scenes_ = [(sparse, False), (1 - sparse, False), (R.corner_voxel(shape), False), (sparse, True)]
    if max(shape) >= 512:
        scenes_ = scenes_[:3]
    for m, vb in scenes_:
        _run_site(gpu, opts, m, vb, _far_proof(instance))


@pytest.mark.parametrize("shape", [(9, 10, 40), (12, 8, 64)], ids=["generic-dense-shape", "tuned-dense-shape"])
@pytest.mark.parametrize("fold", [1, 0])
def test_standby_pair_finish(gpu, shape, fold):
    dense = (np.indices(shape).sum(axis=0) & 1).astype(np.uint8)
    want_dense = O.exact_sdf(dense, 0.05)

    def prepare(g):
        got, ext = g.build(dense, 0.05)                       # a certified dense build, after which the handle trusts its dense tier
        assert g.last_path()["dense_certified"] and np.array_equal(_bits(got), _bits(want_dense[0])) and ext == want_dense[1]
        g.set_option("expect_dense", 1)

    def proof(info, path, dsq):
        assert info["standby_far"] and info["dense"] and not info["fused_zy"], info
        assert info["far_x_instance"] == 7, info             # stage 3, vector loads, the looping form
        assert path["far_y"] and path["far_x"] and not path["dense_certified"], path
    for m, vb in ((_noise(shape, 0.01, 3), False), (R.corner_voxel(shape), False), (1 - R.corner_voxel(shape), False), (R.corner_voxel(shape), True)):
        assert np.abs(O.exact_sdf(m, 1.0, vb)[2]).max() > 8  # (beyond the ball even with the border: the dense tier cannot certify it)
        _run_site(gpu, {"standby_fold": fold}, m, vb, proof, prepare)


# ---- the batched kernel and the host extrema ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("vb", [False, True])
def test_batched_build_mixes_every_class(gpu, vb):
    shape = (9, 10, 40)
    for m in (_noise(shape, 0.03, 5), 1 - _noise(shape, 0.03, 5), _noise(shape, 0.5, 6), R.corner_voxel(shape)):
        _, _, dsq = O.exact_sdf(m, 1.0, vb)
        classes = R.class_resolutions(dsq)
        assert sorted({c for c, _ in classes}) == list("abcdefg")
        order = sorted(range(len(classes)), key=lambda i: (i * 7) % len(classes))        # (c), (e), (f) beside ordinary grids
        res = np.array([classes[i][1] for i in order])
        masks = np.stack([m] * len(res))
        got, ext = gpu.build_batch(masks, res, vb)
        assert gpu.last_batch_info() == (True, 2)
        assert gpu.get_extrema_batch(len(res)) == ext
        for b, r in enumerate(res):
            want, want_ext, _ = O.exact_sdf(m, float(r), vb)
            assert np.array_equal(_bits(got[b]), _bits(want)), (b, r, int((_bits(got[b]) != _bits(want)).sum()))
            assert ext[b] == want_ext, (b, r, ext[b], want_ext)
        for r in (R.SUBNORMAL, R.UNDERFLOW, R.partial_overflow(dsq), 1.0 / 3.0):          # one resolution for the whole batch
            got, ext = gpu.build_batch(masks[:3], r, vb)
            assert gpu.last_batch_info() == (True, 2)
            want, want_ext, _ = O.exact_sdf(m, r, vb)
            for b in range(3):
                assert np.array_equal(_bits(got[b]), _bits(want)) and ext[b] == want_ext, (b, r)


def test_extrema_from_dsq_in_every_class(gpu):
    for D in (1, 2, 3, 8, 15, 16, 17, 63, 64, 1023, 1024, 1025, 262144, 786433):
        dsq = np.array([D, -D, 1, -1], np.int64)
        for res in R.CLASS_A + R.CLASS_B + (R.SUBNORMAL, R.STRADDLE, R.UNDERFLOW, 2.0 ** 125, 2.0 ** 126, 2.0 ** 127, R.TOTAL_OVERFLOW,
                                            5e-324, 1.7976931348623157e308):
            assert capi.extrema_from_dsq(D, D, res) == R.extrema(dsq, res), (D, res)
    assert capi.extrema_from_dsq(0, 5, 1.0 / 3.0) == (-math.inf, 0.0 - math.sqrt(5.0) * (1.0 / 3.0))
    assert capi.extrema_from_dsq(5, capi.SDFGPU_DSQ_INF, 2.0 ** 126) == (math.sqrt(5.0) * 2.0 ** 126, -math.inf)


# ---- the slab stage entry points ----------------------------------------------------------------------------------------------------
def _stage_classes(mask, vb):
    _, _, dsq = O.exact_sdf(mask, 1.0, vb)
    classes = R.class_resolutions(dsq)
    assert sorted({c for c, _ in classes}) == list("abcdefg")
    return classes


@pytest.mark.parametrize("vb", [False, True])
def test_slab_x_sweep_entry_points(gpu, vb):
    s = torch.cuda.current_stream().cuda_stream
    shape = (9, 10, 40)
    nx, ny, nz = shape
    for m in (_noise(shape, 0.03, 5), 1 - R.corner_voxel(shape)):
        dm = torch.from_numpy(m).cuda()
        plane = torch.empty(shape, dtype=torch.int32, device="cuda")
        gpu.sweep_zy_device(dm.data_ptr(), shape, plane.data_ptr(), s)
        for cls, res in _stage_classes(m, vb):
            want, want_ext, _ = O.exact_sdf(m, res, vb)
            for which, opts in (("halo", {}), ("lines", {"envelope": 0}), ("lines", {"envelope_mode": 1})):
                out = torch.full(shape, -7.0, dtype=torch.float32, device="cuda")
                small = torch.zeros(4, dtype=torch.int32, device="cuda")
                try:
                    _set(gpu, opts)
                    if which == "halo":
                        gpu.sweep_x_device(plane.data_ptr(), 0, nx, 0, ny, nz, False, False, 0, nx, res, vb, out.data_ptr(),
                                           small.data_ptr(), small.data_ptr() + 8, s)
                    else:
                        gpu.sweep_x_lines_device(plane.data_ptr(), nx, ny, nz, 0, ny, res, vb, out.data_ptr(), small.data_ptr(), s)
                    torch.cuda.synchronize()
                    info = gpu.last_build_info()
                    if which == "lines":
                        # envelope = 0: the marching sweep alone, unbounded.  envelope_mode = 1: the tier is chosen on the device,
                        # where the forced decision raises the far-field kernel's guard and leaves the marching sweep's down; the
                        # generic vector instance was enqueued for it.  (The stage call clears its status words, so the flag says
                        # "enqueued behind a forced decision", not "ran": that much of this path rests on reading k_decide_tier.)
                        want_info = (True, 3) if opts.get("envelope_mode") else (False, -1)
                        assert (info["lines_tiered"], info["far_x_instance"]) == want_info, (opts, info)
                finally:
                    _restore(gpu, opts)
                mf, mq, status, _ = small.tolist()
                assert status == 0
                assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (which, opts, cls, res)
                assert capi.extrema_from_dsq(mf, mq, res) == want_ext, (which, opts, cls, res)


def test_slab_dense_phase_entry_point(gpu):
    s = torch.cuda.current_stream().cuda_stream
    shape = (13, 9, 64)
    nx, ny, nz = shape
    for m in (R.ball_levels(shape), 1 - R.ball_levels(shape)):
        dm = torch.from_numpy(m).cuda()
        bits = torch.zeros((nx, ny, nz // 32), dtype=torch.int32, device="cuda")
        for cls, res in _stage_classes(m, False):
            want, want_ext, _ = O.exact_sdf(m, res)
            out = torch.full(shape, -7.0, dtype=torch.float32, device="cuda")
            small = torch.full((4,), 7, dtype=torch.int32, device="cuda")
            for phase in (0, 1, 2):
                gpu.slab_dense_phase(phase, dm.data_ptr(), nx, ny, nz, bits.data_ptr(), 0, 0, res, out.data_ptr(), small.data_ptr(), s)
            torch.cuda.synchronize()
            mf, mq, status, uncertified = small.tolist()
            assert status == 0 and uncertified == 0                # KD decided every voxel
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (cls, res)
            assert capi.extrema_from_dsq(mf, mq, res) == want_ext, (cls, res)


# ---- consumers: gradient and query scaling on full-mantissa fields -----------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)
GRAD_SHAPES = [(12, 9, 16), (5, 6, 8), (9, 11, 7)]
# F32SCALE (1 / (2 r) is a float), inside the gate at both ends (1 / (2 r) = 2^98, 2^-99), outside it (2^100 > 1e30, 2^-101 < 1e-30:
# the fp64 scale), and the fp64 class proper.  Around the gate the fp32 products overflow or land in the subnormal range.
GRAD_RES = [0.25, 0.01, 0.05, 2.0 ** -99, 2.0 ** 98, 2.0 ** -101, 2.0 ** 100, 0.03, 1.0 / 3.0]


def _real_field(shape):
    return O.exact_sdf(_noise(shape, 0.3, sum(shape)), 0.05)[0]


def _random_field(shape, seed):
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal(shape) * np.exp2(rng.integers(-20, 21, shape))).astype(np.float32)
    flat = f.reshape(-1)
    n = flat.size
    pick = rng.permutation(n)[:max(12, n // 12)]
    special = np.array([np.inf, -np.inf, -0.0, FLT_MAX, -FLT_MAX, 1e-45, -3e-42, 1.1e-38], np.float32)
    flat[pick] = special[np.arange(pick.size) % special.size]
    nx, ny, nz = shape
    if min(shape) >= 3:                                       # +FLT_MAX and -FLT_MAX across an interior voxel on every axis: the difference overflows
        c = (nx // 2, ny // 2, nz // 2)
        for ax in range(3):
            lo, hi = list(c), list(c)
            lo[ax] -= 1
            hi[ax] += 1
            f[tuple(lo)], f[tuple(hi)] = -FLT_MAX, FLT_MAX
        f[0, 1, 1], f[2, 1, 1] = 1e-40, 3e-40               # two subnormal floats across (1, 1, 1): a subnormal difference
    return f


def _fields(shape):
    return [("sdf", _real_field(shape)), ("random", _random_field(shape, 11 + sum(shape)))]


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=["x".join(map(str, s)) for s in GRAD_SHAPES])
def test_gradient_scaling_on_full_mantissa_fields(gpu, shape):
    rounded = subnormal = overflowed = 0
    for name, f in _fields(shape):
        for res in GRAD_RES:
            for edge in (True, False):
                want = A.grid_gradient(f, res, edge)
                assert _same(_device_gradient(gpu, f, res, edge, True), want), (name, res, edge, "f64")
                with np.errstate(over="ignore", under="ignore"):
                    want32 = want.astype(np.float32)
                for in_shift, out_shift in ((0, 0), (1, 0), (0, 1), (3, 2)):
                    got = _device_gradient(gpu, f, res, edge, False, in_shift, out_shift)
                    assert _same(got, want32), (name, res, edge, in_shift, out_shift, np.argwhere(got.view(np.uint32) != want32.view(np.uint32))[:4].tolist())
                fin = np.isfinite(want)
                rounded += int((want32[fin].astype(np.float64) != want[fin]).sum())
                subnormal += int(((np.abs(want32) > 0) & (np.abs(want32) < R.FLT_MIN)).sum())
                overflowed += int((np.isinf(want32) & fin).sum())
    # the inputs do what they are here for: products that are rounded, that land in the subnormal range, that overflow in fp32 only
    assert rounded > 0 and overflowed > 0 and subnormal > 0, (rounded, subnormal, overflowed)


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=["x".join(map(str, s)) for s in GRAD_SHAPES])
def test_gradient_batch_equals_the_single_call(gpu, shape):
    fields = [f for _, f in _fields(shape)] + [_random_field(shape, 5)]
    B, n = len(fields), int(np.prod(shape))
    d_in = torch.from_numpy(np.stack(fields)).cuda()
    for res in ([0.25, 2.0 ** -99, 1.0 / 3.0], [2.0 ** 100, 0.01, 2.0 ** 98], [0.03, 2.0 ** -101, 0.05], 2.0 ** -99, 1.0 / 3.0):
        for edge in (True, False):
            for f64 in (True, False):
                out = torch.full((B * 3 * n,), -7.0, dtype=torch.float64 if f64 else torch.float32, device="cuda")
                gpu.gradient_batch_device(d_in.data_ptr(), B, shape, out.data_ptr(), np.array(res) if np.ndim(res) else res, edge, f64)
                torch.cuda.synchronize()
                got = out.cpu().numpy().reshape((B,) + shape + (3,))
                for b in range(B):
                    r = res[b] if np.ndim(res) else res
                    assert _same(got[b], _device_gradient(gpu, fields[b], r, edge, f64)), (res, edge, f64, b)


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=["x".join(map(str, s)) for s in GRAD_SHAPES])
def test_point_query_gradient_equals_the_full_grid_kernel(gpu, shape):
    n = int(np.prod(shape))
    cells = np.stack(np.unravel_index(np.arange(n), shape), axis=1).astype(np.float64)
    for name, f in _fields(shape):
        d_f = torch.from_numpy(f).cuda()
        for res in GRAD_RES:
            pts = torch.from_numpy((cells + 0.5) * res).cuda()                       # every cell centre
            for edge in (True, False):
                g = torch.full((n, 3), -7.0, dtype=torch.float64, device="cuda")
                fl = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
                gpu.query_points_device(d_f.data_ptr(), shape, res, pts.data_ptr(), n, 0, g.data_ptr(), fl.data_ptr(), None, None,
                                        math.inf, edge)
                torch.cuda.synchronize()
                full = _device_gradient(gpu, f, res, edge, True).reshape(n, 3)
                with np.errstate(invalid="ignore"):
                    # the kernel's identity rotation, product by product (0 * inf = NaN, as there)
                    want = np.stack([1.0 * full[:, 0] + 0.0 * full[:, 1] + 0.0 * full[:, 2],
                                     0.0 * full[:, 0] + 1.0 * full[:, 1] + 0.0 * full[:, 2],
                                     0.0 * full[:, 0] + 0.0 * full[:, 1] + 1.0 * full[:, 2]], axis=1)
                want[fl.cpu().numpy() != 3] = np.nan
                got = g.cpu().numpy()
                shell = np.ones(shape, bool)
                shell[1:-1, 1:-1, 1:-1] = False
                expect_flags = np.where(edge | ~shell.reshape(-1), 3, 1)        # bit 0: inside the grid, bit 1: the cell has a gradient
                assert np.array_equal(fl.cpu().numpy(), expect_flags), (name, res, edge)
                nan_both = np.isnan(got) & np.isnan(want)
                assert bool(np.all((got.view(np.uint64) == want.view(np.uint64)) | nan_both)), (name, res, edge)


QUERY_RES = GRAD_RES                                          # (all of them positive and finite: none is refused)


def _same_or_nan(a, b):
    """bitwise, NaN == NaN (the host core and the device give a NaN different sign bits: inf - inf on x86 and on the GPU)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float64:
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("res", QUERY_RES, ids=[repr(r) for r in QUERY_RES])
def test_interpolated_gradients_and_projection_on_the_same_fields(res):
    """sdfgpu_query_gradients* (smooth, autodiff, distance to boundary) and sdfgpu_project_points* against the host core on the
    downloaded field -- the fixtures of test_gpu_query_gradients.py / test_gpu_projection.py (_field, _points, the host core's
    QueryGradientsNumpyHost / ProjectOutOfCollisionNumpyHost) -- in the identity frame and a pure translation, where those tests
    claim bit equality, at resolutions of every class these entry points accept.  The fields hold +-inf, so results hold NaN:
    compared as NaN == NaN, every other value bitwise."""
    import test_gpu_projection as P
    import test_gpu_query_gradients as Q
    assert Q.KINDS == [capi.QUERY_SMOOTH_GRADIENT, capi.QUERY_AUTODIFF_GRADIENT, capi.QUERY_DISTANCE_TO_BOUNDARY]
    from test_projection_cpu import inverse, rigid
    ctx = capi.SdfGpu(0)
    try:
        shape = (12, 9, 16)
        mask = _noise(shape, 0.3, sum(shape))
        for name, f in _fields(shape):
            for origin in (np.eye(4), rigid(0.0, (3.0 * res, -2.0 * res, 0.5 * res))):
                d, ptr, host = P._field(ctx, f, res, origin)
                pts = P._points(f, res, origin, mask, 300, 3)
                for kind in Q.KINDS:
                    for window in ([res / 8, res, 3 * res] if kind == capi.QUERY_SMOOTH_GRADIENT else [0.0]):
                        want = host.QueryGradientsNumpyHost(pts, kind, window)
                        for got in (d.QueryGradientsBatch(pts, kind, window), ctx.query_gradients(ptr, shape, res, pts, inverse(origin), kind, window)):
                            for k, what in enumerate(("value", "gradient", "status")):
                                assert _same_or_nan(got[k], want[k]), (name, what, kind, window, int((np.asarray(got[k]) != np.asarray(want[k])).sum()))
                for valid_only in (False, True):
                    for md, mult in ((0.0, 0.125), (1.5 * res, 0.5)):
                        want = host.ProjectOutOfCollisionNumpyHost(pts, md, mult, 0, valid_only)
                        for got in (d.ProjectBatch(pts, md, mult, 0, valid_only), ctx.project_points(ptr, shape, res, pts, inverse(origin), origin, md, mult, 0, valid_only)):
                            for k, what in enumerate(("location", "status", "steps")):
                                assert _same_or_nan(got[k], want[k]), (name, what, md, mult, valid_only, int((np.asarray(got[k]) != np.asarray(want[k])).sum()))
    finally:
        ctx.close()


# ---- one rule for resolutions that are refused --------------------------------------------------------------------------------------
BAD = [math.nan, 0.0, -1.0, math.inf]


def _entry_points(gpu):
    """name -> call(resolution) for every entry point that takes a resolution, on small valid arguments; a call returns the device
    tensors it was given to write to (filled with -7 / 0xEE beforehand)."""
    s = torch.cuda.current_stream().cuda_stream
    shape = (6, 5, 32)
    nx, ny, nz = shape
    n = nx * ny * nz
    m = _noise(shape, 0.3, 1)
    dm = torch.from_numpy(m).cuda()
    cells = np.zeros(shape + (2,), np.float32)
    cells[..., 0] = m
    dcells = torch.from_numpy(cells).cuda()
    tagged = np.zeros(shape + (4,), np.uint32)
    tagged[..., 0] = np.where(m != 0, np.float32(1.0).view(np.uint32), 0)       # TAGGED_OBJECT_COLLISION_CELL: occupancy, component, object id, segment
    tagged[..., 2] = 1
    bits = capi.pack_bits_host(m)
    dbits = torch.from_numpy(bits.view(np.int32)).cuda()
    field = O.exact_sdf(m, 0.05)[0]
    dfield = torch.from_numpy(field).cuda()
    plane = torch.zeros(shape, dtype=torch.int32, device="cuda")
    wbits = torch.zeros((nx, ny, nz // 32), dtype=torch.int32, device="cuda")
    pts_h = (np.random.default_rng(0).random((7, 3)) * np.array(shape) * 0.05)
    pts = torch.from_numpy(pts_h).cuda()
    pts32 = torch.from_numpy(pts_h.astype(np.float32)).cuda()
    eye = np.eye(4)

    def out(*shp, dtype=torch.float32):
        return torch.full(shp, 0xEE if dtype == torch.uint8 else -7, dtype=dtype, device="cuda")

    def per_grid(r):
        return np.array([0.05, 0.1, r])

    def dev(fn, *tensors):
        def call(r):
            fn(r, *tensors)
            return tensors
        return call
    masks3 = np.stack([m] * 3)
    dmasks3 = torch.from_numpy(masks3).cuda()
    dfield3 = torch.from_numpy(np.stack([field] * 3)).cuda()
    E = {
        "sdfgpu_build": lambda r: gpu.build(m, r),
        "sdfgpu_build_cells": lambda r: gpu.build_cells(cells, shape, 8, 0, False, r),
        "sdfgpu_build_tagged_cells": lambda r: gpu.build_tagged_cells(tagged, shape, 0, (), False, r),
        "sdfgpu_build_bits": lambda r: gpu.build_bits(bits, shape, r),
        "sdfgpu_build_to_device": dev(lambda r, o: gpu.build_to_device(m, o.data_ptr(), r), out(n)),
        "sdfgpu_build_cells_to_device": dev(lambda r, o: gpu._check(gpu._lib.sdfgpu_build_cells_to_device(
            gpu._h, cells.ctypes.data, 8, 0, 0, nx, ny, nz, float(r), 0, ctypes.c_void_p(o.data_ptr()), None, None)), out(n)),
        "sdfgpu_build_device": dev(lambda r, o: gpu.build_device(dm.data_ptr(), shape, o.data_ptr(), r, False, s), out(n)),
        "sdfgpu_build_cells_device": dev(lambda r, o: gpu.build_cells_device(dcells.data_ptr(), shape, o.data_ptr(), 8, 0, False, r, False, s), out(n)),
        "sdfgpu_build_bits_device": dev(lambda r, o: gpu.build_bits_device(dbits.data_ptr(), shape, o.data_ptr(), r, False, s), out(n)),
        "sdfgpu_build_batch": lambda r: gpu.build_batch(masks3, r),
        "sdfgpu_build_batch (per grid)": lambda r: gpu.build_batch(masks3, per_grid(r)),
        "sdfgpu_build_batch_device": dev(lambda r, o: gpu.build_batch_device(dmasks3.data_ptr(), 3, shape, o.data_ptr(), r, False, s), out(3 * n)),
        "sdfgpu_build_batch_device (per grid)": dev(lambda r, o: gpu.build_batch_device(dmasks3.data_ptr(), 3, shape, o.data_ptr(), per_grid(r), False, s), out(3 * n)),
        "sdfgpu_build_tagged_objects": lambda r: gpu.build_tagged_objects(tagged, shape, [1, 2], False, r),
        "sdfgpu_gradient": lambda r: gpu.gradient(field, r),
        "sdfgpu_gradient_device": dev(lambda r, o: gpu.gradient_device(dfield.data_ptr(), shape, o.data_ptr(), r, True, False, s), out(3 * n)),
        "sdfgpu_gradient_batch_device": dev(lambda r, o: gpu.gradient_batch_device(dfield3.data_ptr(), 3, shape, o.data_ptr(), r, True, False, s), out(9 * n)),
        "sdfgpu_gradient_batch_device (per grid)": dev(lambda r, o: gpu.gradient_batch_device(dfield3.data_ptr(), 3, shape, o.data_ptr(), per_grid(r), True, False, s), out(9 * n)),
        "sdfgpu_query_points": lambda r: gpu.query_points(dfield.data_ptr(), shape, r, pts_h),
        "sdfgpu_query_points_device": dev(lambda r, a, b, c: gpu.query_points_device(dfield.data_ptr(), shape, r, pts.data_ptr(), 7, a.data_ptr(), b.data_ptr(), c.data_ptr(), None, None, math.inf, True, s),
                                          out(7, dtype=torch.float64), out(21, dtype=torch.float64), out(7, dtype=torch.uint8)),
        "sdfgpu_voxelize_points_device": dev(lambda r, o: gpu.voxelize_points_device(pts32.data_ptr(), 7, (0.0, 0.0, 0.0), r, shape, o.data_ptr(), True, s), out(n, dtype=torch.uint8)),
        "sdfgpu_voxelize_points_bits_device": dev(lambda r, o: gpu.voxelize_points_bits_device(pts32.data_ptr(), 7, (0.0, 0.0, 0.0), r, shape, o.data_ptr(), True, s), out((n + 31) // 32, dtype=torch.int32)),
        "sdfgpu_sweep_x_device": dev(lambda r, o, sm: gpu.sweep_x_device(plane.data_ptr(), 0, nx, 0, ny, nz, False, False, 0, nx, r, False, o.data_ptr(), sm.data_ptr(), sm.data_ptr() + 8, s),
                                     out(n), out(4, dtype=torch.int32)),
        "sdfgpu_sweep_x_lines_device": dev(lambda r, o, sm: gpu.sweep_x_lines_device(plane.data_ptr(), nx, ny, nz, 0, ny, r, False, o.data_ptr(), sm.data_ptr(), s),
                                           out(n), out(4, dtype=torch.int32)),
        "sdfgpu_slab_dense_phase": dev(lambda r, o, sm: [gpu.slab_dense_phase(p, dm.data_ptr(), nx, ny, nz, wbits.data_ptr(), 0, 0, r, o.data_ptr(), sm.data_ptr(), s) for p in (0,)],
                                       out(n), out(4, dtype=torch.int32)),
        "sdfgpu_dense_ball_device": dev(lambda r, o, sm: gpu.dense_ball_device(wbits.data_ptr(), nx, 0, nx, ny, nz, r, o.data_ptr(), sm.data_ptr(), sm.data_ptr() + 12, s),
                                        out(n), out(4, dtype=torch.int32)),
        "sdfgpu_local_extrema": lambda r: gpu.local_extrema(field, r),
        "sdfgpu_local_extrema_device": dev(lambda r, o: gpu.local_extrema_device(dfield.data_ptr(), shape, r, o.data_ptr(), (1.0, 0.0, 0.0, 0.0), s), out(n, dtype=torch.int32)),
        "sdfgpu_convex_segments_cells": lambda r: gpu.convex_segments_cells(tagged.copy(), shape, r, 0.1, False),
        "sdfgpu_project_points": lambda r: gpu.project_points(dfield.data_ptr(), shape, r, pts_h, eye, eye),
        "sdfgpu_project_points_device": dev(lambda r, o: gpu.project_points_device(dfield.data_ptr(), shape, r, pts.data_ptr(), 7, o.data_ptr(), eye, eye, stream=s), out(21, dtype=torch.float64)),
        "sdfgpu_query_gradients": lambda r: gpu.query_gradients(dfield.data_ptr(), shape, r, pts_h, eye, capi.QUERY_AUTODIFF_GRADIENT),
        "sdfgpu_query_gradients_device": dev(lambda r, o: gpu.query_gradients_device(dfield.data_ptr(), shape, r, pts.data_ptr(), 7, eye, capi.QUERY_AUTODIFF_GRADIENT, 0.0, math.inf, o.data_ptr(), 0, 0, s),
                                             out(7, dtype=torch.float64)),
    }
    return E, m


def test_bad_resolutions_are_refused_by_every_entry_point(gpu):
    E, m = _entry_points(gpu)
    want, want_ext, _ = O.exact_sdf(m, 0.05)
    # every symbol of the header whose signature holds a resolution is in the table (the two debug / helper calls apart)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))), "include", "sdfgpu.h")).read()
    declared = set(re.findall(r"\bint (sdfgpu_\w+)\([^;]*?double resolution[^;]*?;", header, re.S))
    assert declared - {"sdfgpu_extrema_from_dsq", "sdfgpu_debug_finish_table"} == {k.split(" ")[0] for k in E}, declared ^ {k.split(" ")[0] for k in E}
    for name, call in E.items():
        for r in BAD:
            with pytest.raises(capi.SdfGpuError) as e:
                call(r)
            assert e.value.code == -1, (name, r, e.value)
            message = str(e.value).split(": ", 1)[1]
            assert message and "resolution" in message, (name, r, str(e.value))
        # (a valid call of the same entry point, so that the outputs below are known to be written by it when it is accepted)
        tensors = call(0.05)
        torch.cuda.synchronize()
        if isinstance(tensors, tuple) and tensors and all(isinstance(t, torch.Tensor) for t in tensors):
            assert any(bool((t != (0xEE if t.dtype == torch.uint8 else -7)).any().item()) for t in tensors), name
            for t in tensors:
                t.fill_(0xEE if t.dtype == torch.uint8 else -7)
            for r in BAD:
                with pytest.raises(capi.SdfGpuError):
                    call(r)
            torch.cuda.synchronize()
            for t in tensors:                                   # refused before anything is enqueued: nothing was written
                assert bool((t == (0xEE if t.dtype == torch.uint8 else -7)).all().item()), name
        got, ext = gpu.build(m, 0.05)                           # the handle builds a correct field right after
        assert np.array_equal(_bits(got), _bits(want)) and ext == want_ext, name
    for r in BAD:                                               # no handle: the code only
        with pytest.raises(capi.SdfGpuError) as e:
            capi.extrema_from_dsq(4, 9, r)
        assert e.value.code == -1
    # subnormal and huge finite resolutions stay valid
    for r in (5e-324, 2.0 ** -160, 1.7976931348623157e308):
        got, ext = gpu.build(m, r)
        w, we, _ = O.exact_sdf(m, r)
        assert np.array_equal(_bits(got), _bits(w)) and ext == we, r


@pytest.mark.parametrize("world", [1, 3])
def test_bad_resolutions_are_refused_by_the_multi_gpu_entry_points(world):
    """include/sdfgpu_multi.h: the same rule, before anything is uploaded, enqueued or written on any rank (every rank on device 0)."""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))), "include", "sdfgpu_multi.h")).read()
    declared = set(re.findall(r"\bint (sdfgpu_\w+)\([^;]*?double resolution[^;]*?;", header, re.S))
    assert declared == {"sdfgpu_multi_build", "sdfgpu_multi_build_cells", "sdfgpu_multi_build_device"}, declared
    shape = (12, 5, 32)
    m = _noise(shape, 0.3, 2)
    want, want_ext, _ = O.exact_sdf(m, 0.05)
    cells = np.zeros(shape + (2,), np.float32)
    cells[..., 0] = m
    mg = capi.MultiSdfGpu(world, [0] * world)
    try:
        ranges = [mg.slab_range(shape[0], r) for r in range(world)]
        d_mask = [torch.from_numpy(m[a:b]).cuda() for a, b in ranges]
        d_out = [torch.full((b - a,) + shape[1:], -7.0, dtype=torch.float32, device="cuda") for a, b in ranges]
        calls = {
            "sdfgpu_multi_build": lambda r: mg.build(m, r),
            "sdfgpu_multi_build_cells": lambda r: mg.build_cells(cells, shape, 8, 0, False, r),
            "sdfgpu_multi_build_device": lambda r: mg.build_device([t.data_ptr() for t in d_mask], shape, [t.data_ptr() for t in d_out], r),
        }
        assert set(calls) == declared
        for name, call in calls.items():
            for r in BAD:
                with pytest.raises(capi.SdfGpuError) as e:
                    call(r)
                assert e.value.code == -1, (name, r, e.value)
                assert "resolution" in str(e.value).split(": ", 1)[1], (name, r, str(e.value))
            torch.cuda.synchronize()
            assert all(bool((t == -7.0).all().item()) for t in d_out), name          # nothing was written
            got, ext = mg.build(m, 0.05)                       # the handle builds a correct field right after
            assert np.array_equal(_bits(got), _bits(want)) and ext == want_ext, name
        ext = mg.build_device([t.data_ptr() for t in d_mask], shape, [t.data_ptr() for t in d_out], 0.05)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(np.concatenate([t.cpu().numpy() for t in d_out])), _bits(want)) and ext == want_ext
        for r in (2.0 ** -160, 1.0 / 3.0, 2.0 ** 126):        # subnormal results, signed zeros and partial overflow stay valid here too
            got, ext = mg.build(m, r)
            w, we, _ = O.exact_sdf(m, r)
            assert np.array_equal(_bits(got), _bits(w)) and ext == we, r
    finally:
        mg.close()
