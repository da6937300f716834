"""GPU: the dense ball kernels with their bookkeeping in front of the stores (KD, KD3: the early-out word read beside the tile
loads, the flag read again and the maxima slot read behind the staging barrier, reductions / flags / slot update in front of the
expansion) and slot_max2's single 8-byte read.  Nothing may change: every field is compared bit for bit with the exact oracle and
every pair of extrema with the oracle's."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from sdf_tools_amd import capi, synth

pytestmark = pytest.mark.gpu

RES = 0.05


def _same(got, want):
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _build(ctx, m_t, out, vb=False, res=RES):
    out.fill_(float("nan"))
    ctx.build_device(m_t.data_ptr(), tuple(m_t.shape), out.data_ptr(), res, vb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ctx.get_extrema()


@functools.lru_cache(maxsize=None)
def _noise(shape, p, seed, vb=False):
    """(mask, exact field, exact extrema, signed d^2) -- computed once per scene."""
    m = synth.bernoulli_mask(shape, p, seed)
    sdf, ext, dsq = O.exact_sdf(m, RES, vb)
    for a in (m, sdf, dsq):
        a.setflags(write=False)
    return m, sdf, ext, dsq


# nz = 512: 2 x 2 tiles of 4 x 4 rows; nz = 128: 2 x 3 tiles of 8 x 8 rows; (12, 20, 128): partial tiles, the bounds-checked
# expansion; nz = 32 and 64: the narrow staging path
CERTIFIED_SHAPES = [(8, 8, 512), (16, 24, 128), (12, 20, 128), (32, 32, 32), (16, 16, 64)]


@pytest.mark.parametrize("vb", [False, True], ids=["plain", "virtual_border"])
@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("shape", CERTIFIED_SHAPES, ids=["x".join(map(str, s)) for s in CERTIFIED_SHAPES])
def test_certified_scene_three_builds_into_one_buffer(shape, seed, vb):
    """A fresh context's first build, then the second and the third into the same buffer (the second walks the tiles the other
    way round)."""
    m, want, want_ext, dsq = _noise(shape, 0.5, seed, vb)
    assert np.abs(dsq).max() <= 8
    m_t = torch.from_numpy(m).cuda()
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    ctx = capi.SdfGpu(0)
    try:
        for i in range(3):
            sdf, ext = _build(ctx, m_t, out, vb)
            assert _same(sdf, want), (i, int((sdf.view(np.uint32) != want.view(np.uint32)).sum()))
            assert ext == want_ext, (i, ext, want_ext)
            assert ctx.last_build_info()["dense"] and ctx.last_dense_certified(), i
    finally:
        ctx.close()


def _half_empty(shape):
    """x < nx / 2 empty; the other half holds filled voxels on a lattice of pitch 4 (no two within distance 3), so every filled
    voxel has a free face neighbour: the filled maximum is d^2 = 1 exactly, and the free one lies deep in the empty half."""
    m = np.zeros(shape, np.uint8)
    m[shape[0] // 2 + 1::4, 1::4, 1::4] = 1
    assert m.sum() > 0
    return m


@pytest.mark.parametrize("shape", [(16, 24, 128), (8, 8, 512)], ids=["16x24x128", "8x8x512"])
def test_voided_maxima_never_leave_a_partly_staged_tile(gpu, shape):
    """The handle trusts its dense tier (expect_dense = 1: KD with the early out, the stand-by pair behind it), the scene makes KD
    give up in its first workgroups.  A wave that ran on over a tile its siblings left half staged finds garbage; nothing of it
    may reach the maxima.  Twenty builds into one buffer."""
    m = _half_empty(shape)
    want, want_ext, dsq = O.exact_sdf(m, RES)
    assert -dsq.min() == 1 and dsq.max() > 8
    m_t = torch.from_numpy(m).cuda()
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    try:
        for i in range(20):
            gpu.set_option("policy_reset", 1)
            gpu.set_option("expect_dense", 1)
            sdf, ext = _build(gpu, m_t, out)
            assert _same(sdf, want), (i, int((sdf.view(np.uint32) != want.view(np.uint32)).sum()))
            assert ext == want_ext, (i, ext, want_ext)
            assert not gpu.last_dense_certified(), i
    finally:
        gpu.set_option("policy_reset", 1)


@pytest.mark.parametrize("dense3", [0, 1], ids=["KD_KF", "KD3_KD6_KF"])
def test_fixup_mode_is_exact(gpu, dense3):
    """Bernoulli p = 0.1 leaves voxels beyond the ball: KD (dense3 = 0) or KD3 with the shell pass (dense3 = 1) writes their
    undecided words and tile flags in front of its stores now; the fix-up kernel behind finds them."""
    shape = (32, 32, 128)
    m, want, want_ext, dsq = _noise(shape, 0.1, 21)
    assert np.abs(dsq).max() > 8
    m_t = torch.from_numpy(m).cuda()
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    try:
        for i in range(3):
            gpu.set_option("dense3", dense3)
            gpu.set_option("fixup_mode", 1)
            sdf, ext = _build(gpu, m_t, out)
            assert _same(sdf, want), (i, int((sdf.view(np.uint32) != want.view(np.uint32)).sum()))
            assert ext == want_ext, (i, ext, want_ext)
            info = gpu.last_build_info()
            assert info["dense"] and info["dense3"] == bool(dense3), (i, info)
    finally:
        gpu.set_option("dense3", 1)
        gpu.set_option("policy_reset", 1)


def test_default_policy_reaches_the_wide_form_and_stays_exact(gpu):
    """Bernoulli p = 0.03 through the default policy, build after build until the wide kernel (KD3: guarded behind KD in the same
    build, or in KD's place) has run; every build exact."""
    shape = (32, 32, 128)
    m, want, want_ext, _ = _noise(shape, 0.03, 5)
    m_t = torch.from_numpy(m).cuda()
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    wide = []
    try:
        for i in range(8):
            sdf, ext = _build(gpu, m_t, out)
            assert _same(sdf, want), (i, int((sdf.view(np.uint32) != want.view(np.uint32)).sum()))
            assert ext == want_ext, (i, ext, want_ext)
            info = gpu.last_build_info()
            wide.append((info["dense3_staged"], info["dense3"]))
            if any(s for s, _ in wide) and any(d for _, d in wide):
                break
    finally:
        gpu.set_option("policy_reset", 1)
    assert any(s or d for s, d in wide), wide


def test_stage_entry_point_without_early_out(gpu):
    """KD the way the slab builder launches it: no early out, no reason word, planes [8, 24) of a 32-plane bit buffer -- 16 x 24 x
    128 output planes with one tile (8 planes) of halo on each side -- against the whole-grid build and the oracle."""
    shape = (32, 24, 128)
    nx, ny, nz = shape
    lo, hi = 8, 24
    m, want, want_ext, dsq = _noise(shape, 0.5, 31)
    m_t = torch.from_numpy(m).cuda()
    whole = torch.empty(shape, dtype=torch.float32, device="cuda")
    sdf, ext = _build(gpu, m_t, whole)
    assert _same(sdf, want) and ext == want_ext
    s = torch.cuda.current_stream().cuda_stream
    bits = torch.zeros((nx, ny, nz // 32), dtype=torch.int32, device="cuda")
    gpu.pack_bits_device(m_t.data_ptr(), nx * ny, nz, bits.data_ptr(), s)
    for i in range(2):
        out = torch.full((hi - lo, ny, nz), float("nan"), dtype=torch.float32, device="cuda")
        small = torch.zeros(4, dtype=torch.int32, device="cuda")
        gpu.dense_ball_device(bits.data_ptr(), nx, lo, hi, ny, nz, RES, out.data_ptr(), small.data_ptr(), small.data_ptr() + 12, s)
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy(), sdf[lo:hi]), i
        got = small.cpu().numpy()
        assert (int(got[0]), int(got[1]), int(got[3])) == (int(dsq[lo:hi].max()), int(-dsq[lo:hi].min()), 0), (i, got)
