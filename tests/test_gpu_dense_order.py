"""GPU: the dense ball kernel's serpentine tile order (option ball_serpentine: a whole build that rewrites the buffer of
the build before it walks the tiles the other way round).  It may not change a bit: every build is compared with the
exact oracle and with a fresh context's first build.  (The compile-time instance of the kernel that was measured beside
it did not earn its place -- LAB_NOTES.md -- so there is no `dense_fixed` option to test.)"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from sdf_tools_amd import capi, synth

pytestmark = pytest.mark.gpu


def _build(ctx, m_t, out, res, vb=False):
    shape = tuple(m_t.shape)
    ctx.build_device(m_t.data_ptr(), shape, out.data_ptr(), res, vb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ctx.get_extrema()


def _fresh(m_t, res, vb=False):
    """What a fresh context's first build (never flipped, nothing learnt) returns."""
    ctx = capi.SdfGpu(0)
    try:
        out = torch.empty(tuple(m_t.shape), dtype=torch.float32, device="cuda")
        return _build(ctx, m_t, out, res, vb)
    finally:
        ctx.close()


def _same(got, want):
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


# 512-voxel lines (4 x 4-row tiles), 1024 (2 x 4), 64 (8 x 16); nx and ny are not multiples of the tile, so the flipped
# walk starts on the partial tiles
ORDER_SHAPES = [(10, 13, 512), (16, 16, 512), (5, 9, 1024), (21, 37, 64), (1, 6, 512)]


@pytest.mark.parametrize("vb", [False, True], ids=["plain", "virtual_border"])
@pytest.mark.parametrize("shape", ORDER_SHAPES, ids=["x".join(map(str, s)) for s in ORDER_SHAPES])
def test_rebuilding_into_one_buffer_is_exact_in_both_directions(gpu, shape, vb):
    """Six builds in a row into one buffer on one handle (both directions, three times), then another buffer, then the
    first one again.  The scenes alternate, so a tile that a flipped walk missed would keep the other scene's values."""
    res = 0.05
    masks = [synth.bernoulli_mask(shape, 0.5, 41 + k) for k in range(2)]
    want = [O.exact_sdf(m, res, vb)[:2] for m in masks]
    m_t = [torch.from_numpy(m).cuda() for m in masks]
    first = [_fresh(t, res, vb) for t in m_t]
    for k in range(2):
        assert _same(first[k][0], want[k][0]) and first[k][1] == want[k][1]
    a = torch.empty(shape, dtype=torch.float32, device="cuda")
    b = torch.empty(shape, dtype=torch.float32, device="cuda")
    for i, buf in enumerate([a] * 6 + [b, a, a]):
        k = i & 1
        buf.fill_(float("nan"))
        sdf, ext = _build(gpu, m_t[k], buf, res, vb)
        assert _same(sdf, want[k][0]), (i, int((sdf.view(np.uint32) != want[k][0].view(np.uint32)).sum()))
        assert _same(sdf, first[k][0])
        assert ext == want[k][1] == first[k][1], i
        assert gpu.last_build_info()["dense"] and gpu.last_dense_certified()


def test_fixup_words_and_tile_flags_under_the_flipped_order(gpu):
    """Bernoulli p = 0.1 leaves a few voxels beyond the ball: KD writes their `unc` words and raises tile flags, which the
    fix-up kernel behind it finds by LOGICAL tile coordinates.  KD + KF forced (dense3 = 0, fixup_mode), and the default
    policy (KD, then the wide stage on its verdict); each three times into one buffer."""
    res = 0.05
    for shape in ((14, 18, 512), (40, 36, 64)):
        m = synth.bernoulli_mask(shape, 0.1, 21)
        ex, ex_ext, dsq = O.exact_sdf(m, res)
        assert np.abs(dsq).max() > 8
        m_t = torch.from_numpy(m).cuda()
        first = _fresh(m_t, res)
        assert _same(first[0], ex) and first[1] == ex_ext
        out = torch.empty(shape, dtype=torch.float32, device="cuda")
        for forced in (True, False):
            gpu.set_option("policy_reset", 1)
            try:
                if forced:
                    gpu.set_option("dense3", 0)
                    gpu.set_option("fixup_mode", 1)
                for i in range(3):
                    out.fill_(float("nan"))
                    sdf, ext = _build(gpu, m_t, out, res)
                    assert _same(sdf, ex) and _same(sdf, first[0]), (shape, forced, i)
                    assert ext == ex_ext
                    if forced:
                        info = gpu.last_build_info()
                        assert info["dense"] and not info["dense3"] and gpu.last_dense_certified()
            finally:
                gpu.set_option("dense3", 1)
                gpu.set_option("policy_reset", 1)


def test_sparse_scene_rewritten_by_the_stage_behind(gpu):
    """A scene that raises `uncertified`: the early out leaves most tiles untouched and the pipeline behind rewrites the
    field -- twice into one buffer (the second walk is flipped), exact both times."""
    res = 0.1
    for shape in ((12, 14, 512), (24, 20, 64)):
        m = synth.bernoulli_mask(shape, 0.002, 9)
        ex, ex_ext, _ = O.exact_sdf(m, res)
        m_t = torch.from_numpy(m).cuda()
        first = _fresh(m_t, res)
        assert _same(first[0], ex) and first[1] == ex_ext
        out = torch.empty(shape, dtype=torch.float32, device="cuda")
        gpu.set_option("dense3", 0)                      # (KD alone in front of the sweeps)
        try:
            for i in range(2):
                out.fill_(float("nan"))
                sdf, ext = _build(gpu, m_t, out, res)
                assert _same(sdf, ex) and _same(sdf, first[0]) and ext == ex_ext, (shape, i)
                assert gpu.last_build_info()["dense"] and not gpu.last_dense_certified()
        finally:
            gpu.set_option("dense3", 1)
            gpu.set_option("policy_reset", 1)


def test_the_option_changes_no_bit_and_no_path(gpu):
    """ball_serpentine off against on, on the same inputs and the same sequence of buffers: identical fields, extrema and
    last_path()."""
    option = "ball_serpentine"
    res = 0.02
    for shape, p in (((10, 13, 512), 0.5), ((5, 9, 1024), 0.5), ((21, 37, 64), 0.5), ((14, 18, 512), 0.1)):
        m = synth.bernoulli_mask(shape, p, 5)
        ex, ex_ext, _ = O.exact_sdf(m, res)
        m_t = torch.from_numpy(m).cuda()
        out = torch.empty(shape, dtype=torch.float32, device="cuda")
        seen = {}
        try:
            for value in (0, 1):
                gpu.set_option(option, value)
                gpu.set_option("policy_reset", 1)
                runs = []
                for i in range(4):
                    out.fill_(float("nan"))
                    sdf, ext = _build(gpu, m_t, out, res)
                    assert _same(sdf, ex) and ext == ex_ext, (shape, p, value, i)
                    runs.append((sdf, ext, gpu.last_path(), gpu.last_build_info()))
                seen[value] = runs
        finally:
            gpu.set_option(option, 1)
            gpu.set_option("policy_reset", 1)
        for r0, r1 in zip(seen[0], seen[1]):
            assert _same(r0[0], r1[0]) and r0[1] == r1[1] and r0[2] == r1[2] and r0[3] == r1[3]
