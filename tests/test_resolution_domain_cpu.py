"""CPU: the oracle at the ends of the resolution domain.  O.exact_sdf and O.reference_sdf, the two checkers of every GPU parity
test, against the plain numpy restatement sign * float32(sqrt(float64(|d^2|)) * res) (resolution_domain.finish) at resolutions
whose results are subnormal floats, signed zeros, partly or wholly infinite, and at doubles that no float holds -- so that the GPU
cases of test_gpu_resolution_domain.py compare against something that is itself pinned there.  Each case also asserts, from the
reference alone, that it exercises the edge it is named for (counts of subnormal / -0.0 / inf voxels).  Tolerance: none."""
import numpy as np
import pytest

import resolution_domain as R
import scenes
from oracle import oracle as O
from sdf_tools_amd import synth

MASKS = {
    "sparse 0.03": synth.bernoulli_mask((9, 10, 40), 0.03, 5),
    "dense 0.5": synth.bernoulli_mask((9, 10, 40), 0.5, 6),
    "single voxel": scenes.single_voxel((9, 10, 40), (1, 2, 3)),
    "inverse corner voxel": 1 - R.corner_voxel((7, 5, 33)),
    "ball levels": R.ball_levels((13, 11, 40)),
}
FIXED = [("a", r) for r in R.CLASS_A] + [("b", r) for r in R.CLASS_B] + [
    ("c", R.SUBNORMAL), ("d", R.STRADDLE), ("e", R.UNDERFLOW), ("f", None), ("g", R.TOTAL_OVERFLOW)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(MASKS))
@pytest.mark.parametrize("cls,res", FIXED, ids=["%s-%s" % (c, "per-scene" if r is None else repr(r)) for c, r in FIXED])
def test_oracles_equal_the_plain_restatement(name, cls, res):
    m = MASKS[name]
    assert 0 < m.sum() < m.size
    _, _, dsq = O.exact_sdf(m, 1.0)
    if res is None:
        res = R.partial_overflow(dsq)                        # chosen per scene, from the integer distances
    want, want_ext = R.finish(dsq, res), R.extrema(dsq, res)
    for vb in (False, True):
        ex, ex_ext, d = O.exact_sdf(m, res, vb)
        assert np.array_equal(_bits(ex), _bits(R.finish(d, res))), (name, res, vb)
        assert ex_ext == R.extrema(d, res), (name, res, vb, ex_ext)
    ex, ex_ext, _ = O.exact_sdf(m, res)
    assert np.array_equal(_bits(ex), _bits(want)) and ex_ext == want_ext
    # the reference algorithm, restated from ITS OWN two d^2 fields (it is inexact on sparse scenes; its finish is the same line)
    ref, ref_ext, df, de = O.reference_sdf(m, res, False, want_dsq=True)
    own = (df - de).astype(np.int64)
    assert np.array_equal(_bits(ref), _bits(R.finish(own, res))), (name, res)
    assert ref_ext == R.extrema(own, res), (name, res, ref_ext)
    assert np.array_equal(np.signbit(ref), m != 0) and np.array_equal(np.signbit(ex), m != 0)      # -0.0 for filled, never +0.0
    c = R.counts(ex)
    print("%s res=%r: %s extrema=%r" % (name, res, c, ex_ext))
    n_filled = int(m.sum())
    if cls == "c":
        assert c["subnormal"] == m.size
    if cls == "d" and np.abs(dsq).max() >= 16:
        assert c["subnormal"] > 0 and c["normal"] > 0
    if cls == "e":
        assert c["negative_zero"] == n_filled and c["positive_zero"] == m.size - n_filled
    if cls == "f":
        assert c["inf"] > 0 and c["normal"] > 0 and all(np.isfinite(ex_ext))
    if cls == "g":
        assert c["inf"] == m.size                            # (1e308 itself is beyond FLT_MAX; the DOUBLE product overflows from D = 4 on)
        assert all(np.isinf(ex_ext)) == bool(min(dsq.max(), -dsq.min()) >= 4)
    if cls in "ab":
        assert c["normal"] == m.size


@pytest.mark.parametrize("name", list(MASKS))
def test_every_class_is_reachable_on_every_scene(name):
    """class_resolutions (what the GPU test iterates over) asserts each class's property itself; here it runs on the CPU scenes,
    and the dense-tier scene is shown to need the second straddle / overflow resolution."""
    _, _, dsq = O.exact_sdf(MASKS[name], 1.0)
    got = R.class_resolutions(dsq)
    assert sorted({c for c, _ in got}) == list("abcdefg")
    if name == "ball levels":
        levels = set(np.unique(np.abs(dsq)).tolist())
        assert levels == {1, 2, 3, 4, 5, 6, 8}
        assert ("d", R.STRADDLE_DENSE) in got and ("f", 2.0 ** 127) in got
    if name == "dense 0.5":
        assert ("d", R.STRADDLE_NOISE) in got and ("f", 1.5 * 2.0 ** 127) in got
    # the oracle against the restatement at EVERY resolution the GPU cases use on this scene, the per-scene extras of classes (d)
    # and (f) included, with and without the virtual border
    m = MASKS[name]
    for vb in (False, True):
        _, _, d = O.exact_sdf(m, 1.0, vb)
        for cls, res in R.class_resolutions(d):
            ex, ex_ext, d2 = O.exact_sdf(m, res, vb)
            assert np.array_equal(d, d2)
            assert np.array_equal(_bits(ex), _bits(R.finish(d, res))) and ex_ext == R.extrema(d, res), (name, vb, cls, res)
            if not vb:
                ref, ref_ext, df, de = O.reference_sdf(m, res, False, want_dsq=True)
                own = (df - de).astype(np.int64)
                assert np.array_equal(_bits(ref), _bits(R.finish(own, res))) and ref_ext == R.extrema(own, res), (name, cls, res)


def test_wide_ball_scene_realises_every_level():
    _, _, dsq = O.exact_sdf(R.ball3_levels((13, 13, 64)), 1.0)
    assert set(np.unique(np.abs(dsq)).tolist()) == {1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14}


def test_a_narrowed_resolution_or_a_subtracted_sign_would_show():
    """The classes can tell the mutants apart: a float copy of a class (a) resolution changes bits of the restatement on these
    scenes, and a sign formed as 0.0f - f gives +0.0 where the reference has -0.0."""
    m = MASKS["sparse 0.03"]
    _, _, dsq = O.exact_sdf(m, 1.0)
    for res in R.CLASS_A:
        assert not np.array_equal(_bits(R.finish(dsq, res)), _bits(R.finish(dsq, float(np.float32(res)))))
    f = np.abs(R.finish(dsq, R.UNDERFLOW))
    subtracted = np.where(m != 0, np.float32(0.0) - f, f)
    assert not np.array_equal(_bits(subtracted), _bits(R.finish(dsq, R.UNDERFLOW)))
