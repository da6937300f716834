"""Resolutions and scenes shared by test_resolution_domain_cpu.py and test_gpu_resolution_domain.py: the finishing step
float(sqrt((double)D) * resolution) (sdf_generation.hpp:254-265) at the ends of the float range, restated in numpy, and the
helpers that PROVE from the integer squared distances alone that a (scene, resolution) pair exercises the edge it is there for.

Classes (the numbers follow from the float format: FLT_MIN = 2^-126, smallest subnormal 2^-149, FLT_MAX = 2^128 (1 - 2^-24)):
  (a) doubles that are not floats          1/3, 0.1 + 2^-40, 0.037       a narrowed copy of the resolution changes low bits
  (b) float-exact                          2^-3, 0.375
  (c) every non-zero output subnormal      2^-140                         sqrt(D) < 2^14: below FLT_MIN; one rounding, not two
  (d) straddling FLT_MIN in one field      2^-128 (1 + 2^-30)             sqrt(D) >= 4 (D >= 16) is normal, below it subnormal
  (e) everything underflows to signed 0    2^-160                         sqrt(D) < 2^10: below half the smallest subnormal
  (f) partial overflow                     2^125 / 2^126 per scene        sqrt(D) 2^126 >= 2^128 iff D >= 16 (2^125: D >= 64)
  (g) total overflow                       1e308                          D >= 4 overflows the DOUBLE product as well
A dense-tier scene has D <= 8 (KD) or <= 14 (KD3) everywhere, so neither (d)'s nor (f)'s resolutions split it: for such scenes
(max D < 16) the lists ALSO hold 2^-127 (1 + 2^-30) and 2^127, which put the split at D >= 4, and for Bernoulli 0.5 noise
(D <= 3) 0.75 * 2^-126 (1 + 2^-30) and 1.5 * 2^127, which put it at D >= 2.  Nothing is left out for it."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
STRADDLE = 2.0 ** -128 * (1.0 + 2.0 ** -30)
STRADDLE_DENSE = 2.0 ** -127 * (1.0 + 2.0 ** -30)
STRADDLE_NOISE = 0.75 * 2.0 ** -126 * (1.0 + 2.0 ** -30)
CLASS_A = (1.0 / 3.0, 0.1 + 2.0 ** -40, 0.037)
CLASS_B = (2.0 ** -3, 0.375)
SUBNORMAL = 2.0 ** -140
UNDERFLOW = 2.0 ** -160
TOTAL_OVERFLOW = 1e308


def finish(dsq, res):
    """The plain restatement: signed int64 d^2 (+ free, - filled; |d^2| = INT64_MAX: no voxel of the other class) -> float32 field."""
    dsq = np.asarray(dsq, np.int64)
    mag = np.abs(dsq).astype(np.float64)
    mag[np.abs(dsq) == np.iinfo(np.int64).max] = np.inf
    with np.errstate(over="ignore", under="ignore"):
        f = (np.sqrt(mag) * res).astype(np.float32)
    return np.where(dsq < 0, np.float32(-1.0), np.float32(1.0)) * f


def extrema(dsq, res):
    """(max, min) of the un-narrowed doubles (sdf_generation.hpp:246-269): max over the free voxels, min over the filled ones."""
    dsq = np.asarray(dsq, np.int64)
    big = np.iinfo(np.int64).max
    free, filled = dsq[dsq > 0], -dsq[dsq < 0]
    with np.errstate(over="ignore"):
        mx = -np.inf if free.size == 0 else np.inf if free.max() == big else float(np.sqrt(np.float64(free.max())) * res)
        mn = np.inf if filled.size == 0 else -np.inf if filled.max() == big else float(0.0 - np.sqrt(np.float64(filled.max())) * res)
    return mx, mn


def counts(f):
    """{subnormal, negative_zero, positive_zero, inf, normal} voxel counts of a float32 field."""
    f = np.asarray(f, np.float32)
    a = np.abs(f)
    return {"subnormal": int(((a > 0) & (a < FLT_MIN)).sum()), "negative_zero": int(((f == 0) & np.signbit(f)).sum()),
            "positive_zero": int(((f == 0) & ~np.signbit(f)).sum()), "inf": int(np.isinf(f).sum()),
            "normal": int((np.isfinite(f) & (a >= FLT_MIN)).sum())}


def partial_overflow(dsq):
    """The class (f) resolution of a scene: the first of 2^125, 2^126 (and 2^127, 1.5 * 2^127 for scenes whose D stays below 16) at which some
    voxels stay finite and others overflow.  Chosen from the integer distances; raises when the scene has no such resolution."""
    for r in (2.0 ** 125, 2.0 ** 126, 2.0 ** 127, 1.5 * 2.0 ** 127):
        c = counts(finish(dsq, r))
        if c["inf"] > 0 and c["normal"] > 0:
            return r
    raise AssertionError("no resolution splits this scene at FLT_MAX")


def straddle(dsq):
    """The class (d) resolutions of a scene: 2^-128 (1 + 2^-30) always, and where that leaves every voxel subnormal (max D < 16)
    the next one that puts subnormal and normal voxels into one field."""
    out = [STRADDLE]
    for r in (STRADDLE, STRADDLE_DENSE, STRADDLE_NOISE):
        c = counts(finish(dsq, r))
        if c["subnormal"] > 0 and c["normal"] > 0:
            return out if r == STRADDLE else out + [r]
    raise AssertionError("no resolution splits this scene at FLT_MIN")


def class_resolutions(dsq):
    """[(class, resolution)] for one scene: every class (a)-(g), each with the property that makes it meaningful asserted here
    from the restatement alone."""
    D = np.abs(np.asarray(dsq, np.int64))
    assert D.max() < (1 << 20) and D.min() >= 1           # both classes present, sqrt(D) < 2^10
    out = [("a", r) for r in CLASS_A] + [("b", r) for r in CLASS_B]
    c = counts(finish(dsq, SUBNORMAL))
    assert c["subnormal"] == D.size, c
    out.append(("c", SUBNORMAL))
    out += [("d", r) for r in straddle(dsq)]
    c = counts(finish(dsq, UNDERFLOW))
    assert c["negative_zero"] == int((np.asarray(dsq) < 0).sum()) > 0 and c["positive_zero"] == int((np.asarray(dsq) > 0).sum()), c
    out.append(("e", UNDERFLOW))
    f = partial_overflow(dsq)
    mx, mn = extrema(dsq, f)
    assert np.isfinite(mx) and np.isfinite(mn)              # the float field overflows, the double extrema do not
    out.append(("f", f))
    c = counts(finish(dsq, TOTAL_OVERFLOW))
    assert c["inf"] > 0, c
    out.append(("g", TOTAL_OVERFLOW))
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def ball_levels(shape):
    """Both classes within d^2 <= 8 of each other, every level of KD's ball (1, 2, 3, 4, 5, 6, 8) realised by free voxels: filled
    lines along z every 4th x and y (d^2 up to (2, 2, 0) = 8) in the low half of z, a (4, 2, 2) lattice (d^2 up to (2, 1, 1) = 6)
    in the high half."""
    m = np.zeros(shape, np.uint8)
    h = shape[2] // 2
    m[::4, ::4, :h] = 1
    m[::4, ::2, h::2] = 1
    return m


def ball3_levels(shape):
    """Every level of KD3's ball (1 .. 6, 8 .. 14) and nothing beyond (shapes (12 i + 1, 4 j + 1, 64)): a (6, 4, 2) lattice (d^2 up to (3, 2, 1) = 14) in the low
    half of z, a (4, 4, 4) lattice ((2, 2, 2) = 12) in the high half."""
    m = np.zeros(shape, np.uint8)
    h = shape[2] // 2
    m[::6, ::4, :h:2] = 1
    m[::4, ::4, h::4] = 1
    m[::4, ::4, -1] = 1                                     # (no voxel farther than the lattice's own cells from the last z plane)
    return m


def corner_voxel(shape):
    m = np.zeros(shape, np.uint8)
    m[0, 0, 0] = 1
    return m
