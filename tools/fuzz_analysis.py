#!/usr/bin/env python3
"""Differential fuzzing of the analysis and per-point kernels on a GPU box: random shapes drawn around cc_plan's tiles, random
scenes (tests/analysis_scenes.py's families beside noise, spheres, boxes and floors) and one or more operations per iteration, every
output compared bit for bit with its restatement (the checkers of tests/, imported from there):

  components        sdfgpu_components, _bits_device, _cells (8- and 16-byte records)   restated_labels
  topology          sdfgpu_component_topology, _device, _cells                          restated_counts
  extrema           sdfgpu_local_extrema, _device                                       restated_extrema
  segments          sdfgpu_convex_segments_cells                                        restated_segments
  projection        sdfgpu_project_points, _device, DeviceSignedDistanceField           the host walk (ProjectCounted4d)
  query_gradients   sdfgpu_query_gradients, _device, DeviceSignedDistanceField          the host core (QueryGradient4d)
  query_points      sdfgpu_query_points in any frame of random_frame                    the exact judge of tests/frame_judge.py;
                    (identity and translations: bit-equal, distance included)           analysis_scenes.query_points
  gradient          sdfgpu_gradient_device, fp32 and fp64, aligned or not               analysis_scenes.grid_gradient

The operations that use atomics (components, topology, segments) run twice on the same input; both results must match.

  python tools/fuzz_analysis.py [seconds] [seed]        FUZZ_VERBOSE=1 prints every iteration before it runs (and keeps its scene)

A failing scene is saved as fuzz_analysis_fail_mask.npy in $FUZZ_OUT_DIR (default fuzz_out/, kept out of git).
"""
import math
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import analysis_scenes as A  # noqa: E402
import frame_judge  # noqa: E402
import resample_restated  # noqa: E402
from sdf_tools_amd import capi, synth  # noqa: E402
from test_components_cpu import restated_labels  # noqa: E402
from test_gpu_components import _all_entry_points as components_all  # noqa: E402
from test_gpu_convex_segments import _check_extrema, _check_segments  # noqa: E402
from test_gpu_projection import _check as projection_check, _field, _points, _same  # noqa: E402
from test_gpu_query_gradients import KINDS, _check as gradients_check, _windows  # noqa: E402
from test_gpu_topology import _all_entry_points as topology_all  # noqa: E402
from test_projection_cpu import inverse, rigid  # noqa: E402

OPS = ["components", "topology", "extrema", "segments", "projection", "query_gradients", "query_points", "gradient"]
BERNOULLI_P = [0.001, 0.02, 0.1, 0.3, 0.3116, 0.5, 0.7, 0.9, 0.99]
# The frames' own generator, seeded [seed, tag] in main(): the general-quaternion arm and the frames of op_query_points are drawn
# from it, so that the scenes, points and parameters that the main generator gives a seed stay what they were before the arm existed.
FRAME_TAG = 0xF4A3
frame_rng = None


def draw_shape(rng, op):
    """Around cc_plan's tiles (tz 32 / 64, ty 16, tx 16384 / (tz ty); singleton axes anywhere; thin grids), or ordinary sizes."""
    if rng.random() < 0.6:
        s = [int(rng.choice([1, 31, 32, 33, 63, 64, 65, 97])), int(rng.choice([1, 15, 16, 17])),
             int(rng.choice([1, 2, 15, 16, 17, 31, 32, 33]))]
        s = [s[2], s[1], s[0]]                                                  # (nx, ny, nz)
        if rng.random() < 0.4:
            s = [s[i] for i in rng.permutation(3)]                              # every placement of the singleton axes
    else:
        s = [int(rng.choice([1, 2, 3, 5, 8, 13, 21, 40, 64, 96, 128])) for _ in range(3)]
    cap = 1 << 18 if op in ("topology", "extrema", "segments") else 1 << 20
    while np.prod(s) > cap:
        s[int(np.argmax(s))] //= 2
    return tuple(max(1, v) for v in s)


def draw_scene(rng, shape):
    kinds = ["bernoulli", "spheres", "boxes", "floor", "serpentine", "comb", "stripes", "checkerboard", "shells", "tori", "full",
             "empty"]
    kind = str(rng.choice(kinds))
    seed = int(rng.integers(1 << 30))
    if kind == "bernoulli":
        p = float(rng.choice(BERNOULLI_P))
        return synth.bernoulli_mask(shape, p, seed), "bernoulli %g" % p
    if kind == "spheres":
        return synth.spheres_mask(shape, int(rng.integers(1, 6)), (1, 9), seed), kind
    if kind == "boxes":
        m = np.zeros(shape, np.uint8)
        for _ in range(int(rng.integers(1, 5))):
            lo = [int(rng.integers(0, s)) for s in shape]
            hi = [min(s, l + int(rng.integers(1, max(2, s // 2 + 1)))) for l, s in zip(lo, shape)]
            m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
            if rng.random() < 0.5 and all(h - l > 2 for l, h in zip(lo, hi)):
                m[lo[0] + 1:hi[0] - 1, lo[1] + 1:hi[1] - 1, lo[2] + 1:hi[2] - 1] = 0      # hollow
        return m, kind
    if kind == "floor":
        m = np.zeros(shape, np.uint8)
        m[:, :, :int(rng.integers(1, 4))] = 1
        for _ in range(int(rng.integers(0, 4))):
            x0, x1 = sorted(int(v) for v in rng.integers(0, shape[0] + 1, 2))
            y0 = int(rng.integers(0, shape[1]))
            m[x0:x1 + 1, y0:y0 + int(rng.integers(1, 6)), :int(rng.integers(1, shape[2] + 1))] = 1        # walls and steps
        return m, kind
    if kind in ("comb", "stripes"):
        axis = int(rng.integers(0, 3))
        return getattr(A, kind)(shape, axis), "%s %d" % (kind, axis)
    if kind == "shells":
        return A.nested_shells(shape, int(rng.integers(1, 3))), kind
    if kind == "tori":
        return A.tori_chain(shape, int(rng.integers(0, 4))), kind
    if kind in ("full", "empty"):
        return np.full(shape, int(kind == "full"), np.uint8), kind
    return getattr(A, kind)(shape), kind


def random_quaternion(rng):
    if rng.random() < 0.4:
        return (1.0, 0.0, 0.0, 0.0)
    if rng.random() < 0.3:
        return tuple(float(v) for v in [(1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), (math.sqrt(0.5), 0.0, 0.0, math.sqrt(0.5))][int(rng.integers(0, 3))])
    q = rng.normal(size=4)
    return tuple(float(v) for v in q / np.linalg.norm(q))


def random_frame(rng, extra=None):
    """A translation, an exact signed permutation or a turn about z from `rng`; with `extra` (a generator), three times in ten a
    general quaternion and a translation from `extra` instead: all nine rotation entries nonzero.  What `rng` gives is the same
    with and without `extra`."""
    o = _frame_without_z_coupling(rng)
    if extra is not None and extra.random() < 0.3:
        q = extra.normal(size=4)
        return resample_restated.quaternion_origin(tuple(float(v) for v in q), tuple(float(v) for v in extra.uniform(-2.0, 2.0, 3)))
    return o


def _frame_without_z_coupling(rng):
    t = tuple(float(v) for v in rng.uniform(-2.0, 2.0, 3))
    r = rng.random()
    if r < 0.3:
        o = np.eye(4)
        o[:3, 3] = t
        return o
    if r < 0.6:                                               # exact quarter and half turns (entries 0, 1, -1)
        o = np.eye(4)
        perm = rng.permutation(3)
        signs = rng.choice([-1.0, 1.0], 3)
        R = np.zeros((3, 3))
        R[np.arange(3), perm] = signs
        if np.linalg.det(R) < 0:
            R[0] *= -1.0
        o[:3, :3] = R
        o[:3, 3] = t
        return o
    return rigid(float(rng.uniform(-math.pi, math.pi)), t)


def with_unknown(rng, mask):
    """occupancy for the cell-record forms: 0 / 1 with unknown (0.5), NaN and near-threshold values sprinkled in"""
    occ = mask.astype(np.float32)
    if rng.random() < 0.5:
        pick = rng.random(mask.shape) < float(rng.choice([0.01, 0.1]))
        occ[pick] = rng.choice(np.array([0.5, np.nan, 0.50001, 0.49999], np.float32), int(pick.sum()))
    return occ


def points(rng, sdf, res, origin, mask):
    pts = _points(sdf, res, origin, mask, int(rng.choice([64, 300])), int(rng.integers(1 << 30)))
    k = np.asarray([[int(rng.integers(0, s + 1)) for s in sdf.shape] for _ in range(32)], np.float64) * res     # multiples of res
    o = np.asarray(origin, np.float64)
    return np.concatenate([pts, np.stack([o[i, 0] * k[:, 0] + o[i, 1] * k[:, 1] + o[i, 2] * k[:, 2] + o[i, 3] for i in range(3)], 1)])


# ---- one operation ----------------------------------------------------------------------------------------------------------------
def op_components(ctx, rng, mask):
    occ = with_unknown(rng, mask)
    components_all(ctx, occ)
    a = ctx.components(occ > 0.5)
    b = ctx.components(occ > 0.5)
    assert a[1] == b[1] and np.array_equal(a[0], b[0]), "components: two runs differ"


def op_topology(ctx, rng, mask):
    labels, k = restated_labels(mask)
    r = rng.random()
    if r < 0.6:
        sel, cls = (mask != 0, capi.TOPOLOGY_FILLED) if rng.random() < 0.5 else (None, 7)
        max_label = k + int(rng.choice([0, 0, 1, 17]))
        topology_all(ctx, labels, sel, max_label, mask.astype(np.float32), cls)
    else:                                                   # arbitrary labels: colliding table labels, many labels, label 0 in use
        sel = None
        if r < 0.8:
            col, _ = A.colliding_labels(int(rng.integers(17, 64)), start=int(rng.integers(1, 5000)))
            labels = col[rng.integers(0, len(col), mask.shape)]
        else:
            labels = rng.integers(0, int(rng.choice([3, 1500, 9000])), mask.shape).astype(np.uint32)
        max_label = int(labels.max()) + int(rng.choice([0, 0, 5]))
        topology_all(ctx, labels, None, max_label, np.zeros(mask.shape, np.float32), 7)
    a = ctx.component_topology(labels, sel, max_label)
    b = ctx.component_topology(labels, sel, max_label)
    assert np.array_equal(a, b), "topology: two runs differ"


def op_extrema(ctx, rng, mask, res):
    if rng.random() < 0.5:
        sdf, _ = ctx.build(mask, res)
    else:                                                   # quantised noise: many exact ties
        sdf = (rng.integers(-4, 5, mask.shape) * float(rng.choice([res, 0.5 * res]))).astype(np.float32)
    _check_extrema(ctx, sdf, res, random_quaternion(rng))


def op_segments(ctx, rng, mask, res):
    occ = with_unknown(rng, mask)
    obj = np.where(mask != 0, rng.integers(0, int(rng.choice([1, 2, 4])), mask.shape), 0).astype(np.uint32)
    thr = float(rng.choice([0.0, 0.5 * res, res, 1.75 * res, 1.5, 40.0]))
    border, q = bool(rng.integers(0, 2)), random_quaternion(rng)
    a, ka = _check_segments(ctx, occ, obj, res, thr, border, q)
    b, kb = _check_segments(ctx, occ, obj, res, thr, border, q)
    assert ka == kb and np.array_equal(a, b)


def _device_field(ctx, rng, mask, res):
    sdf, _ = ctx.build(mask, res)
    origin = random_frame(rng, frame_rng)
    d, ptr, host = _field(ctx, sdf, res, origin)
    return sdf, origin, d, ptr, host


def op_projection(ctx, rng, mask, res):
    sdf, origin, d, ptr, host = _device_field(ctx, rng, mask, res)
    pts = points(rng, sdf, res, origin, mask)
    valid_only = bool(rng.integers(0, 2))
    md = float(rng.choice([0.0, 0.5 * res, 1.5 * res, 4.0 * res, 1e3]))
    mult = float(rng.choice([0.125, 0.5, 1.0, 0.01]))
    max_steps = int(rng.choice([0, 0, 1, 7, 64]))
    want = projection_check(d, ptr, host, res, origin, pts, md, mult, valid_only, max_steps, ctx=ctx)
    n = len(pts)                                            # the device form
    dp = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    out = torch.full((n, 3), -1.0, dtype=torch.float64, device="cuda")
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    steps = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    ctx.project_points_device(ptr, sdf.shape, res, dp.data_ptr(), n, out.data_ptr(), inverse(origin), origin, md, mult, max_steps,
                              valid_only, st.data_ptr(), steps.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), want[0]) and _same(st.cpu().numpy(), want[1]) and _same(steps.cpu().numpy(), want[2]), \
        "sdfgpu_project_points_device"


def op_query_gradients(ctx, rng, mask, res):
    sdf, origin, d, ptr, host = _device_field(ctx, rng, mask, res)
    pts = points(rng, sdf, res, origin, mask)
    kind = int(rng.choice(KINDS))
    windows = _windows(res, sdf.shape) if kind == capi.QUERY_SMOOTH_GRADIENT else [0.0]
    gradients_check(d, ptr, host, res, origin, pts, kind, float(rng.choice(windows)), ctx=ctx)


def _near(a, b):
    """the query_points distance: bit-equal (two NaNs are equal) -- k_query_points rounds every product and sum on its own, and the
    grid coordinates of op_query_points are exact (see there)"""
    return _same(a, b)


def op_query_points(ctx, rng, mask, res):
    sdf, _ = ctx.build(mask, res)
    rng.uniform(-2.0, 2.0, 3)                               # (the translation this operation drew before its frames had their own generator)
    origin = random_frame(frame_rng, frame_rng)
    pts = points(rng, sdf, res, origin, mask)
    edge = bool(rng.integers(0, 2))
    oob = float(rng.choice([math.inf, 55.0, -1.0]))
    d_sdf = torch.from_numpy(sdf).cuda()
    w2g, rot = frame_judge.transforms(origin)
    dist, grad, flags = ctx.query_points(d_sdf.data_ptr(), sdf.shape, res, pts, world_to_grid=w2g, rotation=rot, oob_value=oob,
                                         enable_edge_gradients=edge)
    # any frame: the exact cell unless rounding can move it, the exact estimate and the exactly rotated gradient within their bounds
    frame_judge.judge(sdf, res, w2g, rot, pts, edge).check(dist, grad, flags, oob)
    if not np.array_equal(origin[:3, :3], np.eye(3)):
        return
    # grid frame: w2g = (I, -t), so the kernel's 1 x + 0 y + 0 z - t is x - t exactly, fused or not (finite points)
    g = pts - origin[:3, 3]
    wd, wg, wf = A.query_points(sdf, res, g, oob, edge)
    assert np.array_equal(flags, wf), "query_points flags"
    ok = np.isfinite(pts).all(axis=1)                       # (0 * inf makes a non-finite point's grid coordinates NaN)
    assert _same(grad[ok], wg[ok]), "query_points gradient"
    assert _near(dist[ok], wd[ok]), "query_points distance"


def op_gradient(ctx, rng, mask, res):
    if rng.random() < 0.5:
        sdf, _ = ctx.build(mask, res)
    else:
        sdf = (rng.integers(-40, 41, mask.shape) * 0.125).astype(np.float32)
        sdf[rng.random(mask.shape) < 0.02] = np.inf
    edge = bool(rng.integers(0, 2))
    f64 = bool(rng.integers(0, 2))
    shift_in, shift_out = int(rng.choice([0, 0, 1, 3])), int(rng.choice([0, 0, 1, 2]))
    n = sdf.size
    fin = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    fin[shift_in:shift_in + n] = torch.from_numpy(sdf.reshape(-1)).cuda()
    dt, w = (torch.float64, 8) if f64 else (torch.float32, 4)
    out = torch.full((3 * n + 4,), -7.0, dtype=dt, device="cuda")
    ctx.gradient_device(fin.data_ptr() + 4 * shift_in, sdf.shape, out.data_ptr() + w * shift_out, res, edge, f64)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:shift_out] == -7.0).all() and (o[shift_out + 3 * n:] == -7.0).all(), "gradient: written outside its output"
    want = A.grid_gradient(sdf, res, edge)
    if not f64:
        want = want.astype(np.float32)
    assert _same_nan(o[shift_out:shift_out + 3 * n].reshape(want.shape), want), "gradient values"


def _same_nan(a, b):
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    verbose = bool(os.environ.get("FUZZ_VERBOSE"))
    out_dir = os.environ.get("FUZZ_OUT_DIR", "fuzz_out")
    rng = np.random.default_rng(seed)
    globals()["frame_rng"] = np.random.default_rng([seed, FRAME_TAG])
    ctx = capi.SdfGpu(0)
    counts = {op: 0 for op in OPS}
    order = []
    t0 = time.time()
    it = 0
    while time.time() - t0 < budget:
        if not order:
            order = [OPS[i] for i in rng.permutation(len(OPS))]            # every operation once per round
        ops = [order.pop()]
        if rng.random() < 0.2 and order:
            ops.append(order.pop())                                          # two operations on one scene
        shape = draw_shape(rng, ops[0])
        mask, kind = draw_scene(rng, shape)
        res = float(rng.choice([1.0, 0.05, 0.037]))
        if verbose:
            print("iteration", it, ops, shape, kind, "res", res, "filled", int(mask.sum()), flush=True)
            os.makedirs(out_dir, exist_ok=True)
            np.save(os.path.join(out_dir, "fuzz_analysis_last_mask.npy"), mask)
        for op in ops:
            try:
                if op in ("components", "topology"):
                    globals()["op_" + op](ctx, rng, mask)
                else:
                    globals()["op_" + op](ctx, rng, mask, res)
            except (AssertionError, capi.SdfGpuError):         # (a refusal of a valid input is a finding too)
                os.makedirs(out_dir, exist_ok=True)
                np.save(os.path.join(out_dir, "fuzz_analysis_fail_mask.npy"), mask)
                traceback.print_exc()
                print("MISMATCH op", op, "iteration", it, "shape", shape, "scene", kind, "res", res, "seed", seed)
                sys.exit(1)
            counts[op] += 1
        it += 1
    ctx.close()
    print("fuzz OK: %d iterations in %.0f s (seed %d); operations %s" % (it, time.time() - t0, seed, counts))


if __name__ == "__main__":
    main()
