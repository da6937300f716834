"""GPU: every device entry point of include/sdfgpu.h on a NON-BLOCKING side stream whose inputs arrive late (stream_harness.py).

On the null stream a kernel launched on the wrong stream, a memset or status read-back issued there, a synchronous copy where an
asynchronous one plus a stream synchronisation was meant, or handle scratch shared by two calls in flight all come out right.
PyTorch's side streams are hipStreamNonBlocking: the null stream does not wait for them, so here they do not.

  family 1  each call honours its stream: decoys in the inputs, the real inputs copied over them behind a delay on the side
            stream, the consumer a clone on that stream; red zones off (calls stay asynchronous) and on (every call ends with a
            check on its stream).
  family 2  what the header promises about a handle: the host forms and debug hooks straight behind a delayed build_device with no
            host synchronisation by the caller; a build on stream A, the tiered stage pair and a batch on stream B, a build on A
            again -- exact, and the later work does not start before the earlier (an event recorded behind it is still pending
            while the delay holds).
  family 3  handle-owned analysis scratch: two calls of different shapes back to back on two side streams, one handle and two.
            components, topology and surfaces return fully synchronised and the per-point device calls use no handle scratch;
            sdfgpu_local_extrema_device returns with three kernels pending that use cx_scratch, so the library now orders a
            following extrema computation on another stream behind them with an event of the handle (as builds are ordered).

References are the ones the entry points' own tests use: oracle.exact_sdf, oracle.classify_cells, restated_labels,
restated_counts, restated_surfaces, restated_extrema, analysis_scenes.grid_gradient / query_points, the host walk and the host
core of the C++ mirror, _numpy_voxelize.  Bit for bit (NaN equals NaN where a restatement is numpy's).

The delay: torch.cuda._sleep, calibrated per module with HIP events; every case first runs its call twice undelayed (the first
allocates scratch and uploads first-use tables), times the second on the host and sleeps max(20 ms, 10 x that), 400 ms at most.
Measured on an MI355X: torch.cuda._sleep runs 2 395 000 cycles per ms; the slowest warm call (enqueue and execution, host
side) is the out-of-collision projection of 6076 points, 5.2 ms alone and 7.9 ms in the pair of family 3, so its delay is 52 to
79 ms; every other call is below 0.4 ms warm and sleeps the floor of 20 ms.  Every case prints both figures.  The witnesses,
not the number, are what make a case valid.
The two side streams are chosen once per module by a probe (stream_harness.pick_streams): the runtime deals its 4 hardware queues
out to streams as they are created, and side streams taken blindly shared a queue with the null stream or with each other in
about half of the cases of the first run on an MI355X, which the witnesses reported.

Entry points with a stream that are NOT here: sdfgpu_sweep_zy_device (it is sdfgpu_sweep_zy_tiered_device with d_far = NULL, which
is here), sdfgpu_sweep_x_device, sdfgpu_dense_ball_device, sdfgpu_fold_extrema_device and sdfgpu_slab_dense_phase (the slab
phases of the multi-GPU path, whose stage calls of one build are documented to share one stream), sdfgpu_gradient_batch_device
(one launch of the kernel sdfgpu_gradient_device launches, on two streams in test_gpu_batch_edges.py), sdfgpu_redzone_check (it
ends every red-zone case here).
"""
import functools
import math

import numpy as np
import pytest
import torch

import analysis_scenes as A
import stream_harness as H
from component_surfaces_restated import restated_surfaces
from oracle import oracle as O
from sdf_tools_amd import capi, synth
from sdf_tools_amd._bindings import load_pysdf_tools
from test_components_cpu import restated_labels
from test_convex_segments_cpu import restated_extrema
from test_gpu_parity import _exact_stage_fields
from test_gpu_projection import _points
from test_gpu_streaming import _numpy_voxelize
from test_projection_cpu import inverse, rigid
from test_topology_cpu import restated_counts

pytestmark = pytest.mark.gpu
m = load_pysdf_tools()

S1, S2, SB = (33, 17, 96), (40, 33, 35), (25, 20, 15)
RES = 0.05
ORIGIN = rigid(0.3, (0.1, -0.2, 0.05))


# ---- scenes and references, computed once --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mask(shape, seed):
    """Bernoulli(0.3); seed 11, the decoy of the field and label cases, is sparser, so that its extrema differ as well"""
    return synth.bernoulli_mask(shape, 0.12 if seed == 11 else 0.3, seed)


@functools.lru_cache(maxsize=None)
def exact(shape, seed, vb=False, res=RES):
    sdf, ext, _ = O.exact_sdf(mask(shape, seed), res, vb)
    return sdf, tuple(float(v) for v in ext)


@functools.lru_cache(maxsize=None)
def labels(shape, seed):
    return restated_labels(mask(shape, seed))


@functools.lru_cache(maxsize=None)
def random_labels(shape, seed, max_label):
    """arbitrary labels in blobs (every value up to max_label in use, label 0 too)"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, max_label + 1, [(s + 2) // 3 for s in shape], dtype=np.uint32)
    lab = np.repeat(np.repeat(np.repeat(coarse, 3, 0), 3, 1), 3, 2)[:shape[0], :shape[1], :shape[2]].copy()
    flip = rng.random(shape) < 0.1
    lab[flip] = rng.integers(0, max_label + 1, int(flip.sum()), dtype=np.uint32)
    return lab


@functools.lru_cache(maxsize=None)
def host_field(shape, seed):
    f = m.SignedDistanceField(m.Isometry3d(ORIGIN), "world", RES, *shape, math.inf)
    f.SetRawDataNumpy(exact(shape, seed)[0])
    return f


@functools.lru_cache(maxsize=None)
def world_points(shape, seed, finite=False):
    """the point set of test_gpu_projection.py (faces, corners, deep in obstacles, NaN and inf); finite = a decoy: uniform only"""
    pts = _points(exact(shape, seed)[0], RES, ORIGIN, mask(shape, seed), 3000, seed)
    if finite:
        rng = np.random.default_rng(seed + 7)
        g = rng.uniform(-0.1, 1.1, pts.shape) * np.array(shape) * RES
        pts = np.stack([ORIGIN[i, 0] * g[:, 0] + ORIGIN[i, 1] * g[:, 1] + ORIGIN[i, 2] * g[:, 2] + ORIGIN[i, 3] for i in range(3)], 1)
    return np.ascontiguousarray(pts)


@functools.lru_cache(maxsize=None)
def grid_points(shape, seed, n=6000):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.05, 1.05, (n, 3)) * np.array(shape) * RES


@functools.lru_cache(maxsize=None)
def cloud(shape, seed, n=5000):
    """fp32 points for the voxeliser: most inside the grid, some outside"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-0.1, 1.1, (n, 3)) * np.array(shape) * RES).astype(np.float32)


def cells8(shape, seed):
    rng = np.random.default_rng(seed)
    c = np.zeros(shape + (2,), np.float32)
    c[..., 0] = rng.choice(np.array([0.0, 0.5, 1.0, 0.50000006, np.nan], np.float32), size=shape, p=[0.5, 0.1, 0.3, 0.05, 0.05])
    c[..., 1] = rng.random(shape).astype(np.float32)               # (the component word: any bits)
    return c


def cells16(c8, seed):
    n = c8[..., 0].size
    raw = np.random.default_rng(seed).integers(0, 256, (n, 16), dtype=np.uint8)
    raw[:, 4:8] = np.ascontiguousarray(c8[..., 0]).reshape(-1).view(np.uint8).reshape(n, 4)   # occupancy at offset 4
    return raw


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def delay():
    return H.Delay()


@pytest.fixture(scope="module")
def streams(delay):
    """two side streams that share a hardware queue neither with the null stream nor with each other (probed, not assumed)"""
    return H.pick_streams(delay)


@pytest.fixture(params=[0, 1], ids=["asynchronous", "redzones"])
def ctx(gpu, request):
    gpu.set_option("redzone", request.param)
    gpu.redzones = bool(request.param)
    yield gpu
    gpu.set_option("redzone", 0)


@pytest.fixture
def fresh():
    c = capi.SdfGpu(0)
    yield c
    c.close()


# ---- jobs: one library call with its decoys, outputs and reference ---------------------------------------------------------------
class Job:
    """inputs: {name: (decoy, real)}; outputs: {name: bytes}; call(h, p, stream) -> host result, p[name] = device address;
    check(host, got, which) compares against the reference of which = 1 (real) and requires 0 (decoy) to differ;
    asynchronous: the entry point returns before its work has finished; inout: inputs the call updates in place"""
    asynchronous, inout = True, ()


def _io(job, case):
    p = {}
    for name, (decoy, real) in job.inputs.items():
        p[name] = case.input(name, decoy, real)
    for name, nbytes in job.outputs.items():
        p[name] = case.output(name, nbytes)
    return p


def build_job(kind, shape, vb):
    j = Job()
    n = int(np.prod(shape))
    if kind == "cells":
        c = [cells8(shape, 50), cells8(shape, 51)]
        masks = [O.classify_cells(x, True) for x in c]
        j.inputs = {"in": tuple(c)}
    else:
        masks = [mask(shape, 11), mask(shape, 12)]
        j.inputs = {"in": tuple(capi.pack_bits_host(x) for x in masks) if kind == "bits" else tuple(masks)}
    want = [O.exact_sdf(x, RES, vb) for x in masks]
    j.outputs = {"sdf": n * 4}

    def call(h, p, s):
        if kind == "mask":
            h.build_device(p["in"], shape, p["sdf"], RES, vb, s)
        elif kind == "bits":
            h.build_bits_device(p["in"], shape, p["sdf"], RES, vb, s)
        else:
            h.build_cells_device(p["in"], shape, p["sdf"], 8, 0, True, RES, vb, s)
        return h
    j.call = call

    def check(h, got):
        H.expect("the field", H.view(got["sdf"], np.float32, shape), want[1][0], want[0][0])
        assert h.get_extrema() == tuple(float(v) for v in want[1][1])       # (the decoy's may coincide: the field tells them apart)
    j.check = check
    return j


def classify_job(stride):
    j = Job()
    c = [cells8(S1, 52), cells8(S1, 53)]
    want = [O.classify_cells(x, False) for x in c]
    j.inputs = {"cells": tuple(c) if stride == 8 else tuple(cells16(x, 3) for x in c)}
    j.outputs = {"mask": want[0].size}
    j.call = lambda h, p, s: h.classify_cells_device(p["cells"], want[0].size, p["mask"], stride, 0 if stride == 8 else 4, False, s)
    j.check = lambda host, got: H.expect("the mask", got["mask"], want[1], want[0])
    return j


def pack_job():
    j = Job()
    masks = [mask(S1, 13) * np.uint8(255), mask(S1, 14) * np.uint8(7)]
    j.inputs = {"mask": tuple(masks)}
    j.outputs = {"bits": masks[0].size // 8}
    j.call = lambda h, p, s: h.pack_bits_device(p["mask"], S1[0] * S1[1], S1[2], p["bits"], s)
    j.check = lambda host, got: H.expect("the bits", got["bits"], capi.pack_bits_host(masks[1]), capi.pack_bits_host(masks[0]))
    return j


def voxelize_job(bits, clear_first):
    j = Job()
    shape = S2
    pc = [cloud(shape, 20), cloud(shape, 21)]
    base = [mask(shape, 15), mask(shape, 16)]
    vox = [_numpy_voxelize(x, shape, RES, (0.0, 0.0, 0.0)) for x in pc]
    want = vox if clear_first else [v | b for v, b in zip(vox, base)]
    enc = capi.pack_bits_host if bits else (lambda a: a)
    j.inputs = {"points": tuple(pc)}
    if clear_first:
        j.outputs = {"grid": enc(want[0]).nbytes}
    else:
        j.inputs["grid"] = tuple(enc(b) for b in base)          # the delayed producer writes the mask the points are added to
        j.outputs = {}
        j.inout = ("grid",)
    fn = "voxelize_points_bits_device" if bits else "voxelize_points_device"
    j.call = lambda h, p, s: getattr(h, fn)(p["points"], len(pc[0]), (0.0, 0.0, 0.0), RES, shape, p["grid"], clear_first, s)
    j.check = lambda host, got: H.expect("the grid", got["grid"], enc(want[1]), enc(want[0]))
    return j


def gradient_job(shape, f64):
    j = Job()
    f = [exact(shape, 11)[0], exact(shape, 12)[0]]
    dt = np.float64 if f64 else np.float32
    want = [A.grid_gradient(x, RES, True).astype(dt) for x in f]
    j.inputs = {"sdf": tuple(f)}
    j.outputs = {"grad": want[0].nbytes}
    j.call = lambda h, p, s: h.gradient_device(p["sdf"], shape, p["grad"], RES, True, f64, s)
    j.check = lambda host, got: H.expect("the gradient", H.view(got["grad"], dt, want[0].shape), want[1], want[0], H.same_or_nan)
    return j


def query_points_job(shape, edge):
    j = Job()
    f = [exact(shape, 11)[0], exact(shape, 12)[0]]
    g = [grid_points(shape, 30), grid_points(shape, 31)]
    want = [A.query_points(f[k], RES, g[k], np.inf, edge) for k in range(2)]
    n = len(g[0])
    j.inputs = {"sdf": tuple(f), "points": tuple(g)}
    j.outputs = {"distance": n * 8, "gradient": n * 24, "flags": n}
    j.call = lambda h, p, s: h.query_points_device(p["sdf"], shape, RES, p["points"], n, p["distance"], p["gradient"], p["flags"],
                                                   None, None, math.inf, edge, s)

    def check(host, got):
        H.expect("the distances", H.view(got["distance"], np.float64), want[1][0], want[0][0], H.same_or_nan)
        H.expect("the gradients", H.view(got["gradient"], np.float64, (n, 3)), want[1][1], want[0][1], H.same_or_nan)
        H.expect("the flags", H.view(got["flags"], np.uint8, (n,)), want[1][2], want[0][2])
    j.check = check
    return j


def query_gradients_job(shape, kind):
    j = Job()
    f = [exact(shape, 11)[0], exact(shape, 12)[0]]
    pts = [np.resize(world_points(shape, 11, True), world_points(shape, 12).shape), world_points(shape, 12)]
    window = RES if kind == capi.QUERY_SMOOTH_GRADIENT else 0.0
    want = [host_field(shape, 11 + k).QueryGradientsNumpyHost(pts[k], kind, window) for k in range(2)]
    n = len(pts[1])
    j.inputs = {"sdf": tuple(f), "points": tuple(pts)}
    j.outputs = {"value": n * 8, "gradient": n * 24, "status": n}
    j.call = lambda h, p, s: h.query_gradients_device(p["sdf"], shape, RES, p["points"], n, inverse(ORIGIN), kind, window, math.inf,
                                                      p["value"], p["gradient"], p["status"], s)

    def check(host, got):
        H.expect("the values", H.view(got["value"], np.float64), want[1][0], want[0][0])
        if kind != capi.QUERY_DISTANCE_TO_BOUNDARY:              # (that kind computes no gradient: NaN for every point)
            H.expect("the gradients", H.view(got["gradient"], np.float64, (n, 3)), want[1][1], want[0][1])
        else:
            H.expect("the gradients", H.view(got["gradient"], np.float64, (n, 3)), want[1][1])
        H.expect("the statuses", H.view(got["status"], np.uint8, (n,)), want[1][2], want[0][2])
    j.check = check
    return j


def project_job(shape, valid_only):
    j = Job()
    f = [exact(shape, 11)[0], exact(shape, 12)[0]]
    pts = [np.resize(world_points(shape, 11, True), world_points(shape, 12).shape), world_points(shape, 12)]
    md = 1.5 * RES
    want = [host_field(shape, 11 + k).ProjectOutOfCollisionNumpyHost(pts[k], md, 0.125, 0, valid_only) for k in range(2)]
    n = len(pts[1])
    j.inputs = {"sdf": tuple(f), "points": tuple(pts)}
    j.outputs = {"out": n * 24, "status": n, "steps": n * 4}
    j.call = lambda h, p, s: h.project_points_device(p["sdf"], shape, RES, p["points"], n, p["out"], inverse(ORIGIN), ORIGIN, md, 0.125, 0,
                                                     valid_only, p["status"], p["steps"], s)

    def check(host, got):
        H.expect("the locations", H.view(got["out"], np.float64, (n, 3)), want[1][0], want[0][0])
        H.expect("the statuses", H.view(got["status"], np.uint8, (n,)), want[1][1], want[0][1])
        H.expect("the step counts", H.view(got["steps"], np.int32, (n,)), want[1][2], None if valid_only else want[0][2])
    j.check = check
    return j


def components_job(shape):
    j = Job()
    j.asynchronous = False
    masks = [mask(shape, 11), mask(shape, 12)]
    want = [labels(shape, 11), labels(shape, 12)]
    j.inputs = {"bits": tuple(capi.pack_bits_host(x) for x in masks)}
    j.outputs = {"labels": masks[0].size * 4}
    j.call = lambda h, p, s: h.components_bits_device(p["bits"], shape, p["labels"], s)

    def check(k, got):
        H.expect("the labels", H.view(got["labels"], np.uint32, shape), want[1][0], want[0][0])
        assert k == want[1][1]
    j.check = check
    return j


def topology_job(shape, select):
    j = Job()
    j.asynchronous = False
    lab = [labels(shape, 11)[0], labels(shape, 12)[0]]
    sel = [mask(shape, 11), mask(shape, 12)]                     # the filled components, as ignore_empty_components selects
    max_label = max(int(x.max()) for x in lab)
    want = [restated_counts(lab[k], sel[k] if select else None, max_label) for k in range(2)]
    j.inputs = {"labels": tuple(lab)}
    if select:
        j.inputs["select"] = tuple(capi.pack_bits_host(x) for x in sel)
    j.outputs = {}
    j.call = lambda h, p, s: h.component_topology_device(p["labels"], shape, max_label, p.get("select"), s)
    j.check = lambda counts, got: H.expect("the counters", counts, want[1], want[0])
    return j


def surfaces_job(shape, max_label, variant):
    """variant: counts (no indices), indices (into the caller's buffer), bits (indices, selection and d_surface_bits)"""
    j = Job()
    j.asynchronous = False
    n = int(np.prod(shape))
    lab = [random_labels(shape, 40, max_label), random_labels(shape, 41, max_label)]
    sel = [mask(shape, 17), mask(shape, 18)] if variant == "bits" else [None, None]
    want = [restated_surfaces(lab[k], sel[k], max_label) for k in range(2)]
    j.inputs = {"labels": tuple(lab)}
    j.outputs = {}
    if variant == "bits":
        j.inputs["select"] = tuple(capi.pack_bits_host(x) for x in sel)
        j.outputs["surface_bits"] = ((n + 31) // 32) * 4
    if variant != "counts":
        j.outputs["indices"] = n * 4
    j.call = lambda h, p, s: h.component_surfaces_device(p["labels"], shape, max_label, p.get("select"), p.get("indices"), n,
                                                         p.get("surface_bits"), s, counts_only=variant == "counts")

    def check(host, got):
        counts, total = host
        H.expect("the counts", counts, want[1][0], want[0][0])
        assert total == len(want[1][1])
        if variant != "counts":
            idx = H.view(got["indices"], np.uint32)
            H.expect("the indices", idx[:total], want[1][1])
            assert bool(np.all(idx[total:] == 0xA5A5A5A5)), "stores behind the last index"
        if variant == "bits":
            H.expect("the surface bits", got["surface_bits"], capi.pack_bits_host(want[1][2]), capi.pack_bits_host(want[0][2]))
    j.check = check
    return j


def extrema_job(shape):
    j = Job()
    j.asynchronous = False                                       # (it synchronises its stream once per doubling round)
    f = [exact(shape, 11)[0], exact(shape, 12)[0]]
    want = [restated_extrema(x, RES) for x in f]
    j.inputs = {"sdf": tuple(f)}
    j.outputs = {"extremum": f[0].size * 4}
    j.call = lambda h, p, s: h.local_extrema_device(p["sdf"], shape, RES, p["extremum"], (1.0, 0.0, 0.0, 0.0), s)
    j.check = lambda host, got: H.expect("the extrema", capi.extremum_locations(H.view(got["extremum"], np.uint32), shape, RES), want[1], want[0])
    return j


JOBS = {
    "build_device": lambda: build_job("mask", S1, False),
    "build_device-border-40x33x35": lambda: build_job("mask", S2, True),
    "build_bits_device": lambda: build_job("bits", S2, False),
    "build_cells_device": lambda: build_job("cells", S1, True),
    "classify_cells_device-8": lambda: classify_job(8),
    "classify_cells_device-16": lambda: classify_job(16),
    "pack_bits_device": pack_job,
    "voxelize_points_device-clear": lambda: voxelize_job(False, True),
    "voxelize_points_device-accumulate": lambda: voxelize_job(False, False),
    "voxelize_points_bits_device-clear": lambda: voxelize_job(True, True),
    "voxelize_points_bits_device-accumulate": lambda: voxelize_job(True, False),
    "gradient_device-f32-vector": lambda: gradient_job(S1, False),
    "gradient_device-f32": lambda: gradient_job(S2, False),
    "gradient_device-f64": lambda: gradient_job(S2, True),
    "query_points_device": lambda: query_points_job(S2, False),
    "query_points_device-edge": lambda: query_points_job(S1, True),
    "query_gradients_device-smooth": lambda: query_gradients_job(S1, capi.QUERY_SMOOTH_GRADIENT),
    "query_gradients_device-autodiff": lambda: query_gradients_job(S2, capi.QUERY_AUTODIFF_GRADIENT),
    "query_gradients_device-boundary": lambda: query_gradients_job(S2, capi.QUERY_DISTANCE_TO_BOUNDARY),
    "project_points_device-out-of-collision": lambda: project_job(S2, False),
    "project_points_device-valid-volume": lambda: project_job(S1, True),
    "components_bits_device": lambda: components_job(S1),
    "component_topology_device": lambda: topology_job(S2, False),
    "component_topology_device-select": lambda: topology_job(S1, True),
    "component_surfaces_device-counts": lambda: surfaces_job(S1, 3, "counts"),
    "component_surfaces_device-indices": lambda: surfaces_job(S2, 3, "indices"),
    "component_surfaces_device-bits-two-sort-passes": lambda: surfaces_job(S1, 700, "bits"),
    "local_extrema_device": lambda: extrema_job(S2),
}


def run_job(h, delay, streams, job, asynchronous):
    case = H.Case(delay, streams[0], streams[1])
    p = _io(job, case)
    s = case.side.cuda_stream
    case.warm(lambda: job.call(h, p, s))
    case.arm()
    host = job.call(h, p, s)
    if asynchronous and job.asynchronous:
        case.witness("when the asynchronous call had returned")
    case.consume(job.inout)
    job.check(host, case.finish())
    return case


# ---- family 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(JOBS))
def test_each_call_honours_its_stream(ctx, delay, streams, name):
    run_job(ctx, delay, streams, JOBS[name](), not ctx.redzones)


@pytest.mark.parametrize("what", ["copy_from_host-small", "copy_from_host-pinned", "upload_classified-small", "upload_classified-staged"])
def test_uploads_land_behind_the_work_already_on_the_stream(ctx, delay, streams, what):
    """"enqueued on `stream` behind the work already there": the work there is a delayed fill of the destination with junk.  An
    upload that goes round the stream finishes during the delay and is overwritten."""
    rng = np.random.default_rng(5)
    if what.startswith("copy"):
        n = 100_000 if what.endswith("small") else (4 << 20) + 12_288           # either side of the 4 MiB pinned-chunk threshold
        src = rng.integers(0, 256, n, dtype=np.uint8)
        want, call = src, lambda h, p, s: h.copy_from_host(p, src, s)
    else:
        shape = S1 if what.endswith("small") else (128, 128, 129)                  # bits below / above the 256 KiB staged upload
        src = synth.bernoulli_mask(shape, 0.3, 19) * np.uint8(3)
        n = src.size
        want, call = (src != 0).astype(np.uint8), lambda h, p, s: h.upload_classified(p, filled=src, stream=s)
    case = H.Case(delay, streams[0], streams[1])
    dst = case.input("destination", np.full(n, H.SENTINEL, np.uint8), np.full(n, 0x77, np.uint8))
    case.warm(lambda: call(ctx, dst, case.side.cuda_stream))
    case.arm()
    call(ctx, dst, case.side.cuda_stream)
    case.consume(["destination"])
    H.expect("the destination", case.finish()["destination"], want)


@pytest.mark.parametrize("n", [100_000, (4 << 20) + 12_288], ids=["small", "pinned"])
def test_copy_to_host_reads_behind_the_work_already_on_the_stream(ctx, delay, streams, n):
    rng = np.random.default_rng(6)
    decoy, real = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    case = H.Case(delay, streams[0], streams[1])
    src = case.input("source", decoy, real)
    out = np.empty(n, np.uint8)
    case.warm(lambda: ctx.copy_to_host(out, src, case.side.cuda_stream))
    case.arm()
    got = ctx.copy_to_host(np.empty(n, np.uint8), src, case.side.cuda_stream).copy()
    case.finish()
    H.expect("the host copy", got, real, decoy)


# ---- family 2 ---------------------------------------------------------------------------------------------------------------------
FOLLOWERS = ["get_extrema", "query_points", "project_points", "query_gradients", "debug_copy_zsweep", "debug_copy_yzsweep"]


@pytest.mark.parametrize("first", FOLLOWERS)
def test_host_forms_straight_behind_a_delayed_build(ctx, delay, streams, first):
    """build_device on the side stream behind the delay; then, with no synchronisation by the caller, `first` and after it the
    others: each reflects the real scene (the header: the host forms run "behind this handle's last build", get_extrema and the
    debug hooks wait for it)."""
    shape = S1
    masks = [mask(shape, 11), mask(shape, 12)]
    want_sdf, want_ext = exact(shape, 12)
    assert exact(shape, 11)[1] != want_ext
    g, w = grid_points(shape, 31, 4000), world_points(shape, 12)
    zs, yzs = _exact_stage_fields(masks[1])
    host = host_field(shape, 12)
    followers = {
        "get_extrema": lambda: assert_equal(ctx.get_extrema(), want_ext),
        "query_points": lambda: [H.expect("query_points", a, b, eq=H.same_or_nan)
                                 for a, b in zip(ctx.query_points(out, shape, RES, g), A.query_points(want_sdf, RES, g))],
        "project_points": lambda: [H.expect("project_points", a, b) for a, b in zip(
            ctx.project_points(out, shape, RES, w, inverse(ORIGIN), ORIGIN, 1.5 * RES), host.ProjectOutOfCollisionNumpyHost(w, 1.5 * RES, 0.125, 0, False))],
        "query_gradients": lambda: [H.expect("query_gradients", a, b) for a, b in zip(
            ctx.query_gradients(out, shape, RES, w, inverse(ORIGIN), capi.QUERY_AUTODIFF_GRADIENT), host.QueryGradientsNumpyHost(w, capi.QUERY_AUTODIFF_GRADIENT, 0.0))],
        "debug_copy_zsweep": lambda: H.expect("the z sweep", ctx.debug_zsweep(shape), zs),
        "debug_copy_yzsweep": lambda: H.expect("the yz sweep", ctx.debug_yzsweep(shape), yzs),
    }
    ctx.set_option("dense", 0)                                   # the general pipeline: it leaves both intermediate fields
    try:
        case = H.Case(delay, streams[0], streams[1])
        d_in = case.input("mask", masks[0], masks[1])
        out = case.output("sdf", want_sdf.nbytes)
        s = case.side.cuda_stream

        def sequence():
            ctx.build_device(d_in, shape, out, RES, False, s)
            for name in [first] + [f for f in FOLLOWERS if f != first]:
                followers[name]()
        ctx.build_device(d_in, shape, out, RES, False, s)         # (warm: the decoy's results would fail the followers)
        ctx.query_points(out, shape, RES, g)
        ctx.project_points(out, shape, RES, w, inverse(ORIGIN), ORIGIN, 1.5 * RES)
        case.warm(lambda: ctx.build_device(d_in, shape, out, RES, False, s))
        case.arm()
        sequence()
        case.consume()
        H.expect("the field", H.view(case.finish()["sdf"], np.float32, shape), want_sdf, exact(shape, 11)[0])
    finally:
        ctx.set_option("dense", 1)


def assert_equal(a, b):
    assert a == b, (a, b)


def test_builds_the_stage_pair_and_a_batch_across_two_streams(ctx, delay, streams):
    """A whole build on stream A behind the delay, the tiered stage pair and a batch on stream B, a whole build on A again: all
    exact, and B's work does not start while A's build is pending.  Then the other way round: the stage pair on B behind a delay,
    a whole build on idle A must wait for it."""
    A_, B_ = streams
    sa, sb = A_.cuda_stream, B_.cuda_stream
    shape, vb = S1, True
    n = int(np.prod(shape))
    nb = int(np.prod(SB))
    batch = np.stack([mask(SB, 60 + b) for b in range(5)])
    res_b = np.array([1.0, 0.5, 0.25, 0.05, 0.037])
    want_b = [O.exact_sdf(batch[b], res_b[b], vb) for b in range(5)]
    d_batch, o_batch = H.to_device(batch), torch.zeros(5 * nb * 4, dtype=torch.uint8, device="cuda")
    d2, d3 = H.to_device(mask(shape, 13)), H.to_device(mask(shape, 14))
    plane, far = torch.zeros(n * 4, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.uint8, device="cuda")

    def stage_pair(d_mask, o, small):
        ctx.sweep_zy_tiered_device(d_mask, shape, plane.data_ptr(), far.data_ptr(), sb)
        ctx.sweep_x_lines_device(plane.data_ptr(), shape[0], shape[1], shape[2], 0, shape[1], RES, vb, o, small, sb)

    def check_pair(o, small, seed):
        H.expect("the stage pair's field", H.view(o.cpu().numpy(), np.float32, shape), exact(shape, seed, vb)[0])
        mx = H.view(small.cpu().numpy(), np.uint32)
        assert capi.extrema_from_dsq(int(mx[0]), int(mx[1]), RES) == exact(shape, seed, vb)[1]

    # 1. A is delayed; B and the second build on A follow
    case = H.Case(delay, side=A_)
    d1 = case.input("mask", mask(shape, 11), mask(shape, 12))
    o1 = case.output("sdf", n * 4)
    o2, o3 = [torch.full((n * 4,), H.SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    small = torch.zeros(16, dtype=torch.uint8, device="cuda")
    ctx.build_device(d1, shape, o1, RES, vb, sa)                  # warm: scratch and first-use tables of all three kinds of call
    stage_pair(d2.data_ptr(), o2.data_ptr(), small.data_ptr())
    ctx.build_batch_device(d_batch.data_ptr(), 5, SB, o_batch.data_ptr(), res_b.copy(), vb, sb)
    torch.cuda.synchronize()
    small.zero_()
    case.warm(lambda: ctx.build_device(d1, shape, o1, RES, vb, sa))
    case.arm()
    ctx.build_device(d1, shape, o1, RES, vb, sa)
    stage_pair(d2.data_ptr(), o2.data_ptr(), small.data_ptr())
    behind_pair = torch.cuda.Event()
    behind_pair.record(B_)
    ctx.build_batch_device(d_batch.data_ptr(), 5, SB, o_batch.data_ptr(), res_b.copy(), vb, sb)
    ctx.build_device(d3.data_ptr(), shape, o3.data_ptr(), RES, vb, sa)
    started_early = behind_pair.query()
    if not ctx.redzones:                                         # (with red zones every call has ended with a synchronisation)
        case.witness("when the stage pair's event had been queried")
    ext_batch = ctx.get_extrema_batch(5)
    ext3 = ctx.get_extrema()
    case.consume()
    got = case.finish()
    delay_ms = case.delay_ms
    assert ctx.redzones or not started_early, "the stage pair on stream B finished while the build on stream A was still behind its delay"
    H.expect("the first build", H.view(got["sdf"], np.float32, shape), exact(shape, 12, vb)[0], exact(shape, 11, vb)[0])
    check_pair(o2, small, 13)
    H.expect("the second build", H.view(o3.cpu().numpy(), np.float32, shape), exact(shape, 14, vb)[0])
    assert ext3 == exact(shape, 14, vb)[1]
    ob = H.view(o_batch.cpu().numpy(), np.float32, (5,) + SB)
    for b in range(5):
        H.expect("grid %d of the batch" % b, ob[b], want_b[b][0])
        assert ext_batch[b] == tuple(float(v) for v in want_b[b][1])

    # 2. B is delayed; the build on idle A follows
    case = H.Case(delay, side=B_)
    d2 = case.input("mask", mask(shape, 13), mask(shape, 15))
    o2 = case.output("sdf", n * 4)
    small.zero_()
    o3.fill_(H.SENTINEL)
    case.delay_ms = delay_ms
    case.arm()
    stage_pair(d2, o2, small.data_ptr())
    ctx.build_device(d3.data_ptr(), shape, o3.data_ptr(), RES, vb, sa)
    behind_build = torch.cuda.Event()
    behind_build.record(A_)
    started_early = behind_build.query()
    if not ctx.redzones:
        case.witness("when the build's event had been queried")
    case.consume()
    got = case.finish()
    assert ctx.redzones or not started_early, "the build on stream A finished while the stage pair on stream B was still behind its delay"
    check_pair(torch.from_numpy(got["sdf"]), small, 15)
    H.expect("the build behind the pair", H.view(o3.cpu().numpy(), np.float32, shape), exact(shape, 14, vb)[0])
    assert ctx.get_extrema() == exact(shape, 14, vb)[1]


# ---- family 3 ---------------------------------------------------------------------------------------------------------------------
PAIRS = {
    "components": (lambda: components_job(S1), lambda: components_job(S2)),
    "topology": (lambda: topology_job(S1, True), lambda: topology_job(S2, False)),
    "surfaces": (lambda: surfaces_job(S1, 700, "bits"), lambda: surfaces_job(S2, 3, "indices")),
    "extrema": (lambda: extrema_job(S1), lambda: extrema_job(S2)),
    "extrema-larger-first": (lambda: extrema_job(S2), lambda: extrema_job(S1)),
    "query_points": (lambda: query_points_job(S1, True), lambda: query_points_job(S2, False)),
    "project_points": (lambda: project_job(S1, False), lambda: project_job(S2, True)),
    "query_gradients": (lambda: query_gradients_job(S1, capi.QUERY_SMOOTH_GRADIENT), lambda: query_gradients_job(S2, capi.QUERY_AUTODIFF_GRADIENT)),
}


@pytest.mark.parametrize("handles", [1, 2], ids=["one-handle", "two-handles"])
@pytest.mark.parametrize("name", list(PAIRS))
def test_two_analysis_calls_on_two_side_streams(ctx, fresh, delay, streams, name, handles):
    """Two calls of different shapes back to back, each on its own side stream behind its own delay (the second's is half the
    first's: it has run out when the first call returns, so the second call's kernels start at once, beside whatever the first
    left pending).  On one handle they share its analysis scratch; on two handles nothing."""
    h1, h2 = ctx, (ctx if handles == 1 else fresh)
    if handles == 2:
        fresh.set_option("redzone", int(ctx.redzones))
    jobs = [f() for f in PAIRS[name]]
    cases = [H.Case(delay, streams[0]), H.Case(delay, streams[1])]
    ps = [_io(j, c) for j, c in zip(jobs, cases)]
    for h, j, c, p in zip((h1, h2), jobs, cases, ps):
        c.warm(lambda: j.call(h, p, c.side.cuda_stream))
    cases[0].delay_ms = max(cases[0].delay_ms, 2.0 * cases[1].delay_ms)
    for c in cases:
        c.arm()
    hosts = []
    for h, j, c, p in zip((h1, h2), jobs, cases, ps):
        hosts.append(j.call(h, p, c.side.cuda_stream))
        c.consume(j.inout)
    for j, c, host in zip(jobs, cases, hosts):
        j.check(host, c.finish())
