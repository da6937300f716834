#!/usr/bin/env python3
"""bench.py -- SDF build throughput on MI355X (BASELINE.json metric: Mvoxels/s, % HBM roofline).

A "step" is one pass of the hot path over one synthetic occupancy grid: device-resident uint8
mask -> device-resident fp32 signed distance field + extrema, through the C ABI
(libsdfgpu.so).  Inputs are i.i.d. Bernoulli(p = 0.5) occupancy,
generated directly in HBM before the timed region; the steps rotate over three different grids
(seeds 1, 2, 3) so that no step finds its input in the 256 MiB Infinity Cache.

  N = 1 : 512^3 (the configuration the metric is quoted on)
  N > 1 : one process per GPU, the grid cut into x slabs with an RCCL halo exchange
          (sdf_tools_amd/slab.py); weak scaling at 134 Mvoxel per GPU:
          N=2 1024x512x512, N=4 1024x1024x512, N=8 1024^3 (the metric's 8-GPU configuration).
          `python bench.py --gpus N` launches its own N ranks (re-exec through
          torch.distributed.run on 127.0.0.1); under an existing torchrun it uses the ranks it is given.

A plain run sets up, warms up, times the K steps, writes --dump-outputs if asked and prints ONE JSON line on
rank 0: the contract fields, the workload, the step against the compulsory bytes, the last step's extrema (N = 1)
and the ranks' self-check (N > 1).  Everything else runs only with `--full`, after the timed steps and untimed with
respect to `value`; the full detail is then printed first, as a `BENCH_FULL {...}` line.  At N = 1:
  roofline      dominant kernel of the timed steps: HIP-event duration, compulsory bytes, PMC traffic
  value_without_stage_events, value_repeats, bits_entry   the timed loop again: no events, five repeats, bits input
  legs          the other tiers at the same 512^3 size: general (separable sweeps) tier on the headline
                input, a sparse Bernoulli grid, the streaming two-box point cloud; and BASELINE configs[1], the
                256^3 grid (throughput reported, parity in tests/)  [--no-legs drops them and parity]
  parity        voxels that differ from the reference algorithm (oracle) on 128^3 samples
  host_api, cpu_baseline   host-buffer calls of the library; the oracle timed on this host  [--no-cpu-baseline]
and with the slab builder: the roofline of its ball kernel, `vs_1gpu_same_grid` (the same grid on one GPU) and, at
N = 1 (--force-slab), `multi_native_on_one_gpu`.

`--dump-outputs DIR` (N = 1) writes what the last timed step returned to its caller -- the fp32 field (whole up to 4 Mvoxel,
else a fixed seeded sample with its voxel indices) and the fp64 extrema -- as DIR/*.npy, so two builds can be compared.
"""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s peak
# Compulsory bytes per voxel of each kernel (what it must read + write once):
#   pack 1 B mask in + 1/8 B bits out; ball 1/8 in + 4 out; z sweep 1 + 2; y sweep 2 + 2 (16-bit plane field) or
#   2 + 4 (int32); fused z+y 1 + 2 (or 1 + 4); x sweep 2 + 4 (or 4 + 4); envelope sweeps like the marching ones.
B_KERNEL16 = {"pack_bits": 1.125, "dense_ball": 4.125, "sweep_z": 3, "sweep_y": 4, "sweep_zy": 3, "sweep_x": 6,
              "envelope_y": 4, "envelope_x": 6}
B_KERNEL32 = {"pack_bits": 1.125, "dense_ball": 4.125, "sweep_z": 3, "sweep_y": 6, "sweep_zy": 5, "sweep_x": 8,
              "envelope_y": 6, "envelope_x": 8}
# SURVEY.md 8(d)'s algorithmic figure for the separable formulation (K1 1+2, K2 2+4, K3 4+4 = 17 B/voxel),
# attributed to the kernel that does that part of the work; reported as roofline.alg_equiv, never as frac.
B_ALG = {"pack_bits": 1, "dense_ball": 16, "sweep_z": 3, "sweep_y": 6, "sweep_zy": 9, "sweep_x": 8,
         "envelope_y": 6, "envelope_x": 8}
B_ALG_TOTAL = 17
B_COMPULSORY_TOTAL = 5          # mask in + fp32 out
KERNEL_NAMES = {"envelope_y": "k_envelope_dc<2>", "envelope_x": "k_envelope_dc<3>",
                "pack_bits": "k_pack_bits_mask", "dense_ball": "k_ball_dense", "sweep_z": "k_sweep_z_wave16",
                "sweep_y": "k_sweep_y16 (k_sweep_march<2> on shapes without the 16-bit plane field)", "sweep_zy": "k_sweep_zy_fused",
                "sweep_x": "k_sweep_x16 (k_sweep_march<3> on shapes without the 16-bit plane field)"}
STAGES = ["pack_bits", "dense_ball", "sweep_z", "sweep_y", "envelope_y", "sweep_x", "envelope_x"]
# profiles/traffic.json keys per stage: exact kernels (VERDICT r3 weak #6b: a prefix match had averaged KD with the
# guarded no-op launches of KD3, and the p = 0.03 leg quoted KD's bytes for KD3 + KF)
TRAFFIC_KEY = {"pack_bits": "k_pack_bits_mask", "dense_ball": "k_ball_dense", "sweep_z": "k_sweep_z_wave16",
               "sweep_y": "k_sweep_y16", "sweep_zy": "k_sweep_zy_fused", "sweep_x": "k_sweep_x16",
               "envelope_y": "k_envelope_dc<2>", "envelope_x": "k_envelope_dc<3>"}

GRIDS = {1: (512, 512, 512), 2: (1024, 512, 512), 4: (1024, 1024, 512), 8: (1024, 1024, 1024)}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, nargs=3, default=None, help="override grid nx ny nz")
    ap.add_argument("--p", type=float, default=0.5, help="Bernoulli occupancy probability")
    ap.add_argument("--resolution", type=float, default=0.01)
    ap.add_argument("--halo", type=int, default=3)
    ap.add_argument("--masks", type=int, default=3, help="distinct input grids the steps rotate over")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check what the headline figure does not need: roofline, "
                         "repeats, bits entry, tier legs, parity, host calls, CPU baseline, slab comparisons")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the host-buffer calls and the CPU baseline")
    ap.add_argument("--no-legs", action="store_true", help="with --full: skip the extra (untimed) tier legs and the parity counts")
    ap.add_argument("--cpu-sample", type=int, default=0,
                    help="with --full: edge of the cube timed on the CPU oracle (0 = 512 if the host has the memory, else 320)")
    ap.add_argument("--tune", type=int, nargs=2, default=None, help="rows per chunk: y x")
    ap.add_argument("--no-profile", action="store_true", help="do not record per-stage HIP events in the timed region")
    ap.add_argument("--force-slab", action="store_true", help="run the multi-GPU slab builder even at N = 1")
    ap.add_argument("--opt", action="append", default=[], help="library option name=value (sdfgpu_set_option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (field, or a fixed seeded sample of it, and extrema) as DIR/*.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and (args.gpus > 1 or args.force_slab):
        ap.error("--dump-outputs covers the single-GPU path (--gpus 1 without --force-slab)")
    return args


def relaunch_as_ranks(n):
    """`python bench.py --gpus N` without a launcher: become N ranks (one per GPU) through torch.distributed.run."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.execvpe(sys.executable, cmd, env)


def host_mem_available_gb():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / 1048576.0
    except Exception:
        pass
    return 0.0


def cpu_baseline(sample_n, p, resolution):
    """Times the CPU oracle (kind = "port": the C restatement of the reference's single-threaded
    bucket-queue BuildDistanceField path) on the same generator as the GPU workload."""
    from oracle import oracle as O
    from sdf_tools_amd import synth

    if sample_n <= 0:       # the full 512^3 workload needs ~23 GB and ~35 s; fall back to a 320^3 sample on small hosts
        sample_n = 512 if host_mem_available_gb() >= 96.0 else 320
    m = synth.bernoulli_mask((sample_n,) * 3, p, 1)
    t0 = time.perf_counter()
    O.reference_sdf(m, resolution)
    dt = time.perf_counter() - t0
    return {"value": round(m.size / dt / 1e6, 4), "unit": "Mvoxels/s", "cores": 1, "kind": "port",
            "host_cores": os.cpu_count(), "seconds": round(dt, 2),
            "sample": "%d^3 Bernoulli(p=%g) occupancy grid (seed 1), same generator and resolution as the GPU workload%s; "
                      "single-threaded like the reference" % (sample_n, p, " = the full workload" if sample_n == 512 else "")}


def class_seam_block(shape, res):
    """512^3 CollisionMapGrid::ExtractSignedDistanceField(oob, unknown_is_filled, false), host cells in -> host field out:
    the C++ client binary and the pybind call.  Untimed legs; PCIe inclusive; never `value`."""
    import subprocess

    import numpy as np

    from sdf_tools_amd import build as b
    from sdf_tools_amd._bindings import load_pysdf_tools
    n = shape[0]
    out = {"call": "CollisionMapGrid::ExtractSignedDistanceField(oob, true, false), %d^3 COLLISION_CELL map (host) -> "
                   "SignedDistanceField (host)" % n}
    if len(set(shape)) == 1:
        exe = b.build_example("class_seam")
        r = subprocess.run([exe, str(n), "3", "0.5"], capture_output=True, text=True, timeout=900)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode == 0 and line:
            cpp = json.loads(line[-1])
            out["cpp_ms"] = cpp["min_ms"]
            out["cpp_all_ms"] = cpp["all_ms"]
            out["cpp_bit_identical_to_sdfgpu_build"] = cpp["bit_identical_to_sdfgpu_build"]
        else:
            out["cpp_error"] = (r.stdout + r.stderr)[-400:]
    m = load_pysdf_tools()
    origin = m.Isometry3d([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    g = m.CollisionMapGrid(origin, "world", res, shape[0], shape[1], shape[2], m.COLLISION_CELL(0.0))
    occ = (np.random.default_rng(5).random(shape, dtype=np.float32) < 0.5).astype(np.float32)
    g.SetOccupancyFromNumpy(occ)
    del occ
    keep = [g.ExtractSignedDistanceField(float("inf"), True, False)]      # warm-up (context, device buffers, pinned staging)
    t_py = []
    for _ in range(3):
        t1 = time.perf_counter()
        keep.append(g.ExtractSignedDistanceField(float("inf"), True, False))    # (kept: dropping a 512 MiB result is the caller's munmap)
        t_py.append(time.perf_counter() - t1)
        keep.pop(0)
    out["pybind_ms"] = round(min(t_py) * 1e3, 2)
    out["pybind_all_ms"] = [round(t * 1e3, 2) for t in t_py]
    out["note"] = ("1 GiB of cells is classified to 16 MiB of bits by the host thread team, uploaded, built, and the 512 MiB field "
                   "is drained into uninitialised storage by the same team; round 4 measured 241 ms for this call")
    return out


def load_traffic():
    """HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/traffic.json), if any."""
    path = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(path):
        try:
            return json.load(open(path))
        except Exception:
            return None
    return None


def load_rocprof_times():
    """profiles/kernel_times.json: {kernel name fragment: average ms} from the committed rocprofv3 --stats summary of the
    bench command (written by tools/profile_round.sh); None if absent."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "kernel_times.json")
    try:
        with open(path) as f:
            return json.load(f)
    except Exception:
        return None


def stage_table(ctx, ms_sum, builds, n_total):
    """Per-stage average ms of the profiled builds -> {stage: ms}, kernels used, dominant stage."""
    info = ctx.last_build_info()
    info.update(ctx.last_path())
    avg = [v / max(builds, 1) for v in ms_sum]
    stage_ms = {}
    if info["dense"]:
        stage_ms["pack_bits"], stage_ms["dense_ball"] = avg[0], avg[1]
    if not info["dense_certified"]:
        if info["fused_zy"]:
            stage_ms["sweep_zy"] = avg[3]
        else:
            stage_ms["sweep_z"], stage_ms["sweep_y"] = avg[2], avg[3]
        stage_ms["sweep_x"] = avg[5]
        if info["far_y"] or avg[4] > 0.02:
            stage_ms["envelope_y"] = avg[4]
        if info["far_x"] or avg[6] > 0.02:
            stage_ms["envelope_x"] = avg[6]
    stage_ms = {k: v for k, v in stage_ms.items() if v > 0.0005}
    return info, avg, stage_ms


def roofline_of(stage, ms, n_total, plane16, traffic_table=None, info=None):
    bk = (B_KERNEL16 if plane16 else B_KERNEL32)[stage]
    if info and info.get("far_y") and info.get("far_x") and stage.startswith("envelope"):
        bk = B_KERNEL32[stage]      # far-field pair: exact int32 plane field between the two sweeps (4 B/voxel)
    achieved = n_total * bk / (ms * 1e-3) / 1e9
    kernel, tkey = KERNEL_NAMES[stage], TRAFFIC_KEY.get(stage)
    if stage == "dense_ball" and info and (info.get("dense3") or info.get("dense3_staged")):
        # the stage slot holds the dense tier's wide form: KD3 + the fix-up kernel (behind KD when staged)
        kernel = ("k_ball_dense + " if info.get("dense3_staged") else "") + "k_ball_dense3 + k_ball_fixup"
        tkey = "k_ball_dense3+k_ball_fixup" if not info.get("dense3_staged") else None
    tr = (traffic_table or {}).get(tkey) if (n_total == 512 ** 3 and tkey) else None
    r = {"bound": "hbm", "kernel": kernel, "stage": stage,
         "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
         "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": tr,
         "bytes_per_voxel": bk, "avg_ms": round(ms, 4)}
    if tr:
        r["traffic_frac"] = round(tr / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
        r["traffic_over_compulsory"] = round(tr / (n_total * bk), 3)
    alg = n_total * B_ALG[stage] / (ms * 1e-3) / 1e9
    r["alg_equiv"] = {"bytes_per_voxel": B_ALG[stage], "achieved": round(alg, 1), "ratio_to_peak": round(alg / HBM_PEAK_GBPS, 4),
                      "note": "SURVEY 8(d) bytes of the three materialised sweeps attributed to this kernel; a fused / "
                              "bit-parallel kernel moves fewer bytes, so this is an equivalence figure, not a hardware fraction"}
    return r


DUMP_FULL_MAX_VOXELS = 1 << 22      # fields up to 16 MB are written whole; larger ones as a seeded sample of this many draws


def dump_outputs(d, out, extrema):
    """--dump-outputs: the device field `out` and the build's (max, min) as .npy files under `d` (64 MB at most in all).
    Large fields are sampled at voxel indices drawn with a fixed seed (sorted, duplicates dropped), so two runs with the
    same arguments -- or two builds of the project -- write the same voxels; the indices are written beside the values."""
    import numpy as np
    import torch

    os.makedirs(d, exist_ok=True)
    n_total = out.numel()
    if n_total <= DUMP_FULL_MAX_VOXELS:
        np.save(os.path.join(d, "sdf.npy"), out.cpu().numpy().astype(np.float32))
    else:
        idx = np.unique(np.random.default_rng(0).integers(0, n_total, size=DUMP_FULL_MAX_VOXELS, dtype=np.int64))
        vals = out.reshape(-1)[torch.from_numpy(idx).to(out.device)].cpu().numpy()
        np.save(os.path.join(d, "sdf_sample.npy"), vals.astype(np.float32))
        np.save(os.path.join(d, "sdf_sample_index.npy"), idx.astype(np.float64))     # flat x*ny*nz + y*nz + z, exact below 2^53
    np.save(os.path.join(d, "extrema.npy"), np.asarray(extrema, dtype=np.float64))


def timed_loop(step, steps, fence):
    fence()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    fence()
    return time.perf_counter() - t0


def run_leg(torch, capi, dev, shape, res, masks, opts, steps, warmup, label):
    """One extra (untimed w.r.t. `value`) leg: its own context, its own loop, per-stage HIP events."""
    ctx = capi.SdfGpu(dev.index)
    for k, v in opts.items():
        ctx.set_option(k, v)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n_total = shape[0] * shape[1] * shape[2]

    def step(i):
        ctx.build_device(masks[i % len(masks)].data_ptr(), shape, out.data_ptr(), res, False, stream)

    def fence():
        torch.cuda.synchronize(dev)

    # a fresh context on this scene (what a one-shot caller of the reference API pays); a throw-away context builds the
    # scene once first so that process-level one-time costs (first launch of each kernel) are not billed to it
    warm = capi.SdfGpu(dev.index)
    for k, v in opts.items():
        warm.set_option(k, v)
    warm.build_device(masks[0].data_ptr(), shape, out.data_ptr(), res, False, stream)
    fence()
    warm.close()
    t_first0 = time.perf_counter()
    step(0)
    fence()
    first_ms = (time.perf_counter() - t_first0) * 1e3
    for i in range(warmup):
        step(i)
        fence()
    dt = timed_loop(step, steps, fence)
    ctx.get_stage_times()
    ctx.set_profiling(1)
    timed_loop(step, min(steps, 20), fence)
    ms_sum, builds = ctx.get_stage_times()
    ctx.set_profiling(0)
    info, avg, stage_ms = stage_table(ctx, ms_sum, builds, n_total)
    leg = {"workload": label, "ms_per_step": round(dt / steps * 1e3, 4),
           "Mvoxels_per_s": round(n_total / (dt / steps) / 1e6, 1),
           "first_build_ms_fresh_context": round(first_ms, 3),
           "pipeline_frac_compulsory": round(n_total * B_COMPULSORY_TOTAL / (dt / steps) / 1e9 / HBM_PEAK_GBPS, 4),
           "kernels": info, "stages_ms": {k: round(v, 4) for k, v in stage_ms.items()}, "extrema": list(ctx.get_extrema())}
    if stage_ms:
        dom = max(stage_ms, key=stage_ms.get)
        leg["roofline"] = roofline_of(dom, stage_ms[dom], n_total, info["plane16"], load_traffic(), info)
    ctx.close()
    return leg


def streaming_leg(torch, dev, n, res, frames, n_query=1 << 20):
    """BASELINE configs[4]: 200 k points / frame -> occupancy -> SDF -> the consumer's EstimateDistance + gradient queries
    (1 M points, one fused gather kernel) at n^3, everything in HBM.  The full-grid gradient variant (what round 3
    reported as the frame: +1.6 GB written per frame) is timed beside it."""
    from sdf_tools_amd import synth
    from sdf_tools_amd.streaming import StreamingSdf

    clouds = [torch.from_numpy(synth.two_box_points(200000, seed=f, scale=n * res)).to(dev) for f in range(4)]
    gen = torch.Generator(device=dev).manual_seed(0)
    qpts = torch.rand((n_query, 3), dtype=torch.float64, device=dev, generator=gen) * (n * res)

    def run(mode):
        st = StreamingSdf((n, n, n), res, (0.0, 0.0, 0.0), dev.index, gradient=mode)
        warm = StreamingSdf((n, n, n), res, (0.0, 0.0, 0.0), dev.index, gradient=mode)      # process-level warm-up (see run_leg)
        q = qpts if mode == "query" else None
        warm.frame(clouds[0], q)
        torch.cuda.synchronize(dev)
        warm.ctx.close()
        del warm
        t0 = time.perf_counter()
        st.frame(clouds[0], q)
        torch.cuda.synchronize(dev)
        first_ms = (time.perf_counter() - t0) * 1e3
        for f in range(3):
            st.frame(clouds[f % 4], q)
            torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for f in range(frames):
            st.frame(clouds[f % 4], q)
        torch.cuda.synchronize(dev)
        return st, (time.perf_counter() - t0) / frames * 1e3, first_ms

    st, ms_q, first_q = run("query")
    st.ctx.get_stage_times()
    st.ctx.set_profiling(1)
    for f in range(8):
        st.frame(clouds[f % 4], qpts)
    torch.cuda.synchronize(dev)
    ms_sum, builds = st.ctx.get_stage_times()
    st.ctx.set_profiling(0)
    info, avg, stage_ms = stage_table(st.ctx, ms_sum, builds, n ** 3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        st.query(qpts)
    e1.record()
    torch.cuda.synchronize(dev)
    leg = {"workload": "200 k points in two boxes (scripts/3d_sdf_demo_rviz.py pattern) -> %d^3 occupancy @ %g m -> SDF -> "
                       "%d EstimateDistance + gradient queries (one fused gather kernel), per frame" % (n, res, n_query),
           "frames_per_s": round(1e3 / ms_q, 1), "ms_per_frame": round(ms_q, 3), "target_hz": 30,
           "first_frame_ms_fresh_context": round(first_q, 3), "query_ms": round(e0.elapsed_time(e1) / 10, 4),
           "kernels": info, "stages_ms": {k: round(v, 4) for k, v in stage_ms.items()}, "extrema": list(st.extrema())}
    if stage_ms:
        dom = max(stage_ms, key=stage_ms.get)
        leg["roofline"] = roofline_of(dom, stage_ms[dom], n ** 3, info["plane16"], load_traffic(), info)
    st.ctx.close()
    del st
    st2, ms_full, first_full = run("full")
    leg["full_grid_gradient_variant"] = {"what": "the same frames with the grid-aligned gradient of EVERY voxel written (k_gradient_f32x4, "
                                                 "12 B/voxel out) instead of the query kernel: GetFullGradient callers",
                                         "ms_per_frame": round(ms_full, 3), "frames_per_s": round(1e3 / ms_full, 1),
                                         "first_frame_ms_fresh_context": round(first_full, 3)}
    st2.ctx.close()
    return leg


def parity_counts(ctx, res):
    """Voxels whose GPU value differs from the reference algorithm (the oracle's restatement of the bucket-queue
    propagation) on 128^3 samples of the benchmark generators.  The reference is exact wherever the true squared
    distance is < 8 and over-estimates a few voxels beyond; every mismatch is checked to be such an over-estimate
    (GPU == exact EDT, |reference| > |GPU|)."""
    import numpy as np

    from oracle import oracle as O
    from sdf_tools_amd import synth

    out = {"tolerance": 1e-5, "sample": "128^3, resolution %g" % res, "cases": {}}
    for name, p, seed in (("bernoulli_p0.5", 0.5, 1), ("bernoulli_p0.01", 0.01, 2)):
        m = synth.bernoulli_mask((128, 128, 128), p, seed)
        got, ext = ctx.build(m, res)
        ref, ref_ext = O.reference_sdf(m, res)
        ex, ex_ext, _ = O.exact_sdf(m, res)
        diff = np.abs(got.astype(np.float64) - ref.astype(np.float64)) > 1e-5
        n_diff = int(diff.sum())
        bit_equal_exact = bool(np.array_equal(got.view(np.uint32), ex.view(np.uint32)))
        over = int((np.abs(ref[diff]) > np.abs(got[diff])).sum()) if n_diff else 0
        out["cases"][name] = {"voxels": int(m.size), "differ_from_reference_gt_tol": n_diff,
                              "of_which_reference_overestimates": over,
                              "gpu_bit_equal_to_exact_edt": bit_equal_exact,
                              "sign_mismatches": int(((got < 0) != (m != 0)).sum()),
                              "extrema_equal_reference": bool(ext == ref_ext)}
    return out


CONTRACT_KEYS = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data"]


def summary_line(result):
    """The ONE line the driver parses (VERDICT r5 "next round" 7): the contract fields, `roofline`, `cpu_baseline` and a short
    summary of everything else -- round 5's single line had grown past the driver's stdout tail and lost its head."""
    out = {k: result[k] for k in CONTRACT_KEYS if k in result}
    cfg = result.get("config", {})
    out["config"] = {k: cfg[k] for k in ("workload", "grid", "voxels", "partition") if k in cfg}
    r = result.get("roofline")
    if r:
        out["roofline"] = {k: r[k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "bytes_per_voxel", "avg_ms",
                                             "rocprof_avg_ms", "traffic_frac", "traffic_over_compulsory", "launches_timed") if k in r}
    if "cpu_baseline" in result:
        out["cpu_baseline"] = result["cpu_baseline"]
    for k in ("value_without_stage_events", "extrema", "vs_1gpu_same_grid", "multi_gpu"):
        if k in result:
            out[k] = result[k]
    if "value_repeats" in result:
        out["value_repeats"] = {k: result["value_repeats"][k] for k in ("min", "median", "max")}
    if "pipeline" in result:
        out["pipeline_frac_of_hbm_peak"] = result["pipeline"]["frac_of_hbm_peak"]
    b = result.get("bits_entry")
    if b:
        out["bits_entry"] = {k: b[k] for k in ("ms_per_step", "Mvoxels_per_s", "frac_of_hbm_peak", "bit_identical_to_the_mask_build", "error") if k in b}
    legs = {}
    for name, leg in (result.get("legs") or {}).items():
        if not isinstance(leg, dict):
            legs[name] = str(leg)[:80]
            continue
        ent = {"ms": leg.get("ms_per_step", leg.get("ms_per_frame"))}
        if "frames_per_s" in leg:
            ent["hz"] = leg["frames_per_s"]
        lr = leg.get("roofline")
        if lr:
            ent["kernel"], ent["frac"] = lr["stage"], lr["frac"]
        if "error" in leg:
            ent = {"error": leg["error"][:80]}
        legs[name] = ent
    if legs:
        out["legs"] = legs
    p = result.get("parity", {}).get("cases")
    if p:
        out["parity"] = {k: [v["differ_from_reference_gt_tol"], v["of_which_reference_overestimates"], v["gpu_bit_equal_to_exact_edt"]]
                         for k, v in p.items()}
        out["parity_key"] = "[voxels differing from the reference algorithm by > 1e-5, of which reference over-estimates, GPU bit-equal to the exact EDT]"
    h = result.get("host_api")
    if h:
        out["host_api_ms"] = {"sdfgpu_build": h.get("ms"), "to_device": (h.get("device_resident") or {}).get("build_ms"),
                              "class_seam_cpp": (h.get("class_seam") or {}).get("cpp_ms"), "class_seam_pybind": (h.get("class_seam") or {}).get("pybind_ms")}
    return out


def emit(result):
    """--full: the whole result as a `BENCH_FULL {...}` line (also written to a file), then the summary line."""
    full = json.dumps(result)
    print("BENCH_FULL " + full, flush=True)
    line = summary_line(result)
    line["full_detail"] = "the line above (BENCH_FULL ...)"
    try:
        d = os.path.join(ROOT, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "bench_full.json"), "w") as f:
            f.write(full + "\n")
        line["full_detail"] += " and " + os.path.relpath(f.name, ROOT)
    except Exception:
        pass
    print(json.dumps(line), flush=True)


def main():
    args = parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: required for RCCL between processes here
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_as_ranks(args.gpus)                                # does not return
    import torch
    import torch.distributed as dist

    from sdf_tools_amd import capi, slab, synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("--gpus %d does not match the launcher's WORLD_SIZE %d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the SDF build path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if torch.cuda.device_count() < world:
            raise SystemExit("bench.py --gpus %d: this node shows %d GPU(s); one process per GPU is the only supported layout"
                             % (world, torch.cuda.device_count()))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        # start-up self-check (VERDICT r3 "next round" 5): every rank answers over RCCL before anything is timed
        probe = torch.tensor([float(rank)], dtype=torch.float64, device=dev)
        seen = [torch.zeros_like(probe) for _ in range(world)]
        dist.all_gather(seen, probe)
        seen = sorted(int(t.item()) for t in seen)
        if seen != list(range(world)) or dist.get_backend() != "nccl":
            raise SystemExit("bench.py --gpus %d: start-up self-check failed: ranks seen %s over backend %s" %
                             (world, seen, dist.get_backend()))

    shape = tuple(args.size) if args.size else GRIDS.get(world, (128 * world, 1024, 1024))
    nx, ny, nz = shape
    n_total = nx * ny * nz
    res = args.resolution
    stream = torch.cuda.current_stream(dev)
    n_masks = max(1, args.masks)

    use_slab = world > 1 or args.force_slab
    if not use_slab:
        ctx = capi.SdfGpu(local_rank)
        if args.tune:
            ctx.set_tuning(*args.tune)
        for kv in args.opt:
            ctx.set_option(kv.split("=")[0], int(kv.split("=")[1]))
        masks = [synth.bernoulli_mask_torch(shape, args.p, 1 + k, device=dev) for k in range(n_masks)]
        out = torch.empty(shape, dtype=torch.float32, device=dev)

        def step(i):
            ctx.build_device(masks[i % n_masks].data_ptr(), shape, out.data_ptr(), res, False, stream.cuda_stream)
    else:
        stages = slab.HipStages(local_rank)
        ctx = stages.ctx
        if args.tune:
            ctx.set_tuning(*args.tune)
        for kv in args.opt:
            ctx.set_option(kv.split("=")[0], int(kv.split("=")[1]))
        x0, x1 = slab.slab_range(nx, rank, world)
        masks = [synth.bernoulli_mask_torch(shape, args.p, 1 + k, x_range=(x0, x1), device=dev) for k in range(n_masks)]
        builder = slab.SlabSdfBuilder(stages, shape, res, False, halo=args.halo, rank=rank, world=world)
        pending = []

        def step(i):
            # enqueue this build, then validate the previous one (its all-reduced status has already
            # landed in pinned host memory): every build is validated inside the timed region, but the
            # GPUs never wait for the host between builds
            pending.append(builder.build_async(masks[i % n_masks]))
            if len(pending) > 1:
                builder.finish(pending.pop(0))

        def drain():
            while pending:
                builder.finish(pending.pop(0))

    def fence():
        if use_slab:
            drain()
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize(dev)

    for i in range(args.warmup):
        step(i)
        torch.cuda.synchronize(dev)     # untimed: lets the handle's policy see each warm-up build before the next one
    fence()
    if use_slab and not args.no_profile:
        builder.time_ball_kernel(4)     # events around the dominant kernel of every 4th build, on its launch stream
    dominant_only = False
    if not use_slab:
        ctx.get_stage_times()           # drop anything recorded so far
        # HIP events on the launch stream inside the timed region: around the dominant kernel only when the
        # warm-up builds were dense-certified (2 events on every 4th build), around every stage otherwise
        try:
            dominant_only = bool(ctx.last_path().get("dense_certified")) and not args.no_profile
        except Exception:               # no warm-up build yet
            dominant_only = False
        ctx.set_profiling(0 if args.no_profile else (3 if dominant_only else 1))
    dt = timed_loop(step, args.steps, fence)
    if args.dump_outputs:           # before any later loop touches `out`: the last timed step's field and extrema
        dump_outputs(args.dump_outputs, out, ctx.get_extrema())
    per_rank_ms = [dt / args.steps * 1e3]
    if world > 1:
        mine = torch.tensor([dt, float(rank)], dtype=torch.float64, device=dev)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)                                # (RCCL: each rank's own clock around the same K steps)
        per_rank_ms = [float(e[0].item()) / args.steps * 1e3 for e in every]
        ranks_seen = sorted(int(e[1].item()) for e in every)
        dt = max(float(e[0].item()) for e in every)

    ms_per_step = dt / args.steps * 1e3
    value = n_total / (dt / args.steps) / 1e6
    result = {
        "metric": "Mvoxels/sec SDF build", "value": round(value, 2), "unit": "Mvoxels/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "int32", "data": "synthetic",
        "config": {"workload": "%dx%dx%d uint8 occupancy grid, Bernoulli(p=%g), %d grids (seeds 1..%d) in rotation, "
                               "resolution %g, no virtual border; device-resident mask -> device-resident fp32 SDF + extrema"
                               % (nx, ny, nz, args.p, n_masks, n_masks, res),
                   "grid": list(shape), "voxels": n_total,
                   "partition": "single GPU" if world == 1 else
                   "x-slab x%d; RCCL halo exchange: 2 bit-planes (dense path) / %d int32 planes (general path)"
                   % (world, args.halo)},
    }
    if world > 1:
        # first contact with a multi-GPU node must be boring: a line whose ranks did not all take part, or whose exchange did
        # not run over RCCL, is not a measurement of the 8-GPU configuration -- say so and stop instead of printing it
        if ranks_seen != list(range(world)) or dist.get_backend() != "nccl":
            raise SystemExit("bench.py --gpus %d: self-check failed (ranks seen %s, backend %s): refusing to report a "
                             "multi-GPU number that was not measured on %d RCCL ranks" % (world, ranks_seen, dist.get_backend(), world))
        result["multi_gpu"] = {"ranks_seen": ranks_seen, "rccl": dist.get_backend() == "nccl",
                               "ms_per_step_by_rank": [round(v, 4) for v in per_rank_ms],
                               "general_path_builds": builder.general_builds, "whole_line_sweeps": builder.fallbacks,
                               "general_path_host_reads": builder.host_reads, "general_path_mispredictions": builder.mispredictions}
    if use_slab and args.full:
        # (also at world = 1 with --force-slab: the same code path runs on a one-GPU box every round)
        # BASELINE.md section 3's target is ">= 6x at 8 GPUs ON 1024^3": the denominator is the SAME grid on ONE GPU, not the
        # 512^3 N = 1 line.  Rank 0 builds the whole grid of this run through the single-GPU ABI (same masks' seeds, same
        # timing discipline, fewer steps) while the other ranks wait at the barrier; value / that rate = vs_1gpu_same_grid.
        same = None
        if rank == 0:
            try:
                one = capi.SdfGpu(local_rank)
                whole = [synth.bernoulli_mask_torch(shape, args.p, 1 + k, device=dev) for k in range(min(n_masks, 2))]
                o1 = torch.empty(shape, dtype=torch.float32, device=dev)

                def one_step(i):
                    one.build_device(whole[i % len(whole)].data_ptr(), shape, o1.data_ptr(), res, False, stream.cuda_stream)

                for i in range(5):
                    one_step(i)
                    torch.cuda.synchronize(dev)
                k1 = max(5, min(args.steps, 20))
                dt1 = timed_loop(one_step, k1, lambda: torch.cuda.synchronize(dev))
                rate1 = n_total / (dt1 / k1) / 1e6
                same = {"single_gpu_ms_per_step": round(dt1 / k1 * 1e3, 4), "single_gpu_Mvoxels_per_s": round(rate1, 2),
                        "speedup": round(value / rate1, 3), "steps": k1,
                        "note": "the whole %dx%dx%d grid of this run on rank 0's GPU alone through sdfgpu_build_device" % shape}
                one.close()
                del whole, o1
                torch.cuda.empty_cache()
            except Exception as e:
                same = {"error": repr(e)}
        if world > 1:
            dist.barrier()
        if rank == 0:
            result["vs_1gpu_same_grid"] = same
    # whole step against the compulsory 5 B/voxel (mask in, fp32 out) and against SURVEY 8(d)'s 17 B/voxel
    result["pipeline"] = {
        "compulsory_bytes_per_voxel": B_COMPULSORY_TOTAL,
        "frac_of_hbm_peak": round(n_total * B_COMPULSORY_TOTAL / (dt / args.steps) / 1e9 / HBM_PEAK_GBPS / world, 4),
        "alg_equiv": {"bytes_per_voxel": B_ALG_TOTAL,
                      "ratio_to_peak": round(n_total * B_ALG_TOTAL / (dt / args.steps) / 1e9 / HBM_PEAK_GBPS / world, 4)},
    }

    if not use_slab and not args.full:
        result["extrema"] = list(ctx.get_extrema())
    elif not use_slab:
        ms_sum, builds = ctx.get_stage_times()
        ctx.set_profiling(False)
        if not args.no_profile and dominant_only:
            # per-stage breakdown from a second, untimed pass with an event behind every stage
            dominant_ms = ms_sum[1] / max(builds, 1)
            ctx.set_profiling(1)
            timed_loop(step, min(args.steps, 50), fence)
            ms_sum, builds = ctx.get_stage_times()
            ctx.set_profiling(False)
            ms_sum = list(ms_sum)
            result["config"]["stage_breakdown"] = ("untimed second pass with an event behind every stage; dense_ball from "
                                                   "the timed pass (events around it on every 4th build)")
            ms_sum[1] = dominant_ms * builds
        if not args.no_profile:
            # the same steps again without any HIP events: reported next to `value`, never instead of it
            dt2 = timed_loop(step, args.steps, fence)
            result["value_without_stage_events"] = round(n_total / (dt2 / args.steps) / 1e6, 2)
        # spread: the same K-step loop five more times (`value` stays the first, contract-timed loop)
        reps = sorted(n_total / (timed_loop(step, args.steps, fence) / args.steps) / 1e6 for _ in range(5))
        result["value_repeats"] = {"n": 5, "min": round(reps[0], 2), "median": round(reps[2], 2), "max": round(reps[4], 2),
                                   "note": "five more runs of the same timed loop (events off), Mvoxels/s"}
        mx, mn = ctx.get_extrema()
        result["extrema"] = [mx, mn]
        # the same K steps through the BITS entry point (VERDICT r5 "next round" 4): the caller holds one bit per voxel, the
        # dense tier reads it in place, no pack kernel runs.  Reported beside `value`, never instead of it (BASELINE.json's
        # workload is a uint8 occupancy grid).
        if nz % 32 == 0:
            try:
                bits = [torch.empty(n_total // 32, dtype=torch.int32, device=dev) for _ in range(n_masks)]
                for m_, b_ in zip(masks, bits):
                    ctx.pack_bits_device(m_.data_ptr(), nx * ny, nz, b_.data_ptr(), stream.cuda_stream)
                out_b = torch.empty(shape, dtype=torch.float32, device=dev)

                def step_bits(i):
                    ctx.build_bits_device(bits[i % n_masks].data_ptr(), shape, out_b.data_ptr(), res, False, stream.cuda_stream)

                for i in range(max(args.warmup, 3)):
                    step_bits(i)
                    torch.cuda.synchronize(dev)
                same = bool(torch.equal(out_b.view(torch.int32), out.view(torch.int32))) if (max(args.warmup, 3) - 1) % n_masks == (args.steps - 1) % n_masks else None
                tb = sorted(timed_loop(step_bits, args.steps, fence) for _ in range(3))
                result["bits_entry"] = {"call": "sdfgpu_build_bits_device: 1 bit per voxel in (device), fp32 SDF + extrema out",
                                        "ms_per_step": round(tb[1] / args.steps * 1e3, 4),
                                        "Mvoxels_per_s": round(n_total / (tb[1] / args.steps) / 1e6, 2),
                                        "Mvoxels_per_s_min_max": [round(n_total / (tb[2] / args.steps) / 1e6, 2), round(n_total / (tb[0] / args.steps) / 1e6, 2)],
                                        "compulsory_bytes_per_voxel": 4.125,
                                        "frac_of_hbm_peak": round(n_total * 4.125 / (tb[1] / args.steps) / 1e9 / HBM_PEAK_GBPS, 4),
                                        "bit_identical_to_the_mask_build": same, "kernels": ctx.last_build_info()}
                del bits, out_b
            except Exception as e:
                result["bits_entry"] = {"error": repr(e)}
        if builds:
            info, avg, stage_ms = stage_table(ctx, ms_sum, builds, n_total)
            result["config"]["kernels"] = info
            if info["dense_certified"]:
                result["config"]["guarded_general_pipeline_ms"] = round(sum(avg[2:]), 4)
            dom = max(stage_ms, key=stage_ms.get)
            r = roofline_of(dom, stage_ms[dom], n_total, info["plane16"], load_traffic(), info)
            r["stages_ms"] = {k: round(v, 4) for k, v in stage_ms.items()}
            rp = load_rocprof_times()
            ent = (rp or {}).get(TRAFFIC_KEY.get(dom) if r.get("kernel") == KERNEL_NAMES[dom] else None)
            if ent:                                                 # rocprofv3 --kernel-trace --stats of the same command (profiles/)
                r["rocprof_avg_ms"] = ent["avg_ms"] if isinstance(ent, dict) else ent
            r["note"] = ("frac = compulsory bytes of this kernel (bytes_per_voxel x voxels) / HIP-event duration / peak; "
                         "traffic = HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/traffic.json)")
            result["roofline"] = r
    else:
        launches, ms_total, vox = builder.pop_ball_timings()
        if launches and rank == 0 and args.full:
            avg_ms = ms_total / launches
            traffic = load_traffic()
            per_voxel = ((traffic or {}).get("dense_ball") or 0) / float(512 ** 3)
            r = roofline_of("dense_ball", avg_ms, vox, True, None)
            r["traffic"] = int(per_voxel * vox) if per_voxel else None
            if per_voxel:
                r["traffic_frac"] = round(per_voxel * vox / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
            r["launches_timed"] = launches
            r["voxels_per_launch"] = vox
            r["note"] = "rank 0, interior planes of its slab, every 4th build; traffic scaled from the 512^3 PMC pass"
            result["roofline"] = r
        result["config"]["dense_path"] = builder.dense
        result["config"]["builds_needing_general_path"] = builder.general_builds
        result["config"]["whole_line_fallbacks"] = builder.fallbacks
        result["config"]["general_exchange"] = getattr(builder, "general_exchange", None)

    if args.force_slab and world == 1 and args.full:
        # VERDICT r3 "next round" 5: what the HOST costs a multi-rank build.  libsdfgpu_multi with 1 / 2 / 8 logical ranks on
        # this one GPU (the messages travel as device-to-device copies) against the single-GPU ABI on the same scenes:
        # wall time per synchronous build, its host round trips, and the difference to the single-GPU build = host calls +
        # exchange + (for 2 and 8 ranks) the lost overlap of slabs that share one GPU.
        try:
            import numpy as np
            one = capi.SdfGpu(local_rank)
            dense_m = synth.bernoulli_mask_torch(shape, 0.5, 1, device=dev)
            pts = torch.from_numpy(synth.two_box_points(200000, seed=0, scale=nx * res)).to(dev)
            far_m = torch.zeros(shape, dtype=torch.uint8, device=dev)
            one.voxelize_points_device(pts.data_ptr(), pts.shape[0], (0.0, 0.0, 0.0), res, shape, far_m.data_ptr(), True, stream.cuda_stream)
            o1 = torch.empty(shape, dtype=torch.float32, device=dev)

            def wall(fn, reps=10):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize(dev)
                return (time.perf_counter() - t0) / reps * 1e3

            def single(mk):
                one.build_device(mk.data_ptr(), shape, o1.data_ptr(), res, False, stream.cuda_stream)
                one.get_extrema()                                       # (synchronous like the multi-rank call)

            ref = {"dense": wall(lambda: single(dense_m)), "far": wall(lambda: single(far_m))}
            block = {"single_gpu_abi_ms": {k: round(v, 4) for k, v in ref.items()}, "logical_ranks": {}}
            block["note"] = ("logical ranks share ONE GPU here: their kernels serialise and their rank threads contend for one "
                             "device's queues, so ms_per_build grows with the rank count by construction; host_us_slowest_rank_thread "
                             "is the figure that carries over to one GPU per rank")
            for ranks in (1, 2, 8):
                mg = capi.MultiSdfGpu(ranks, [local_rank] * ranks)
                outs = []
                row = {}
                for name, mk in (("dense", dense_m), ("far", far_m)):
                    slabs = [mk[a:b] for a, b in (mg.slab_range(nx, r) for r in range(ranks))]
                    outs = [torch.empty(tuple(t.shape), dtype=torch.float32, device=dev) for t in slabs]
                    ms = wall(lambda: mg.build_device([t.data_ptr() for t in slabs], shape, [t.data_ptr() for t in outs], res, False))
                    st = mg.last_stats()
                    row[name] = {"ms_per_build": round(ms, 4), "host_reads": st["host_reads"],
                                 "over_single_gpu_us": round((ms - ref[name]) * 1e3, 1), "path": mg.last_path(),
                                 # host time inside API calls of the last build: the slowest rank thread (what bounds a build
                                 # when every rank has its own GPU) and the sum over the rank threads (what ONE issuing thread,
                                 # rounds 2 - 4, would have spent); waiting for the device excluded
                                 "host_us_slowest_rank_thread": round(st["host_us_max_rank"], 1),
                                 "host_us_sum_over_rank_threads": round(st["host_us_sum"], 1)}
                row["mispredictions"] = mg.last_stats()["mispredictions"]
                block["logical_ranks"][str(ranks)] = row
                mg.close()
                del outs
            one.close()
            result["multi_native_on_one_gpu"] = block
        except Exception as e:
            result["multi_native_on_one_gpu"] = {"error": repr(e)}

    single = rank == 0 and world == 1 and not args.force_slab
    if single and args.full and not args.no_legs:
        legs = {}
        leg_steps = max(10, min(50, args.steps))
        try:
            legs["general_tier_headline_input"] = run_leg(
                torch, capi, dev, shape, res, masks, {"dense": 0}, leg_steps, 5,
                "the headline grids through the separable-sweep tier only (option dense=0)")
            sparse = [synth.bernoulli_mask_torch(shape, 0.01, 11 + k, device=dev) for k in range(2)]
            legs["sparse_bernoulli_p0.01"] = run_leg(
                torch, capi, dev, shape, res, sparse, {}, leg_steps, 20,
                "%dx%dx%d Bernoulli(p=0.01), 2 grids in rotation, default policy" % shape)
            del sparse
            mid = [synth.bernoulli_mask_torch(shape, 0.03, 21 + k, device=dev) for k in range(2)]
            legs["mid_bernoulli_p0.03"] = run_leg(
                torch, capi, dev, shape, res, mid, {}, leg_steps, 20,
                "%dx%dx%d Bernoulli(p=0.03), 2 grids in rotation, default policy (the dense tier's wide form KD3 + fix-up kernel)" % shape)
            del mid
            # a structured scene of the kind CollisionMapGrid callers hold (solid obstacles in free space: floor, walls, a table,
            # a shelf): far-field pair, thin and thick solids
            room = [synth.room_mask_torch(shape, dev)]
            legs["structured_room"] = run_leg(
                torch, capi, dev, shape, res, room, {}, leg_steps, 10,
                "%dx%dx%d room scene (floor + two walls 2 %% of the grid thick, table on legs, shelf; 6.9 %% filled), default policy" % shape)
            del room
            # ... and obstacles in OPEN space (the reference's tutorial boxes, src/sdf_tools_tutorial.cpp:45-59, scaled to the grid): most
            # x-planes and z rows hold no filled voxel, which the far-field pair skips (round 6, option plane_skip)
            boxes = [synth.tutorial_boxes_mask_torch(shape, dev, True)]
            legs["structured_boxes"] = run_leg(
                torch, capi, dev, shape, res, boxes, {}, leg_steps, 10,
                "%dx%dx%d solid boxes in open space (the tutorial scene scaled to the grid), default policy" % shape)
            del boxes
            if shape == (512, 512, 512):
                legs["streaming_two_box"] = streaming_leg(torch, dev, 512, 0.01, 30)
            # BASELINE.json configs[1] / BASELINE.md section 3: 256^3, fp32 distances, single MI355X -- "throughput reported"
            # (parity <= 1e-5 is tests/test_gpu_parity.py's 256^3 case).  16.8 Mvoxel per build: launch-bound, not HBM-bound.
            s256 = (256, 256, 256)
            m256 = [synth.bernoulli_mask_torch(s256, 0.5, 31 + k, device=dev) for k in range(3)]
            legs["config_256_cube"] = run_leg(torch, capi, dev, s256, res, m256, {}, max(leg_steps, 50), 10,
                                              "256x256x256 Bernoulli(p=0.5), 3 grids in rotation, default policy (BASELINE configs[1])")
            del m256
            # BASELINE configs[3]'s WORKLOAD (1024^3) on this one GPU -- the N = 1 point of that grid's scaling table (the
            # 8-GPU x-slab run of it is `bench.py --gpus 8`); 1 GiB of mask in, 4 GiB of fp32 out, everything resident
            try:
                free_b, _ = torch.cuda.mem_get_info(dev)
                if free_b > 24 * (1 << 30):
                    s1k = (1024, 1024, 1024)
                    m1k = [synth.bernoulli_mask_torch(s1k, 0.5, 41, device=dev)]
                    legs["config_1024_cube_single_gpu"] = run_leg(torch, capi, dev, s1k, res, m1k, {}, 10, 3,
                                                                  "1024x1024x1024 Bernoulli(p=0.5), one grid, default policy, ONE GPU "
                                                                  "(BASELINE configs[3]'s workload; its 8-GPU partition is --gpus 8)")
                    del m1k
                    torch.cuda.empty_cache()
                    # ... and the room at that size: the far-field pair on 1024-voxel lines (round 6: its y sweep no longer searches
                    # the open volume above the floor -- two-valued tiles)
                    r1k = [synth.room_mask_torch(s1k, dev)]
                    legs["structured_room_1024"] = run_leg(torch, capi, dev, s1k, res, r1k, {}, 10, 8,
                                                           "1024x1024x1024 room scene (as structured_room), default policy, ONE GPU")
                    del r1k
                    torch.cuda.empty_cache()
            except Exception as e:
                legs["config_1024_cube_single_gpu"] = {"error": repr(e)}
        except Exception as e:                     # a leg must never take the contract line down with it
            legs["error"] = repr(e)
        result["legs"] = legs
        try:
            result["parity"] = parity_counts(ctx, res)
        except Exception as e:
            result["parity"] = {"error": repr(e)}
    if single and args.full and not args.no_cpu_baseline:
        # what a caller of the reference's C++ API sees: host mask -> host SDF through sdfgpu_build (PCIe both ways,
        # fresh output buffer).  Reported for context only -- never `value`.
        host_mask = masks[0].cpu().numpy()
        ctx.build(host_mask, res)
        t_host, keep = [], []
        for _ in range(2):
            t1 = time.perf_counter()
            keep.append(ctx.build(host_mask, res))          # (kept alive: freeing a 512 MiB result is ~20 ms of munmap
            t_host.append(time.perf_counter() - t1)         #  that belongs to the caller, not to the call)
        del keep
        result["host_api"] = {"call": "sdfgpu_build (host -> host, PCIe inclusive)", "ms": round(min(t_host) * 1e3, 2),
                              "Mvoxels_per_s": round(n_total / min(t_host) / 1e6, 1),
                              "note": "includes numpy output allocation; not the benchmark metric"}
        # ... and what a C++ caller of the device-resident seam sees (DeviceSignedDistanceField: host mask in, field stays
        # in HBM, 1 M EstimateDistance + gradient queries answered from there, no 512 MiB download)
        try:
            import numpy as np
            d_field = ctx.device_malloc(n_total * 4)
            qp = np.random.default_rng(0).random((1 << 20, 3)) * (np.asarray(shape, np.float64) * res)
            ctx.build_to_device(host_mask, d_field, res)
            ctx.query_points(d_field, shape, res, qp, enable_edge_gradients=True)
            t_b, t_q = [], []
            for _ in range(3):
                t1 = time.perf_counter()
                ctx.build_to_device(host_mask, d_field, res)
                t2 = time.perf_counter()
                ctx.query_points(d_field, shape, res, qp, enable_edge_gradients=True)
                t_b.append(t2 - t1)
                t_q.append(time.perf_counter() - t2)
            ctx.device_free(d_field)
            result["host_api"]["device_resident"] = {
                "call": "sdfgpu_build_to_device (host mask -> field in HBM) + sdfgpu_query_points (1 M host points -> host answers)",
                "build_ms": round(min(t_b) * 1e3, 2), "query_1M_ms": round(min(t_q) * 1e3, 2),
                "note": "the mask upload (128 MiB) is the PCIe cost left; the query moves 24 MB up and 33 MB down"}
        except Exception as e:
            result["host_api"]["device_resident"] = {"error": repr(e)}
        del host_mask
        # ... and the reference-shaped call itself (VERDICT r4 "next round" 3): CollisionMapGrid::ExtractSignedDistanceField
        # (collision_map.hpp:680-712) on a host map of 8-byte COLLISION_CELL records -> host SignedDistanceField, end to end,
        # from a C++ client (examples/class_seam.cpp, which also checks the field bit for bit against sdfgpu_build) and
        # through the pybind method the reference's Python callers use (bindings.cpp:81)
        try:
            result["host_api"]["class_seam"] = class_seam_block(shape, res)
        except Exception as e:
            result["host_api"]["class_seam"] = {"error": repr(e)}
        result["cpu_baseline"] = cpu_baseline(args.cpu_sample, args.p, res)
    if rank == 0 and args.full:
        emit(result)
    elif rank == 0:
        print(json.dumps(summary_line(result)), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
