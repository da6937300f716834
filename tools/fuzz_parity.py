#!/usr/bin/env python3
"""Differential fuzzing on a GPU box: random shapes / densities / borders / scene types through the C ABI,
every voxel compared bit for bit with the oracle's exact EDT (oracle/ is the checker here, as in tests/).

  python tools/fuzz_parity.py [seconds] [seed]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from oracle import oracle as O  # noqa: E402
from sdf_tools_amd import capi, synth  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import analysis_scenes as AS  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rng = np.random.default_rng(seed)
# where the guard and bits modes put their buffers relative to a 16-byte boundary: a generator of its own, so that the scenes and
# options of a seed stay the ones they were before the shifts were drawn
shift_rng = np.random.default_rng([seed, 0xA119])
ctx = capi.SdfGpu(0)
VERBOSE = bool(os.environ.get("FUZZ_VERBOSE"))           # print every scene's shape and options before its build (to find a crash)
if VERBOSE:
    _set = ctx.set_option
    _opts = {}

    def _recording_set(name, value):
        _opts[name] = value
        return _set(name, value)
    ctx.set_option = _recording_set
MULTI = {}
MODES = {}
sizes = [1, 2, 3, 5, 8, 13, 16, 21, 32, 33, 40, 64, 96, 128]
t0 = time.time()
n = 0
while time.time() - t0 < budget:
    shape = tuple(int(rng.choice(sizes)) for _ in range(3))
    if rng.random() < 0.5:
        shape = shape[:2] + (int(rng.choice([32, 64, 128, 256])),)        # dense-path eligible z extents
    if rng.random() < 0.08:                                              # wide rows: other tile shapes / expansion paths
        shape = (int(rng.choice([1, 2, 5, 9, 17])), int(rng.choice([1, 3, 8, 20])), int(rng.choice([512, 1024, 2048])))
    if rng.random() < 0.08:                                              # long x / y lines: the far-field kernel's levels with one interval
        a, b = int(rng.choice([300, 512, 520, 777, 1024])), int(rng.choice([1, 2, 5, 9]))     # per lane (> 512) / two lanes per interval, wave-cooperative scans
        shape = ((a, b) if rng.random() < 0.5 else (b, a)) + (int(rng.choice([16, 32, 64])),)
    floor_scene = rng.random() < 0.12                                    # round 6: floors (see kind 5)
    if floor_scene:
        shape = (int(rng.choice([8, 9, 16, 33, 64])), int(rng.choice([8, 21, 64, 100, 130, 256, 512, 515, 777, 1024])), int(rng.choice([64, 64, 128])))
    if np.prod(shape) > 1 << 21:
        continue
    kind = 5 if floor_scene else rng.integers(0, 5)
    if kind == 4:
        # round 5: axis-aligned slabs (floors / walls, whole extent in two axes), solid boxes and box shells, optionally a few noise
        # voxels -- the far-field kernel's flat-stretch shortcut (plateaus of the sweep's input with jumps and holes, unit steps
        # next to slabs) on both swept axes, through both passes
        m = np.zeros(shape, np.uint8)
        for _ in range(int(rng.integers(1, 5))):
            if rng.random() < 0.5:
                ax = int(rng.integers(0, 3))
                a = int(rng.integers(0, shape[ax]))
                sl = [slice(None)] * 3
                sl[ax] = slice(a, min(shape[ax], a + int(rng.integers(1, 12))))
                m[tuple(sl)] = 1
            else:
                lo = [int(rng.integers(0, s)) for s in shape]
                hi = [min(s, l + int(rng.integers(1, max(2, s // 2 + 1)))) for l, s in zip(lo, shape)]
                m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
                if rng.random() < 0.4 and all(h - l > 2 for l, h in zip(lo, hi)):
                    m[lo[0] + 1:hi[0] - 1, lo[1] + 1:hi[1] - 1, lo[2] + 1:hi[2] - 1] = 0
        if rng.random() < 0.3:
            m |= (rng.random(shape) < 0.002).astype(np.uint8)
        if rng.random() < 0.2:
            m = 1 - m
    elif kind == 5:
        # round 6: a floor (every z row holds a filled voxel: the far-field pair's row flags say "floor-like") under walls, plates,
        # steps and pillars -- y lines with one, two and more values outside their zero sites, zero sites at chunk edges -- and now
        # and then noise or a hole in the floor: the two-valued tiles of the far-field y sweep, with their habit open, closed and forced
        m = np.zeros(shape, np.uint8)
        m[:, :, :int(rng.integers(1, 4))] = 1
        for _ in range(int(rng.integers(0, 5))):
            what = int(rng.integers(0, 4))
            x0, x1 = sorted(int(v) for v in rng.integers(0, shape[0] + 1, 2))
            y0, y1 = sorted(int(v) for v in rng.integers(0, shape[1] + 1, 2))
            z0 = int(rng.integers(0, shape[2]))
            if what == 0:
                m[:, y0:y0 + int(rng.integers(1, 12)), :] = 1                     # a wall across y lines
            elif what == 1:
                m[x0:x1 + 1, y0:y1 + 1, z0:z0 + int(rng.integers(1, 4))] = 1     # a plate
            elif what == 2:
                m[x0:x1 + 1, y0:y1 + 1, :z0] = 1                                  # a step
            else:
                m[x0:x1 + 1:3, int(rng.choice([0, 7, 8, 9, 63, 64, y0])) % shape[1], :] = 1     # pillars
        if rng.random() < 0.25:
            m |= (rng.random(shape) < 0.001).astype(np.uint8)
        if rng.random() < 0.1:
            m[int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1])), :] = 0
    elif kind == 0:
        m = synth.bernoulli_mask(shape, float(rng.choice([0.5, 0.3, 0.1, 0.05, 0.03, 0.02, 0.01, 0.001, 0.9, 0.96, 0.99, 0.999])), int(rng.integers(1 << 30)))
    elif kind == 1:
        m = synth.spheres_mask(shape, int(rng.integers(1, 5)), (1, 9), int(rng.integers(1 << 30)))
    elif kind == 2:
        m = np.zeros(shape, np.uint8)
        for _ in range(int(rng.integers(0, 4))):
            m[tuple(int(rng.integers(0, s)) for s in shape)] = 1
        if rng.random() < 0.3:
            m = 1 - m
    else:
        m = (rng.random(shape) < rng.random() ** 3).astype(np.uint8)
        lo = [int(rng.integers(0, s)) for s in shape]
        hi = [int(rng.integers(l, s)) + 1 for l, s in zip(lo, shape)]
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = rng.integers(0, 2)
    res = float(rng.choice([1.0, 0.5, 0.01, 0.037]))
    vb = bool(rng.integers(0, 2))
    for k, v in (("dense", int(rng.integers(0, 2))), ("envelope", int(rng.integers(0, 2))), ("plane16", int(rng.integers(0, 2)))):
        ctx.set_option(k, v)
    if rng.random() < 0.3:
        ctx.set_option("fixup_mode", 1)                 # force the fix-up kernel behind the dense ball kernel
    if rng.random() < 0.35:
        ctx.set_option("dense3_mode", 1)                # ... the wide ball kernel (KD3) in KD's place
    ctx.set_option("dense3_fixed", int(rng.random() < 0.7))   # round 5: KD3's nz = 512 instance (compile-time row pitch) or the generic one
    ctx.set_option("dense_shell", int(rng.random() < 0.8))     # round 5: the shell pass (KD6) between KD3 and KF, or KF alone
    # tier selection: fresh decisions, forced far-field sweeps, both hand-off forms, low thresholds (far-field kernel on
    # scenes the marching kernels would normally take)
    if rng.random() < 0.5:
        ctx.set_option("policy_reset", 1)
    ctx.set_option("i32_handoff", int(rng.integers(0, 2)))
    ctx.set_option("envelope_mode", 1 if rng.random() < 0.2 else 0)
    ctx.set_option("far_threshold_y", int(rng.choice([1, 4, 64])))
    ctx.set_option("far_threshold_x", int(rng.choice([1, 9, 25])))
    ctx.set_option("probe_window", int(rng.random() < 0.7))      # window statistic / level A on sampled tiles
    ctx.set_option("z_wave", int(rng.random() < 0.8))
    # round 4: the handle "trusts its dense tier" (the general pipeline behind it is then the stand-by pair: far-field y sweep
    # staged from the bit field + far-field x sweep, LOOP form) with small and large stand-by grids, or the old stand-by
    ctx.set_option("dc_fixed", int(rng.random() < 0.7))         # round 5: far-field instances with a compile-time line length (512)
    ctx.set_option("far_predict", int(rng.choice([0, 1, 2, 2])))   # round 5: the far-field pair without probes (learnt / forced)
    ctx.set_option("plane_skip", int(rng.random() < 0.85))      # round 6: row / plane flags of the far-field pair, the two-valued tiles behind them
    ctx.set_option("flat_tiles", int(rng.choice([0, 1, 1, 2, 2])))
    if floor_scene:
        for k, v in (("dense", 0), ("far_predict", 2), ("envelope", 1), ("envelope_mode", 0), ("z_wave", 1)):
            if rng.random() < 0.8:
                ctx.set_option(k, v)
    ctx.set_option("standby_far", int(rng.random() < 0.85))
    ctx.set_option("standby_grid", int(rng.choice([32, 64, 1024])))
    if rng.random() < 0.4:
        ctx.set_option("expect_dense", 1)
    if VERBOSE:
        print("scene", n, shape, "kind", int(kind), "res", res, "vb", vb, "filled", int(m.sum()), _opts, flush=True)
    os.makedirs("gpurun_out", exist_ok=True)
    if VERBOSE:
        np.save("gpurun_out/fuzz_last_mask.npy", m)       # (the scene a crash happened in)
    # which entry point builds this scene (round 6): the host-buffer ABI, the device-resident ABI into a guard-banded field, the
    # bits-in ABI, libsdfgpu_multi with 1 .. 4 logical ranks on this GPU (x slabs: sdfgpu_slab_dense_phase, the tiered z / y sweep,
    # the halo and whole-line x sweeps, the re-partition), and now and then the gradient / query kernels on the result.  With
    # SDFGPU_REDZONE=1 every buffer the library owns -- the ranks' slabs and exchange buffers included -- and every
    # sdfgpu_device_malloc buffer used here carries canaries that each call checks.
    mode = str(rng.choice(["host", "guard", "guard", "bits", "multi", "rz_out"]))
    values_bad = None                                   # rz_out: what the gradient / query value check found
    placed = ""                                         # guard / bits: where the buffers sat (printed with a failure)
    if os.environ.get("FUZZ_GUARD") and mode == "host":
        mode = "guard"
    if mode == "multi" and (shape[0] < 4 or vb and rng.random() < 0.5):
        mode = "guard"
    if mode == "multi":
        ranks = int(rng.choice([r for r in (1, 2, 3, 4) if r <= shape[0]]))
        if ranks not in MULTI:
            MULTI[ranks] = capi.MultiSdfGpu(ranks, [0] * ranks)
        mg = MULTI[ranks]
        mg.set_option("halo", int(rng.choice([1, 2, 3, 8])))
        mg.set_option("dense", int(rng.integers(0, 2)))
        mg.set_option("predict_far", int(rng.integers(0, 2)))
        mg.set_option("dense_retry", 0)
        got, ext = mg.build(m, res, vb)
    elif mode == "rz_out":
        # exact-size output and input from sdfgpu_device_malloc: in red-zone mode the first byte behind the field is canary
        import torch
        nvox = int(m.size)
        d_in, d_out = ctx.device_malloc(nvox), ctx.device_malloc(nvox * 4)
        ctx.copy_from_host(d_in, m)
        ctx.build_device(d_in, shape, d_out, res, vb, 0)
        ext = ctx.get_extrema()
        got = ctx.copy_to_host(np.empty(shape, np.float32), d_out)
        if rng.random() < 0.3:                      # the gradient and query kernels on the fresh field, exact-size outputs
            d_g = ctx.device_malloc(nvox * 12)
            ctx.gradient_device(d_out, shape, d_g, res, True, False, 0)
            npts = 257
            pts = (rng.random((npts, 3)) * (np.asarray(shape) * res * 1.2) - 0.1 * res).astype(np.float64)
            d_p, d_d, d_gr, d_f = ctx.device_malloc(npts * 24), ctx.device_malloc(npts * 8), ctx.device_malloc(npts * 24), ctx.device_malloc(npts)
            ctx.copy_from_host(d_p, pts)
            q_edge = bool(rng.integers(0, 2))
            ctx.query_points_device(d_out, shape, res, d_p, npts, d_d, d_gr, d_f, enable_edge_gradients=q_edge)
            ctx.redzone_check()
            # their values against the numpy restatements (tests/analysis_scenes.py): the field itself is checked below
            g32 = ctx.copy_to_host(np.empty(shape + (3,), np.float32), d_g)
            q_d, q_g, q_f = (ctx.copy_to_host(np.empty(npts, np.float64), d_d), ctx.copy_to_host(np.empty((npts, 3), np.float64), d_gr),
                             ctx.copy_to_host(np.empty(npts, np.uint8), d_f))
            w_d, w_g, w_f = AS.query_points(got, res, pts, np.inf, q_edge)
            w32 = AS.grid_gradient(got, res, True).astype(np.float32)
            same_g = np.all((g32.view(np.uint32) == w32.view(np.uint32)) | (np.isnan(g32) & np.isnan(w32)))
            same_q = np.array_equal(q_f, w_f) and np.all((q_g.view(np.uint64) == w_g.view(np.uint64)) | (np.isnan(q_g) & np.isnan(w_g)))
            # (k_query_points does not fuse products with sums: the distance is bit-equal under the identity transform)
            near = (q_d.view(np.uint64) == w_d.view(np.uint64)) | (np.isnan(q_d) & np.isnan(w_d))
            if not (same_g and same_q and near.all()):      # (reported with the field's own check below, which saves the scene)
                values_bad = "gradient / query values differ: gradient %s query %s distance %d" % (bool(same_g), bool(same_q),
                                                                                                   int((~near).sum()))
            for ptr in (d_g, d_p, d_d, d_gr, d_f):
                ctx.device_free(ptr)
        ctx.device_free(d_in)
        ctx.device_free(d_out)
    elif mode == "bits":
        import torch
        nvox = int(m.size)
        g = ((max(4096, 8 * shape[1] * shape[2]) + 3) // 4) * 4
        # the field 0, 4, 8 or 12 bytes past a 16-byte boundary (every second scene: at one), the bit field 0 .. 3 words past one
        o = int(shift_rng.choice([0, 1, 2, 3])) if shift_rng.random() < 0.5 else 0
        buf = torch.full((g + nvox + g + 3,), -12345.0, dtype=torch.float32, device="cuda")
        words = capi.pack_bits_host(m).view(np.int32)
        db = torch.zeros(words.size + 3, dtype=torch.int32, device="cuda")
        sh = int(rng.integers(0, 2))               # (a field that is only 4-byte aligned takes the device copy)
        sh += 2 * int(shift_rng.integers(0, 2))
        placed = "bits +%d B, field +%d B" % (4 * sh, 4 * o)
        db[sh:sh + words.size] = torch.from_numpy(words).cuda()
        ctx.build_bits_device(db.data_ptr() + 4 * sh, shape, buf.data_ptr() + 4 * (g + o), res, vb, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ext = ctx.get_extrema()
        got = buf[g + o:g + o + nvox].cpu().numpy().reshape(shape)
        if not bool((buf[:g + o] == -12345.0).all().item()) or not bool((buf[g + o + nvox:] == -12345.0).all().item()):
            print("GUARD BAND WRITTEN (bits in) shape", shape, "kind", kind, "res", res, "vb", vb, placed)
            np.save("gpurun_out/fuzz_fail_mask.npy", m)
            sys.exit(1)
    elif mode == "guard":
        # device-resident build into a field with a guard band in front of it and behind it (round 5: a store past the end of the
        # field is silent on the host path, whose staging buffer is as large as the largest scene so far)
        import torch
        nvox = int(m.size)
        g = ((max(4096, 8 * shape[1] * shape[2]) + 3) // 4) * 4
        # every second scene: the mask 0 .. 15 bytes past a 16-byte boundary; every second: the field 0, 4, 8 or 12 bytes past one
        # (element alignment is all the header asks for; the 16-byte kernels are chosen by the pointers)
        ms = int(shift_rng.integers(0, 16)) if shift_rng.random() < 0.5 else 0
        o = int(shift_rng.choice([0, 1, 2, 3])) if shift_rng.random() < 0.5 else 0
        placed = "mask +%d B, field +%d B" % (ms, 4 * o)
        buf = torch.full((g + nvox + g + 3,), -12345.0, dtype=torch.float32, device="cuda")
        dm = torch.zeros(nvox + 16, dtype=torch.uint8, device="cuda")
        dm[ms:ms + nvox] = torch.from_numpy(m.reshape(-1)).cuda()
        ctx.build_device(dm.data_ptr() + ms, shape, buf.data_ptr() + 4 * (g + o), res, vb, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ext = ctx.get_extrema()
        got = buf[g + o:g + o + nvox].cpu().numpy().reshape(shape)
        if not bool((buf[:g + o] == -12345.0).all().item()) or not bool((buf[g + o + nvox:] == -12345.0).all().item()):
            print("GUARD BAND WRITTEN shape", shape, "kind", kind, "res", res, "vb", vb, placed,
                  "before", int((buf[:g + o] != -12345.0).sum().item()), "behind", int((buf[g + o + nvox:] != -12345.0).sum().item()))
            os.makedirs("gpurun_out", exist_ok=True)
            np.save("gpurun_out/fuzz_fail_mask.npy", m)
            sys.exit(1)
    else:
        got, ext = ctx.build(m, res, vb)
    want, want_ext, _ = O.exact_sdf(m, res, vb)
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)) or tuple(ext) != tuple(float(v) for v in want_ext) or values_bad:
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        os.makedirs("gpurun_out", exist_ok=True)
        np.save("gpurun_out/fuzz_fail_mask.npy", m)
        print("MISMATCH shape", shape, "kind", kind, "res", res, "vb", vb, "bad", len(bad), bad[:3].tolist(), ext, want_ext, values_bad or "", placed)
        sys.exit(1)
    n += 1
    MODES[mode] = MODES.get(mode, 0) + 1
print("fuzz OK: %d scenes in %.0f s (seed %d)%s; entry points %s" % (n, time.time() - t0, seed, ", red zones on" if os.environ.get("SDFGPU_REDZONE") else "", MODES))
