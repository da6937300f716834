#!/usr/bin/env python3
"""The dense-certified step (n^3 Bernoulli p = 0.5, three masks in rotation, one output buffer, device-resident) with the stand-by
behind the dense tier as ONE guarded launch (option standby_single = 1, the default) and as two (standby_single = 0), and
(other=<path>) on another build of the library, e.g. the parent commit's.  All configurations run in ONE process, alternated
repetition by repetition, on the same masks and the same output tensor.  One JSON line per configuration.

  python tools/standby_single_ab.py [other=<libsdfgpu.so>] [reps=5] [steps=200] [n=256]

transition=1 instead times the build in which the scene leaves the dense tier (the two-box cloud behind a trusted dense tier: the
stand-by does the work) next to the steady far-field build, `reps` times per configuration.
"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: the libraries then bind to torch's HIP runtime)

from sdf_tools_amd import synth  # noqa: E402

kv = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
other = kv.get("other")
reps, steps, n = int(kv.get("reps", 5)), int(kv.get("steps", 200)), int(kv.get("n", 256))
transition = int(kv.get("transition", 0)) != 0
vp, i64, dbl, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int


def bind(path, opts):
    L = ctypes.CDLL(os.path.abspath(path))
    L.sdfgpu_create.argtypes = [ci, ctypes.POINTER(vp)]
    L.sdfgpu_set_option.argtypes = [vp, ctypes.c_char_p, ci]
    L.sdfgpu_build_device.argtypes = [vp, vp, i64, i64, i64, dbl, ci, vp, vp]
    L.sdfgpu_last_dense_certified.argtypes = [vp, ctypes.POINTER(ci)]
    h = vp()
    assert L.sdfgpu_create(0, ctypes.byref(h)) == 0
    for k, v in opts.items():
        assert L.sdfgpu_set_option(h, k.encode(), v) == 0, (path, k)
    return L, h


dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
shape = (n, n, n)
masks = [synth.bernoulli_mask_torch(shape, 0.5, 1 + k, device=dev) for k in range(3)]
out = torch.empty(shape, dtype=torch.float32, device=dev)
stream = torch.cuda.current_stream(dev).cuda_stream
tree = os.path.join(ROOT, "sdf_tools_amd", "libsdfgpu.so")
configs = [{"lib": "in-tree", "standby_single": 1, "ctx": bind(tree, {"standby_single": 1})},
           {"lib": "in-tree", "standby_single": 0, "ctx": bind(tree, {"standby_single": 0})}]
if other:
    configs.append({"lib": "other", "standby_single": None, "ctx": bind(other, {})})


def build(c, mask):
    L, h = c["ctx"]
    assert L.sdfgpu_build_device(h, mask.data_ptr(), n, n, n, 0.01, 0, out.data_ptr(), stream) == 0


def path(c):
    L, h = c["ctx"]
    v = ci()
    assert L.sdfgpu_last_dense_certified(h, ctypes.byref(v)) == 0
    return v.value & 7


def timed(c, mask):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    build(c, mask)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1)


if transition:
    far = (torch.from_numpy(synth.two_box_points(200000, seed=0, scale=n * 0.01)).to(dev) / 0.01).long().clamp_(0, n - 1)
    far_mask = torch.zeros(shape, dtype=torch.uint8, device=dev)
    far_mask[far[:, 0], far[:, 1], far[:, 2]] = 1
    for c in configs:
        c["transition_ms"], c["far_ms"], c["paths"] = [], [], []
    for _ in range(reps):
        for c in configs:
            for _ in range(8):                              # synchronised: the policy sees every report and trusts the dense tier
                timed(c, masks[0])
            assert path(c) == 1, path(c)
            c["transition_ms"].append(round(timed(c, far_mask), 4))
            c["paths"].append(path(c))
            for _ in range(4):
                timed(c, far_mask)
            c["far_ms"].append(round(min(timed(c, far_mask) for _ in range(5)), 4))
    for c in configs:
        print(json.dumps({k: v for k, v in c.items() if k != "ctx"} | {"n": n}), flush=True)
    sys.exit(0)

for c in configs:
    c["ms"] = []
    for i in range(10):                                     # the handles' policies see a few synchronised builds first, as in bench.py
        build(c, masks[i % 3])
        torch.cuda.synchronize(dev)
for _ in range(reps):
    for c in configs:
        for i in range(6):
            build(c, masks[i % 3])
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(steps):
            build(c, masks[i % 3])
        torch.cuda.synchronize(dev)
        c["ms"].append((time.perf_counter() - t0) / steps * 1e3)
for c in configs:
    ms = sorted(c["ms"])
    print(json.dumps({"lib": c["lib"], "standby_single": c["standby_single"], "n": n, "steps": steps,
                      "ms_per_step_run_order": [round(v, 4) for v in c["ms"]], "median_ms": round(ms[len(ms) // 2], 4),
                      "spread_ms": round(ms[-1] - ms[0], 4), "median_Gvoxel_per_s": round(n ** 3 / ms[len(ms) // 2] / 1e6, 1)}), flush=True)
