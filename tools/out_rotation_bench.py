#!/usr/bin/env python3
"""The headline step (512^3 Bernoulli p = 0.5, three masks in rotation, device-resident) when the caller rebuilds into ONE
output buffer -- what bench.py times -- and when it rotates over THREE.  The serpentine tile order of the dense ball kernel
only helps the first kind of caller (each build starts on the lines the previous one left in the Infinity Cache), so the
two figures belong side by side, and the three-buffer figure is the one to hold against HBM.

All configurations run in ONE process, alternated repetition by repetition, on the same masks and the same three output
tensors: in-tree library with 1 / 3 buffers, the same with ball_serpentine = 0, and (other=<path>) another build of the
library, e.g. the parent commit's.  One JSON line per configuration.

  python tools/out_rotation_bench.py [other=<libsdfgpu.so>] [reps=5] [steps=200] [n=512]
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
reps, steps, n = int(kv.get("reps", 5)), int(kv.get("steps", 200)), int(kv.get("n", 512))
vp, i64, dbl, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int


def bind(path, opts):
    L = ctypes.CDLL(os.path.abspath(path))
    L.sdfgpu_create.argtypes = [ci, ctypes.POINTER(vp)]
    L.sdfgpu_set_option.argtypes = [vp, ctypes.c_char_p, ci]
    L.sdfgpu_build_device.argtypes = [vp, vp, i64, i64, i64, dbl, ci, vp, vp]
    h = vp()
    assert L.sdfgpu_create(0, ctypes.byref(h)) == 0
    for k, v in opts.items():
        assert L.sdfgpu_set_option(h, k.encode(), v) == 0, (path, k)
    return L, h


dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
shape = (n, n, n)
masks = [synth.bernoulli_mask_torch(shape, 0.5, 1 + k, device=dev) for k in range(3)]
outs = [torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(3)]
stream = torch.cuda.current_stream(dev).cuda_stream
tree = os.path.join(ROOT, "sdf_tools_amd", "libsdfgpu.so")
configs = []
for name, path, opts in (("in-tree", tree, {}), ("in-tree ball_serpentine=0", tree, {"ball_serpentine": 0})) + (
        (("other", other, {}),) if other else ()):
    for n_out in (1, 3):
        configs.append({"lib": name, "output_buffers": n_out, "ctx": bind(path, opts), "ms": []})


def run(c, k):
    L, h = c["ctx"]
    for i in range(k):
        assert L.sdfgpu_build_device(h, masks[i % 3].data_ptr(), n, n, n, 0.01, 0, outs[i % c["output_buffers"]].data_ptr(), stream) == 0


for c in configs:                               # the handles' policies see a few synchronised builds first, as in bench.py
    for _ in range(10):
        run(c, 1)
        torch.cuda.synchronize(dev)
for _ in range(reps):
    for c in configs:
        run(c, 6)                               # this configuration's own steady state (cache contents, direction)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        run(c, steps)
        torch.cuda.synchronize(dev)
        c["ms"].append((time.perf_counter() - t0) / steps * 1e3)
for c in configs:
    ms = sorted(c["ms"])
    print(json.dumps({"lib": c["lib"], "output_buffers": c["output_buffers"], "steps": steps,
                      "ms_per_step_sorted": [round(v, 4) for v in ms], "median_ms": round(ms[len(ms) // 2], 4),
                      "median_Gvoxel_per_s": round(n ** 3 / ms[len(ms) // 2] / 1e6, 1)}), flush=True)
