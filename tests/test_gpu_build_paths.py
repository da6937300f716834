"""GPU: which tier a build enqueues, pinned against a recorded fixture.

build_device_impl plans a build on the host (sdfgpu_plan.hpp: tests/test_plan_cpu.py drives the planner on the CPU) and then
enqueues it.  Here a matrix of small builds -- the smallest shapes at which the branches differ, every input form, pointers on and
off 16 bytes, a scene the dense tier certifies and one that is far-field on both axes, the option situations a caller can reach,
with and without the virtual border -- is built on the device; after each build `last_build_info()` and `last_path()` must equal
tests/golden/build_paths.json, and the field and the extrema must equal the exact oracle bit for bit.

The fixture was recorded by `record_fixture` below at the commit BEFORE the planner existed (the test never calls it): any entry
that differs is a build that changed its path.
"""
import json
import os

import numpy as np
import pytest

import scenes
from oracle import oracle as O
from sdf_tools_amd import capi, synth

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_paths.json")
RES = 0.05

# (name, shape, input form, byte offset of the input from 16-byte alignment, of the output)
VARIANTS = [
    ("16x32x64 mask", (16, 32, 64), "mask", 0, 0),          # tuned dense, 16-bit plane field, wave-private z sweep, plane-skip eligible
    ("8x16x512 mask", (8, 16, 512), "mask", 0, 0),          # fused-eligible; KD3's fixed 4 x 4 instance
    ("8x12x30 mask", (8, 12, 30), "mask", 0, 0),            # generic dense, int32 plane field
    ("16x32x64 mask, out+4", (16, 32, 64), "mask", 0, 4),
    ("16x32x64 cells", (16, 32, 64), "cells", 0, 0),
    ("16x32x64 bits", (16, 32, 64), "bits", 0, 0),
    ("16x32x64 bits+4", (16, 32, 64), "bits", 4, 0),
]

DEFAULTS = {"dense": 1, "standby_single": 1, "standby_fold": 1, "standby_far": 1, "fused_zy": 1, "far_predict": 1, "plane_skip": 1,
            "envelope_mode": 0, "envelope": 1}
# the option situations a caller can reach; "expect_dense" is set after the policy reset (the reset clears it)
SITUATIONS = [
    ("defaults", {}),
    ("expect_dense", {"expect_dense": 1}),
    ("expect_dense standby_single=0", {"expect_dense": 1, "standby_single": 0}),
    ("expect_dense standby_fold=0", {"expect_dense": 1, "standby_fold": 0}),
    ("expect_dense standby_far=0", {"expect_dense": 1, "standby_far": 0}),
    ("expect_dense fused_zy=2", {"expect_dense": 1, "fused_zy": 2}),
    ("dense=0", {"dense": 0}),
    ("dense=0 far_predict=2", {"dense": 0, "far_predict": 2}),
    ("dense=0 far_predict=2 plane_skip=0", {"dense": 0, "far_predict": 2, "plane_skip": 0}),
    ("dense=0 envelope_mode=1", {"dense": 0, "envelope_mode": 1}),
    ("dense=0 envelope=0", {"dense": 0, "envelope": 0}),
]


def _scenes(shape):
    return {"bernoulli 0.5": synth.bernoulli_mask(shape, 0.5, 1), "single voxel": scenes.single_voxel(shape)}


def _at_offset(nbytes, off):
    """a device byte buffer of nbytes that starts `off` bytes past a 16-byte boundary"""
    import torch
    store = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
    assert store.data_ptr() % 16 == 0
    return store[off:off + nbytes]


def _upload(m, form, off):
    import torch
    if form == "cells":
        a = np.zeros(m.shape + (2,), np.float32)
        a[..., 0] = m
    elif form == "bits":
        a = capi.pack_bits_host(m)
    else:
        a = m
    host = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = _at_offset(host.size, off)
    buf.copy_(torch.from_numpy(host.copy()))
    return buf


def run_matrix(gpu):
    """Every build of the matrix: yields (key, last_build_info, last_path, field, extrema, want field, want extrema)."""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    want = {}
    try:
        for vname, shape, form, in_off, out_off in VARIANTS:
            n = int(np.prod(shape))
            for sname, m in _scenes(shape).items():
                d_in = _upload(m, form, in_off)
                d_out = _at_offset(n * 4, out_off)
                for vb in (False, True):
                    if (shape, sname, vb) not in want:
                        want[(shape, sname, vb)] = O.exact_sdf(m, RES, vb)[:2]
                    for tname, opts in SITUATIONS:
                        gpu.set_option("policy_reset", 1)
                        for k, v in opts.items():
                            gpu.set_option(k, v)
                        d_out.fill_(0xA5)
                        if form == "cells":
                            gpu.build_cells_device(d_in.data_ptr(), shape, d_out.data_ptr(), 8, 0, False, RES, vb, stream)
                        elif form == "bits":
                            gpu.build_bits_device(d_in.data_ptr(), shape, d_out.data_ptr(), RES, vb, stream)
                        else:
                            gpu.build_device(d_in.data_ptr(), shape, d_out.data_ptr(), RES, vb, stream)
                        torch.cuda.synchronize()
                        info, path, ext = gpu.last_build_info(), gpu.last_path(), gpu.get_extrema()
                        field = d_out.cpu().numpy().view(np.float32).reshape(shape)
                        for k in opts:
                            if k in DEFAULTS:
                                gpu.set_option(k, DEFAULTS[k])
                        yield ("%s | %s | %s | vb=%d" % (vname, sname, tname, vb), info, path, field, ext) + want[(shape, sname, vb)]
    finally:
        for k, v in DEFAULTS.items():
            gpu.set_option(k, v)
        gpu.set_option("policy_reset", 1)


def record_fixture(gpu, path=FIXTURE):
    """Writes the fixture from the library as it is built now.  Not called by the test: run once, by hand, at the commit the
    test is to pin."""
    rec = {key: {"info": info, "path": p} for key, info, p, *_ in run_matrix(gpu)}
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    return rec


def test_every_build_takes_its_recorded_path_and_is_exact(gpu):
    with open(FIXTURE) as f:
        recorded = json.load(f)
    seen, wrong_path, wrong_value = set(), [], []
    for key, info, path, field, ext, want, want_ext in run_matrix(gpu):
        seen.add(key)
        got = {"info": info, "path": path}
        if recorded.get(key) != got:
            wrong_path.append((key, got, recorded.get(key)))
        bad = np.argwhere(field.view(np.uint32) != want.view(np.uint32))
        if len(bad) or ext != want_ext:
            wrong_value.append((key, len(bad), bad[:1].tolist(), ext, want_ext, path))
    assert seen == set(recorded), (sorted(seen - set(recorded))[:3], sorted(set(recorded) - seen)[:3])
    assert len(seen) == len(VARIANTS) * 2 * 2 * len(SITUATIONS)
    assert not wrong_value, "%d builds differ from the exact oracle, the first: %r" % (len(wrong_value), wrong_value[0])
    assert not wrong_path, "%d builds left their recorded path, the first (key, got, recorded): %r" % (len(wrong_path), wrong_path[0])
