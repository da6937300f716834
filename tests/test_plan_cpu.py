"""CPU: sdf_tools_amd/csrc/sdfgpu_plan.hpp compiled host-only (tests/plan_harness.cpp) -- what a build enqueues, for the named
situations of the build path and, as invariants, over every combination of the options (on a dozen sets of facts) and every
combination of the facts (under the named sets of options): 27 000 plans, about a second."""
import ctypes
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sdf_tools_amd", "csrc")

FLAGS = ["out16", "p16", "dense", "dense_generic", "fix", "dense3", "staged", "far_ok", "envelope", "standby", "standby_single", "fused",
         "select", "predicted", "handoff", "window_choice", "plane_skip", "standby_folds", "z_sweep", "far_pair"]
BITS = ["none", "caller", "copy", "pack", "rows"]
REPORT = ["none", "dense", "far"]
SIZES = ["yz_bytes", "plane16_bytes", "z_bytes", "bits_bytes", "unc_bytes", "planebits_bytes"]
OCC = {"mask": 0, "cells": 1, "bits": 2}


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(HERE, "plan_harness.cpp")
    out = os.path.join(HERE, "plan_harness.so")
    deps = [src, os.path.join(CSRC, "sdfgpu_plan.hpp"), os.path.join(CSRC, "sdfgpu_policy.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", src, "-o", out])
    L = ctypes.CDLL(out)
    L.plan_new.restype = ctypes.c_void_p
    L.plan_free.argtypes = [ctypes.c_void_p]
    L.plan_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    L.plan_far_report.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.plan_counter.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.plan_counter.restype = ctypes.c_int64
    L.plan_set_dense_skip.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.plan_run.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    return L


class Planner:
    """a fresh set of options and a fresh policy, as sdfgpu_create leaves them"""

    def __init__(self, L, **options):
        self.L, self.h = L, L.plan_new()
        for k, v in options.items():
            self.set(k, v)

    def set(self, name, value):
        assert self.L.plan_set_option(self.h, name.encode(), int(value)) == 0, name

    def plan(self, shape=(16, 32, 64), vb=False, occ="mask", occ16=True, out16=True, far_shape=(True, True), dense_slot_free=True,
             far_slot_free=True, dense_shape=None, z_wave_shape=None, fused_nz=None):
        """the facts of a shape as sdfgpu.hip's predicates state them, unless given"""
        nx, ny, nz = shape
        nzw = nz // 32
        if dense_shape is None:
            dense_shape = nz % 32 == 0 and 1 <= nzw <= 64 and nzw & (nzw - 1) == 0
        if z_wave_shape is None:
            z_wave_shape = nz in (64, 128, 256, 512, 1024)
        if fused_nz is None:
            fused_nz = nz in (512, 1024)
        facts = (ctypes.c_int64 * 14)(nx, ny, nz, vb, OCC[occ], occ16, out16, dense_shape, far_shape[0], far_shape[1], z_wave_shape,
                                      fused_nz, dense_slot_free, far_slot_free)
        out = (ctypes.c_int64 * 9)()
        self.L.plan_run(self.h, facts, out)
        p = {name: bool(out[0] >> k & 1) for k, name in enumerate(FLAGS)}
        p["bits"], p["report"] = BITS[out[1]], REPORT[out[2]]
        p.update({name: out[3 + k] for k, name in enumerate(SIZES)})
        return p

    def seq(self):
        return self.L.plan_counter(self.h, 0)

    def close(self):
        self.L.plan_free(self.h)


def _plan(L, options=None, **facts):
    p = Planner(L, **(options or {}))
    try:
        return p.plan(**facts)
    finally:
        p.close()


def _has(p, yes=(), no=()):
    assert [k for k in yes if not p[k]] == [] and [k for k in no if p[k]] == [], p


def test_named_situations(lib):
    n = 16 * 32 * 64
    # defaults: the tuned dense tier with the fix-up stage staged behind it, then the probe-selected sweeps
    p = _plan(lib)
    _has(p, ["dense", "staged", "p16", "select", "handoff", "window_choice", "envelope", "z_sweep"],
         ["dense_generic", "fix", "dense3", "predicted", "standby", "fused", "standby_folds", "plane_skip", "far_pair"])
    assert p["report"] == "dense" and p["bits"] == "pack" and p["z_bytes"] == 2 * n and p["bits_bytes"] == n // 8
    assert p["yz_bytes"] == 4 * n and p["plane16_bytes"] == 2 * n and p["unc_bytes"] == 0 and p["planebits_bytes"] == 0
    p = _plan(lib, vb=True)
    _has(p, ["dense", "p16", "select", "handoff", "window_choice", "z_sweep"], ["staged", "fix", "dense3", "predicted", "standby", "fused"])
    assert p["report"] == "dense"
    # a trusted dense tier: the stand-by pair, one launch that folds
    p = _plan(lib, {"expect_dense": 1})
    _has(p, ["dense", "standby", "standby_single", "standby_folds", "far_pair"], ["staged", "fused", "select", "predicted", "z_sweep", "envelope"])
    assert p["z_bytes"] == 0 and p["report"] == "dense"
    p = _plan(lib, {"expect_dense": 1, "standby_single": 0})
    _has(p, ["standby", "standby_folds"], ["standby_single"])
    p = _plan(lib, {"expect_dense": 1, "standby_fold": 0})
    _has(p, ["standby", "standby_single"], ["standby_folds"])
    for opts in ({"expect_dense": 1, "standby_far": 0}, {"expect_dense": 1, "fused_zy": 2}):
        p = _plan(lib, opts, shape=(8, 16, 512))
        _has(p, ["dense", "fused"], ["standby", "select", "z_sweep", "far_pair"])
    # without the dense tier
    p = _plan(lib, {"dense": 0})
    _has(p, ["select", "z_sweep"], ["dense", "dense_generic", "predicted", "fused"])
    assert p["report"] == "far" and p["bits"] == "none" and p["bits_bytes"] == 0
    assert _plan(lib, {"dense": 0}, far_slot_free=False)["report"] == "none"
    p = _plan(lib, {"dense": 0, "far_predict": 2})
    _has(p, ["select", "predicted", "plane_skip", "far_pair", "z_sweep"], ["dense", "fused", "standby"])
    assert p["report"] == "none" and p["planebits_bytes"] == ((16 * 32 + 16 + 255) & ~255) + 16 * 1 * 4
    _has(_plan(lib, {"dense": 0, "far_predict": 2}, occ="cells"), ["predicted"], ["plane_skip"])
    _has(_plan(lib, {"dense": 0, "far_predict": 2, "plane_skip": 0}), ["predicted"], ["plane_skip"])
    _has(_plan(lib, {"dense": 0, "far_predict": 2}, occ16=False), ["predicted"], ["plane_skip"])
    _has(_plan(lib, {"dense": 0, "far_predict": 2}, occ="bits", occ16=False), ["predicted", "plane_skip"])     # (the bit loader takes any alignment)
    _has(_plan(lib, {"dense": 0, "far_predict": 2}, shape=(4, 32, 64)), ["predicted"], ["plane_skip"])
    _has(_plan(lib, {"dense": 0, "far_predict": 2}, shape=(16, 1025, 64)), ["predicted"], ["plane_skip"])
    _has(_plan(lib, {"dense": 0, "far_predict": 2, "envelope_mode": 1}), ["select"], ["predicted"])
    _has(_plan(lib, {"dense": 0, "envelope_mode": 1}), ["select"], ["predicted"])
    # one unbounded sweep per axis / the fused sweep where it has an instance
    _has(_plan(lib, {"dense": 0, "envelope": 0}), ["z_sweep"], ["select", "fused", "far_ok", "envelope", "predicted"])
    p = _plan(lib, {"dense": 0, "envelope": 0}, shape=(8, 16, 512))
    _has(p, ["fused"], ["select", "z_sweep"])
    assert p["report"] == "none"
    # pointers off 16 bytes, shapes the tuned kernels do not take
    p = _plan(lib, out16=False)
    _has(p, ["dense", "dense_generic", "select"], ["out16", "p16", "fix", "staged", "dense3", "handoff"])
    assert p["bits"] == "rows" and p["bits_bytes"] == 16 * 32 * 2 * 4
    p = _plan(lib, shape=(8, 12, 30))
    _has(p, ["dense", "dense_generic", "select"], ["p16", "window_choice", "handoff", "staged"])
    assert p["bits_bytes"] == 8 * 12 * 4
    p = _plan(lib, occ="bits", occ16=False)
    _has(p, ["dense"], ["dense_generic"])
    assert p["bits"] == "copy" and p["bits_bytes"] == n // 8
    p = _plan(lib, occ="bits")
    assert p["bits"] == "caller" and p["bits_bytes"] == 0
    # fix-up mode keeps its undecided words in a field of their own; a staged stage without a z field too
    assert _plan(lib, {"fixup_mode": 1})["unc_bytes"] == n // 8
    p = _plan(lib, {"fused_zy": 2}, shape=(8, 16, 512))
    _has(p, ["staged", "fused"], ["z_sweep"])
    assert p["unc_bytes"] == 8 * 16 * 512 // 8


def test_far_habit_through_the_planner(lib):
    """After four far-field reports builds 1 - 15 are predicted and the 16th probes; FarHabit::seq counts every plan."""
    P = Planner(lib, dense=0)
    for _ in range(4):
        lib.plan_far_report(P.h, 1, 1)
    got = [P.plan()["predicted"] for _ in range(16)]
    assert got == [True] * 15 + [False] and P.seq() == 16
    P.close()


def test_invariants_over_the_cross_product(lib):
    option_axes = {"dense": (0, 1), "expect_dense": (0, 1), "envelope": (0, 1), "envelope_mode": (0, 1), "far_predict": (1, 2),
                   "standby_far": (0, 1), "standby_fold": (0, 1), "standby_single": (0, 1), "fused_zy": (0, 1, 2), "plane_skip": (0, 1)}
    fact_axes = {"shape": ((16, 32, 64), (8, 16, 512), (8, 12, 30)), "vb": (False, True), "occ": ("mask", "cells", "bits"),
                 "occ16": (False, True), "out16": (False, True), "far_shape": ((True, True), (False, True)),
                 "dense_slot_free": (False, True), "far_slot_free": (False, True)}
    # every combination of the options on a few sets of facts, every combination of the facts under a few sets of options
    all_options = [dict(zip(option_axes, ov)) for ov in itertools.product(*option_axes.values())]
    all_facts = [dict(zip(fact_axes, fv)) for fv in itertools.product(*fact_axes.values())]
    few_facts = [{}, {"vb": True}, {"shape": (8, 16, 512)}, {"shape": (8, 12, 30)}, {"out16": False}, {"occ": "cells"}, {"occ": "bits"},
                 {"occ": "bits", "occ16": False}, {"occ16": False, "shape": (8, 16, 512)}, {"far_shape": (False, True)},
                 {"dense_slot_free": False}, {"dense_slot_free": False, "far_slot_free": False}]
    few_options = [{}, {"expect_dense": 1}, {"expect_dense": 1, "standby_single": 0}, {"expect_dense": 1, "standby_fold": 0},
                   {"expect_dense": 1, "standby_far": 0}, {"expect_dense": 1, "fused_zy": 2}, {"fused_zy": 2}, {"dense": 0},
                   {"dense": 0, "far_predict": 2}, {"dense": 0, "far_predict": 2, "plane_skip": 0}, {"dense": 0, "envelope_mode": 1},
                   {"dense": 0, "envelope": 0}, {"envelope": 0}, {"far_predict": 2}]
    defaults = {"dense": 1, "expect_dense": 0, "envelope": 1, "envelope_mode": 0, "far_predict": 1, "standby_far": 1, "standby_fold": 1,
                "standby_single": 1, "fused_zy": 1, "plane_skip": 1}
    pairs = [(o, f) for o in all_options for f in few_facts] + [(dict(defaults, **o), f) for o in few_options for f in all_facts]
    P = Planner(lib)
    for opts, facts in pairs:
        P.set("policy_reset", 1)
        for k, v in opts.items():                             # (after the reset, which clears "expect_dense")
            P.set(k, v)
        lib.plan_set_dense_skip(P.h, 0)
        seq = P.seq()
        p = P.plan(**facts)
        what = (opts, facts, p)
        assert P.seq() == seq + 1, what
        assert not p["predicted"] or p["select"], what
        assert not p["select"] or (not p["fused"] and p["envelope"]), what
        assert not p["standby"] or not (p["fused"] or p["select"] or p["predicted"]), what
        assert not p["standby_folds"] or p["standby"], what
        assert not p["standby_single"] or p["standby"], what
        assert not p["plane_skip"] or p["predicted"], what
        assert not p["handoff"] or (p["p16"] and p["select"]), what
        assert p["z_sweep"] == (not p["fused"] and not p["standby"]) and (p["z_bytes"] > 0) == p["z_sweep"], what
        assert p["far_pair"] == (p["standby"] or p["predicted"]), what
        # (a build with the dense tier reports to the far slot when its own is taken and it probed)
        assert p["report"] in REPORT and (p["report"] != "dense" or p["dense"]) and (p["report"] != "far" or p["select"]), what
        assert not p["dense_generic"] or (p["dense"] and not (p["fix"] or p["dense3"] or p["staged"])), what
        assert (p["bits"] == "none") == (not p["dense"]) and (p["bits"] == "rows") == p["dense_generic"], what
        assert (p["bits_bytes"] > 0) == (p["bits"] in ("copy", "pack", "rows")), what
        # the staged fix-up stage finds storage for its undecided words: the z field's, or a field of its own
        shape = facts.get("shape", (16, 32, 64))
        n = shape[0] * shape[1] * shape[2]
        assert not p["staged"] or p["z_bytes"] >= n // 8 or p["unc_bytes"] == n // 8, what
        assert (p["plane16_bytes"] > 0) == p["p16"] and p["yz_bytes"] == 4 * n and (p["planebits_bytes"] > 0) == p["plane_skip"], what
    assert len(pairs) == 2 ** 9 * 3 * len(few_facts) + len(few_options) * 3 * 3 * 2 ** 6
    # DensePolicy::plan is called once: a pause of three builds is one build shorter after one plan, whatever the outcome
    for opts in ({}, {"dense": 0}):
        P.set("policy_reset", 1)
        P.set("dense", opts.get("dense", 1))
        lib.plan_set_dense_skip(P.h, 3)
        p = P.plan()
        assert not p["dense"] and lib.plan_counter(P.h, 1) == (2 if not opts else 3), (opts, p)
    P.close()
