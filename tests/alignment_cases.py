"""Plain data for the off-alignment tests (alignment_harness.py, test_gpu_alignment.py, test_alignment_harness_cpu.py): the parts
of DESIGN.md section 22 ("Caller pointers and their alignment") that the suite is driven by.  Nothing here runs on a GPU.

The header promises element alignment only: a byte mask may sit anywhere, a float / int32 / uint32 buffer and a cell record at any
multiple of 4.  A wider alignment selects a faster kernel, never another result."""

SENTINEL = 0xA5          # every byte of an arena that is not payload
BAND = 4096              # sentinel bytes in front of the arena and behind the payload, at least
LEAD = 256               # the payload starts LEAD + shift bytes into the arena, which is itself 256-byte aligned

# byte offsets from a 256-byte boundary, by the kind of buffer; 0 is the control
SHIFTS = {
    "bytes": (0, 1, 3, 4, 8, 15),        # uint8 masks
    "words": (0, 4, 8, 12),              # float / int32 / uint32 buffers
    "cells8": (0, 4),                    # COLLISION_CELL records
    "cells16": (0, 4, 8),                # TAGGED_OBJECT_COLLISION_CELL records
    "doubles": (0, 8),                   # a float64 gradient
}
# ... and the shift each kind takes in a case that moves every pointer of a call at once
ALL_OFF = {"bytes": 1, "words": 4, "cells8": 4, "cells16": 4, "doubles": 8}

# (nx, ny, nz) -> what the shape reaches.  Ordered from the scalar arms to the widest ones: the order the tests run in.
SHAPES = {
    (4, 5, 13): "scalar everywhere: the control that shows a shift changes nothing there",
    (6, 6, 20): "nz % 4 == 0, plane % 8 == 0: 4-voxel y and x sweeps, 16-bit plane field; no 16-byte z sweep",
    (5, 7, 48): "nz % 16 == 0 without a wave shape: k_sweep_z_vec16 or the generic z sweep; generic dense tier only",
    (9, 12, 64): "wave-private z sweep, tuned dense tier (2 words per row), 16-bit plane field, plane skipping (nx >= 8)",
    (3, 8, 512): "fused z+y kernel, 512-voxel instances of the far-field kernel, tuned dense tier with 16-byte row loads",
}
DENSITIES = (0.3, 0.002)   # synth.bernoulli_mask: the dense tier decides the first, the far-field pair the second

# Options every case starts from (the library's defaults, with the dense tier tried on every build) ...
OPTION_DEFAULTS = {
    "dense": 1, "dense_retry": 0, "plane16": 1, "fused_zy": 1, "envelope": 1, "envelope_mode": 0, "far_predict": 1, "plane_skip": 1,
    "z_wave": 1, "i32_handoff": 1, "far_threshold_y": 16, "far_threshold_x": 9,
}
# ... and the sets that force a tier.  "once": options that hold for the next build only and are set again before each one.
TIERS = {
    "default": {},
    "sweeps": {"dense": 0},
    "sweeps-int32-plane": {"dense": 0, "plane16": 0},
    "sweeps-z-workgroup": {"dense": 0, "z_wave": 0},
    "sweeps-unbounded": {"dense": 0, "envelope": 0, "fused_zy": 0},
    "fused": {"dense": 0, "fused_zy": 2},
    "fused-unbounded": {"dense": 0, "envelope": 0, "fused_zy": 2},
    "far-field-only": {"dense": 0, "envelope_mode": 1},
    "far-field-probed-handoff": {"dense": 0, "far_threshold_y": 1, "far_threshold_x": 1},
    "far-field-probed-no-handoff": {"dense": 0, "far_threshold_y": 1, "far_threshold_x": 1, "i32_handoff": 0},
    "far-field-predicted-plane-skip": {"dense": 0, "far_predict": 2, "plane_skip": 1},
    "dense-fixup": {"once": {"fixup_mode": 1}},
    "dense-kd3": {"once": {"dense3_mode": 1}},
}

# The audit: for every caller-supplied device pointer of the build path's entry points
#   kind      which SHIFTS row the pointer takes
#   widest    the widest access any reachable kernel makes through it, in bytes
#   predicate the host-side test (or, for k_unpack_bits_mask, the test in the kernel) that keeps that access off a pointer not aligned for it
#   narrow    the arm taken when the test fails
# DESIGN.md section 22 holds the same rows as prose; the tests walk this table (one pointer moved at a time, then all at once).
POINTERS = {
    "build_device": {
        "mask": ("bytes", 16, "launch_sweep_z / launch_pack_bits / fused_zy_eligible / plane_skip test d_filled % 16",
                 "k_sweep_z_generic<MaskLoader>, k_pack_bits_generic<MaskLoader>, K1 + K2 in K12's place, no row flags"),
        "out": ("words", 16, "build_device_impl: d_out % 16 gates plane16 (K3/16) and the tuned dense tier; launch_sweep_x tests it for its 4-voxel form",
                "int32 plane field + k_sweep_march<3, 1>, k_ball_dense_generic; the far-field x sweep stores floats"),
    },
    "build_cells_device": {
        "cells": ("cells8", 4, "none needed: CellLoader reads one float per record", "-"),
        "out": ("words", 16, "as build_device", "as build_device"),
    },
    "build_batch_device": {
        "masks": ("bytes", 16, "fast path: bytes only; above 128 voxels per axis each grid is a build_device", "as build_device"),
        "out": ("words", 16, "fast path: floats only; above 128 as build_device", "as build_device"),
    },
    "gradient_batch_device": {
        "sdf": ("words", 4, "none needed: k_batch_gradient reads floats", "-"),
        "out": ("words", 4, "none needed: one float per store (a float64 gradient: one double, 8-byte aligned by its type)", "-"),
    },
    "sweep_zy_device": {
        "mask": ("bytes", 16, "launch_sweep_z and fused_zy_eligible test d_filled % 16", "k_sweep_z_generic<MaskLoader>, K1 + K2"),
        "plane": ("words", 16, "the tiered form, launch_sweep_y's 4-voxel form and fused_zy_eligible test d_plane_dsq % 16",
                  "untiered K1 + k_sweep_march<2, 1>; the far-field y sweep stores int32"),
        "far": ("words", 4, "none needed: a 4-byte device copy", "-"),
    },
    "sweep_x_device": {
        "plane": ("words", 16, "launch_sweep_x tests d_in % 16", "k_sweep_march<3, 1>"),
        "out": ("words", 16, "launch_sweep_x tests d_out % 16", "k_sweep_march<3, 1>"),
        "maxdsq": ("words", 4, "none needed", "-"),
        "status": ("words", 4, "none needed", "-"),
    },
    "sweep_x_lines_device": {
        "plane": ("words", 16, "the tiered form and launch_sweep_x test d_plane_dsq % 16; launch_envelope tests in_i32 % 16 for its vector loads",
                  "untiered k_sweep_march<3, 1>, unbounded"),
        "out": ("words", 16, "launch_sweep_x tests d_out % 16", "k_sweep_march<3, 1>; the far-field x sweep stores floats"),
        "maxdsq": ("words", 4, "none needed", "-"),
    },
    "pack_bits_device": {
        "mask": ("bytes", 16, "launch_pack_bits tests d_mask % 16", "k_pack_bits_generic<MaskLoader>"),
        "bits": ("words", 4, "none needed: one word per store", "-"),
    },
    "dense_ball_device": {
        "bits": ("words", 16, "launch_ball_dense tests d_bits % 16", "the planes are copied into the handle's scratch first"),
        "out": ("words", 16, "launch_ball_dense tests d_out % 16", "the field is built in the handle's scratch and copied out"),
        "maxdsq": ("words", 4, "none needed", "-"),
        "uncertified": ("words", 4, "none needed", "-"),
    },
    "slab_dense_phase": {
        "mask": ("bytes", 16, "launch_pack_bits tests d_mask % 16", "k_pack_bits_generic<MaskLoader>"),
        "bits": ("words", 16, "launch_ball_dense tests d_bits % 16", "copied into scratch"),
        "out": ("words", 16, "launch_ball_dense tests d_out % 16", "built in scratch and copied out"),
        "small": ("words", 4, "none needed", "-"),
    },
    "classify_cells_device": {
        "cells": ("cells8", 4, "none needed", "-"),
        "mask": ("bytes", 1, "none needed", "-"),
    },
    "upload_classified": {
        "mask": ("bytes", 16, "k_unpack_bits_mask tests mask % 16 itself", "16 byte stores per lane"),
    },
}


def moves(entry, kinds=None):
    """[(label, {pointer: shift})]: the control, one pointer moved at a time through its non-zero shifts, every pointer at once.
    kinds overrides a pointer's kind (16-byte cell records, a double gradient)."""
    ptrs = {name: (kinds or {}).get(name, row[0]) for name, row in POINTERS[entry].items()}
    out = [("control", {name: 0 for name in ptrs})]
    for name, kind in ptrs.items():
        for s in SHIFTS[kind]:
            if s:
                out.append(("%s+%d" % (name, s), {n: (s if n == name else 0) for n in ptrs}))
    out.append(("all-off", {name: ALL_OFF[kind] for name, kind in ptrs.items()}))
    return out
