#!/usr/bin/env python3
"""Differential fuzzing of the batched small-grid build on a GPU box (sdf_tools_amd/csrc/sdfgpu_batch.hip):
random shapes around the changes of P (planes per workgroup of k_batch_zy), batch sizes, scenes mixed within one batch (far-field
grids beside dense ones, all filled beside all free), resolutions, borders and entry points, on ONE handle with red zones on and
device buffers of exact size from sdfgpu_device_malloc.  Every voxel of every grid is compared as uint32 with oracle.exact_sdf,
the extrema as exact doubles, and each grid a second time with its single build.

  entry points   host      sdfgpu_build_batch
                 device    sdfgpu_build_batch_device on the null stream or a torch stream (the caller's resolutions are
                           overwritten as soon as the call returns)
                 tagged    sdfgpu_build_tagged_objects (ids 0, absent and repeated; both unknown_is_filled; 16- and 24-byte
                           records with shifted offsets; cells = NULL re-using the records)
                 gradient  sdfgpu_gradient_batch_device on a device batch result, fp32 / fp64, edge gradients on / off, against
                           analysis_scenes.grid_gradient and sdfgpu_gradient_device per grid

A fixed prelude (one small batch for each P in 1 .. 8 with B nx % P != 0 among them, one batch on the per-grid path) runs before
the random phase whatever the time budget is.  Between batches a single build of another shape sometimes runs on the same handle
and is checked too; sdfgpu_get_extrema must keep answering for the last single build.

  python tools/fuzz_batch.py [seconds] [seed]        FUZZ_VERBOSE=1 prints every iteration before it runs

On the first mismatch one reproducer line is printed, the batch's masks are saved as fuzz_batch_fail_masks.npy in $FUZZ_OUT_DIR
(default fuzz_out/, kept out of git) and the exit code is 1.
"""
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import analysis_scenes as A  # noqa: E402
from oracle import oracle as O  # noqa: E402
from sdf_tools_amd import capi, synth  # noqa: E402

AXES = [1, 2, 3, 5, 7, 8, 15, 16, 20, 25, 31, 32, 33, 40, 63, 64, 65, 96, 100, 127, 128]
BATCHES = [1, 2, 3, 5, 7, 8, 9, 31, 32, 33, 100]
RESOLUTIONS = [1.0, 0.5, 0.25, 0.05, 0.037, 0.01]
BERNOULLI_P = [0.5, 0.3, 0.1, 0.05, 0.03, 0.02, 0.01, 0.001, 0.9, 0.96, 0.99, 0.999]        # tools/fuzz_parity.py's
KINDS = ["bernoulli", "spheres", "voxels", "structured", "free", "filled", "serpentine", "comb", "stripes", "checkerboard",
         "nested_shells"]
ENTRIES = ["host", "device", "tagged", "gradient"]
VOXEL_CAP = 2200000          # the oracle takes 1.7 s for 2^21 Bernoulli(0.5) voxels: about 2 s an iteration at most
PALETTE = np.array([0, 1, 2, 3, 5, 8, 13, 40], np.uint32)
# (shape, B) of the prelude: P = 1 .. 8 in turn; 3 * 6 % 5 and 3 * 11 % 8 are not 0
PRELUDE = [((5, 33, 32), 2), ((7, 16, 25), 3), ((25, 20, 15), 2), ((9, 16, 15), 3), ((6, 20, 10), 3), ((7, 10, 16), 2),
           ((5, 9, 16), 3), ((11, 8, 8), 3)]
PRELUDE_SLOW = ((3, 5, 129), 2)


# ---- the launch plan of DESIGN section 18, restated --------------------------------------------------------------------------------
def canonical(shape):
    """singleton axes to the front (sdfgpu_context.hip canonical_dims)"""
    nx, ny, nz = (int(s) for s in shape)
    if nz == 1:
        nx, ny, nz = 1, nx, ny
    if nz == 1:
        nx, ny, nz = 1, nx, ny
    if ny == 1:
        nx, ny = 1, nx
    return nx, ny, nz


def fast_shape(shape):
    return max(shape) <= 128


def planes_per_workgroup(shape, batch):
    """P = max(1, min(1024 / (ny nz), 8, B nx)) on the canonical shape"""
    nx, ny, nz = canonical(shape)
    return max(1, min(1024 // (ny * nz), 8, batch * nx))


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def structured(rng, shape):
    """kind 4 of tools/fuzz_parity.py: slabs over the whole extent of two axes, solid boxes, box shells; now and then noise or the
    complement.  Long empty runs: the outward min-plus walks run their full length."""
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
    return m


def draw_scene(rng, shape, kind=None):
    kind = str(rng.choice(KINDS)) if kind is None else kind
    seed = int(rng.integers(1 << 30))
    if kind == "bernoulli":
        p = float(rng.choice(BERNOULLI_P))
        return synth.bernoulli_mask(shape, p, seed), "bernoulli %g" % p
    if kind == "spheres":
        return synth.spheres_mask(shape, int(rng.integers(1, 5)), (1, 9), seed), kind
    if kind == "voxels":
        m = np.zeros(shape, np.uint8)
        for _ in range(int(rng.integers(1, 4))):
            m[tuple(int(rng.integers(0, s)) for s in shape)] = 1
        if rng.random() < 0.4:
            return 1 - m, "voxels complement"
        return m, kind
    if kind == "structured":
        return structured(rng, shape), kind
    if kind in ("free", "filled"):
        return np.full(shape, int(kind == "filled"), np.uint8), kind
    if kind in ("comb", "stripes"):
        axis = int(rng.integers(0, 3))
        return np.ascontiguousarray(getattr(A, kind)(shape, axis)), "%s %d" % (kind, axis)
    if kind == "nested_shells":
        return A.nested_shells(shape, int(rng.integers(1, 3))), kind
    return np.ascontiguousarray(getattr(A, kind)(shape)), kind


def draw_shape(rng):
    """Every axis from AXES; at least half of the draws are planes of at most 1024 cells (P > 1); now and then an axis of 129 or
    130 (the per-grid path)."""
    small = rng.random() < 0.6
    while True:
        shape = [int(rng.choice(AXES)) for _ in range(3)]
        c = canonical(shape)                                 # (singleton axes move to the front: the plane is the canonical one)
        if not small or c[1] * c[2] <= 1024:
            break
    if rng.random() < 0.07:
        shape[int(rng.integers(0, 3))] = int(rng.choice([129, 130]))
    return tuple(shape)


def draw_batch(rng, shape, cap=VOXEL_CAP):
    n = int(np.prod(shape))
    fits = [b for b in BATCHES if b * n <= cap]
    return int(rng.choice(fits)) if fits else 1


# ---- comparisons -------------------------------------------------------------------------------------------------------------------
class Mismatch(Exception):
    pass


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_bits_or_nan(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def first_difference(got, want, nan_equal=False):
    bad = bits(got) != bits(want)
    if nan_equal:
        bad &= ~(np.isnan(got) & np.isnan(want))
    idx = tuple(int(v) for v in np.argwhere(bad)[0])
    return "%d voxels differ, the first at %s: got %r want %r" % (int(bad.sum()), idx, got[idx].item(), want[idx].item())


def check_fields(what, got, ext, masks, res, vb):
    """every grid of a batch result against the oracle: voxels as uint32, extrema as exact doubles"""
    if got.shape != masks.shape or got.dtype != np.float32 or len(ext) != masks.shape[0]:
        raise Mismatch("%s: result of shape %s / %d extrema for masks %s" % (what, got.shape, len(ext), masks.shape))
    wants = []
    for b in range(masks.shape[0]):
        want, want_ext, _ = O.exact_sdf(masks[b], float(res[b]), vb)
        if not same_bits(got[b], want):
            raise Mismatch("%s: grid %d against the oracle: %s" % (what, b, first_difference(got[b], want)))
        if tuple(ext[b]) != tuple(float(v) for v in want_ext):
            raise Mismatch("%s: grid %d extrema: got %r want %r" % (what, b, tuple(ext[b]), tuple(want_ext)))
        wants.append((want, tuple(float(v) for v in want_ext)))
    return wants


class Fuzz:
    def __init__(self, seed):
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self.ctx = capi.SdfGpu(0)
        self.ctx.set_option("redzone", 1)
        self.last_single = None                  # what sdfgpu_get_extrema must keep saying
        self.streams = {}
        self.counts = {"batches": 0, "grids": 0, "singles": 0, "entry": {e: 0 for e in ENTRIES}, "P": {}, "paths": {"fast": 0, "slow": 0}}

    def close(self):
        self.ctx.close()

    # -- helpers
    def stream(self, name):
        """'null' or 'torch': the stream handle to pass (0 = the null stream)"""
        if name == "null":
            return 0
        import torch
        if "torch" not in self.streams:
            self.streams["torch"] = torch.cuda.Stream()
        return self.streams["torch"].cuda_stream

    def after_batch(self, what, shape):
        fast, launches = self.ctx.last_batch_info()
        if fast != fast_shape(shape) or launches != (2 if fast else -1):
            raise Mismatch("%s: last_batch_info says %r for shape %s" % (what, (fast, launches), shape))
        if self.last_single is not None and self.ctx.get_extrema() != self.last_single:
            raise Mismatch("%s: get_extrema after the batch says %r, the last single build had %r" % (what, self.ctx.get_extrema(), self.last_single))

    def single(self, what, mask, res, vb, want):
        one, one_ext = self.ctx.build(mask, res, vb)
        self.last_single = one_ext
        if not same_bits(one, want[0]) or one_ext != want[1]:
            raise Mismatch("%s: the single build differs from the oracle (extrema %r want %r)" % (what, one_ext, want[1]))

    # -- entry points
    def run_host(self, masks, res, per_grid, vb, info):
        got, ext = self.ctx.build_batch(masks, np.array(res) if per_grid else res[0], vb)
        self.after_batch("build_batch", masks.shape[1:])
        wants = check_fields("build_batch", got, ext, masks, res, vb)
        for b in range(masks.shape[0]):
            self.single("build_batch grid %d" % b, masks[b], res[b], vb, wants[b])

    def device_batch(self, masks, res, per_grid, vb, stream_name):
        """build_batch_device into an exact-size output; returns (d_out, fields, extrema); the caller frees d_out"""
        ctx = self.ctx
        B, n = masks.shape[0], int(np.prod(masks.shape[1:]))
        d_in, d_out = ctx.device_malloc(B * n), ctx.device_malloc(B * n * 4)
        ctx.copy_from_host(d_in, masks)
        arr = np.array(res, np.float64)
        ctx.build_batch_device(d_in, B, masks.shape[1:], d_out, arr if per_grid else res[0], vb, self.stream(stream_name))
        arr[:] = -1.0                                 # (consumed before the call returned)
        ext = ctx.get_extrema_batch(B)
        got = ctx.copy_to_host(np.empty(masks.shape, np.float32), d_out)
        ctx.device_free(d_in)
        return d_out, got, ext

    def run_device(self, masks, res, per_grid, vb, info):
        d_out, got, ext = self.device_batch(masks, res, per_grid, vb, info["stream"])
        self.ctx.device_free(d_out)
        self.after_batch("build_batch_device", masks.shape[1:])
        wants = check_fields("build_batch_device", got, ext, masks, res, vb)
        for b in range(masks.shape[0]):
            self.single("build_batch_device grid %d" % b, masks[b], res[b], vb, wants[b])

    def run_gradient(self, masks, res, per_grid, vb, info):
        ctx = self.ctx
        shape = masks.shape[1:]
        B, n = masks.shape[0], int(np.prod(shape))
        d_sdf, got, ext = self.device_batch(masks, res, per_grid, vb, info["stream"])
        self.after_batch("build_batch_device", shape)
        wants = check_fields("build_batch_device (gradient input)", got, ext, masks, res, vb)
        for b in range(B):
            self.single("build_batch_device (gradient input) grid %d" % b, masks[b], res[b], vb, wants[b])
        f64, edge = info["f64"], info["edge"]
        dt, w = (np.float64, 8) if f64 else (np.float32, 4)
        d_g, d_one = ctx.device_malloc(B * n * 3 * w), ctx.device_malloc(n * 3 * w)
        s = self.stream(info["stream"])
        ctx.gradient_batch_device(d_sdf, B, shape, d_g, np.array(res) if per_grid else res[0], edge, f64, s)
        if s:
            import torch
            torch.cuda.synchronize()
        grad = ctx.copy_to_host(np.empty(masks.shape + (3,), dt), d_g)
        for b in range(B):
            want = A.grid_gradient(got[b], float(res[b]), edge).astype(dt)
            if not same_bits_or_nan(grad[b], want):
                raise Mismatch("gradient_batch_device: grid %d against grid_gradient: %s" % (b, first_difference(grad[b], want, True)))
            ctx.gradient_device(d_sdf + 4 * b * n, shape, d_one, float(res[b]), edge, f64, s)
            if s:
                torch.cuda.synchronize()
            one = ctx.copy_to_host(np.empty(tuple(shape) + (3,), dt), d_one)
            if not same_bits_or_nan(grad[b], one):
                raise Mismatch("gradient_batch_device: grid %d against gradient_device: %s" % (b, first_difference(grad[b], one, True)))
        for p in (d_sdf, d_g, d_one):
            ctx.device_free(p)

    def run_tagged(self, masks, res, per_grid, vb, info):
        """masks[0] is the occupancy of the ONE grid of records; the object ids are regions or noise over PALETTE"""
        rng, ctx = self.rng, self.ctx
        shape = masks.shape[1:]
        n = int(np.prod(shape))
        occ = masks[0].astype(np.float32)
        pick = rng.random(shape) < 0.1
        occ[pick] = rng.choice(np.array([0.5, 0.50001, 0.49999], np.float32), int(pick.sum()))
        if rng.random() < 0.5:
            obj = rng.choice(PALETTE, size=shape)
        else:                                          # slabs of one id along an axis: far-field grids per id
            ax = int(rng.integers(0, 3))
            line = PALETTE[(np.arange(shape[ax]) * len(PALETTE)) // shape[ax]][rng.permutation(shape[ax]) if rng.random() < 0.3 else slice(None)]
            obj = np.broadcast_to(line.reshape([-1 if k == ax else 1 for k in range(3)]), shape).copy()
        stride, occ_off, obj_off = info["layout"]
        raw = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
        raw[:, occ_off:occ_off + 4] = occ.reshape(-1).view(np.uint8).reshape(n, 4)
        raw[:, obj_off:obj_off + 4] = np.ascontiguousarray(obj, np.uint32).reshape(-1).view(np.uint8).reshape(n, 4)
        ids, unknown = info["ids"], info["unknown"]
        r = float(res[0])
        filled = (occ > 0.5) | (unknown & (occ == 0.5))
        per_id = np.stack([(filled & (obj == i)).astype(np.uint8) for i in ids])
        kw = dict(unknown_is_filled=unknown, resolution=r, add_virtual_border=vb, cell_stride=stride, occupancy_offset=occ_off, object_id_offset=obj_off)
        got, ext = ctx.build_tagged_objects(raw, shape, ids, **kw)
        self.after_batch("build_tagged_objects", shape)
        wants = check_fields("build_tagged_objects", got, ext, per_id, [r] * len(ids), vb)
        if info["reuse"]:                              # cells = NULL: the records of the call before, other ids first
            again, ext2 = ctx.build_tagged_objects(None, shape, ids[::-1], **kw)
            self.after_batch("build_tagged_objects (cells = NULL)", shape)
            check_fields("build_tagged_objects (cells = NULL)", again, ext2, per_id[::-1], [r] * len(ids), vb)
        for b, i in enumerate(ids):
            one, one_ext = ctx.build_tagged_cells(raw, shape, object_mode=2, object_ids=[i], **kw)
            self.last_single = one_ext
            if not same_bits(one, wants[b][0]) or one_ext != wants[b][1]:
                raise Mismatch("build_tagged_objects: the single tagged build of id %d differs from the oracle" % i)

    # -- one iteration
    def batch(self, it, shape, B, entry, kinds=None):
        rng = self.rng
        per_grid = bool(rng.integers(0, 2)) and entry != "tagged"
        res = [float(rng.choice(RESOLUTIONS)) for _ in range(B)] if per_grid else [float(rng.choice(RESOLUTIONS))] * B
        vb = bool(rng.integers(0, 2))
        info = {"stream": str(rng.choice(["null", "torch"])) if entry in ("device", "gradient") else "-"}
        if entry == "tagged":
            layout = [(16, 0, 8), (24, 4, 16), (24, 8, 20)][int(rng.integers(0, 3))]
            ids = [int(v) for v in rng.choice(np.concatenate([PALETTE, np.array([0, 7, 99], np.uint32)]), size=B)]
            info.update(layout=layout, ids=ids, unknown=bool(rng.integers(0, 2)), reuse=rng.random() < 0.4)
            scenes = [draw_scene(rng, shape, "bernoulli" if kinds else None)]
        else:
            scenes = [draw_scene(rng, shape, kinds[b % len(kinds)] if kinds else None) for b in range(B)]
        if entry == "gradient":
            info.update(f64=bool(rng.integers(0, 2)), edge=bool(rng.integers(0, 2)))
        masks = np.stack([np.ascontiguousarray(m, np.uint8) for m, _ in scenes])
        names = [k for _, k in scenes]
        P = planes_per_workgroup(shape, B)
        line = ("seed %d iteration %s shape %s B %d P %d scenes %s resolutions %s border %s entry %s %s" %
                (self.seed, it, "x".join(map(str, shape)), B, P, names, sorted(set(res)) if per_grid else res[0], vb, entry,
                 {k: v for k, v in info.items() if v != "-"}))
        if os.environ.get("FUZZ_VERBOSE"):
            print(line, flush=True)
        try:
            getattr(self, "run_" + entry)(masks, res, per_grid, vb, info)
        except (Mismatch, AssertionError, capi.SdfGpuError) as e:        # (a refusal or a canary report is a finding too)
            out_dir = os.environ.get("FUZZ_OUT_DIR", "fuzz_out")
            os.makedirs(out_dir, exist_ok=True)
            np.save(os.path.join(out_dir, "fuzz_batch_fail_masks.npy"), masks)
            if not isinstance(e, Mismatch):
                traceback.print_exc()
            print("MISMATCH %s: %s" % (line, e), flush=True)
            sys.exit(1)
        c = self.counts
        c["batches"] += 1
        c["grids"] += B
        c["entry"][entry] += 1
        if fast_shape(shape):
            c["paths"]["fast"] += 1
            c["P"][P] = c["P"].get(P, 0) + 1
        else:
            c["paths"]["slow"] += 1

    def interleaved_single(self, it):
        rng = self.rng
        shape = tuple(int(rng.choice(AXES)) for _ in range(3))
        while np.prod(shape) > 1 << 19:
            shape = tuple(max(1, s // 2) if s == max(shape) else s for s in shape)
        m, kind = draw_scene(rng, shape)
        res, vb = float(rng.choice(RESOLUTIONS)), bool(rng.integers(0, 2))
        want, want_ext, _ = O.exact_sdf(m, res, vb)
        try:
            self.single("single build", m, res, vb, (want, tuple(float(v) for v in want_ext)))
            if self.ctx.get_extrema() != self.last_single:
                raise Mismatch("get_extrema does not answer for the single build")
        except (Mismatch, capi.SdfGpuError) as e:
            print("MISMATCH seed %d iteration %s single build between batches shape %s scene %s resolution %g border %s: %s" %
                  (self.seed, it, "x".join(map(str, shape)), kind, res, vb, e), flush=True)
            sys.exit(1)
        self.counts["singles"] += 1


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    fz = Fuzz(seed)
    t0 = time.time()
    mixed = ["filled", "free", "bernoulli", "structured", "voxels"]
    for k, (shape, B) in enumerate(PRELUDE):
        assert planes_per_workgroup(shape, B) == k + 1
        fz.batch("prelude %d" % k, shape, B, ENTRIES[k % 4], mixed[k % 5:] + mixed[:k % 5])
    fz.batch("prelude slow", PRELUDE_SLOW[0], PRELUDE_SLOW[1], "device", mixed)
    it = 0
    while time.time() - t0 < budget:
        shape = draw_shape(fz.rng)
        entry = str(fz.rng.choice(ENTRIES))
        # (the numpy restatement of the gradient costs more per voxel than the oracle's EDT)
        fz.batch(it, shape, draw_batch(fz.rng, shape, VOXEL_CAP // 4 if entry == "gradient" else VOXEL_CAP), entry)
        if fz.rng.random() < 0.25:
            fz.interleaved_single(it)
        it += 1
    fz.ctx.redzone_check()
    fz.close()
    c = fz.counts
    print("fuzz OK: %d batches, %d grids and %d single builds in %.0f s (seed %d), red zones on; entry points %s; P %s; paths %s" %
          (c["batches"], c["grids"], c["singles"], time.time() - t0, seed, c["entry"], dict(sorted(c["P"].items())), c["paths"]))


if __name__ == "__main__":
    main()
