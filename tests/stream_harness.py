"""The harness of test_gpu_stream_order.py: run one library call on a non-blocking side stream whose inputs arrive late.

A Case keeps every device input buffer filled with a DECOY (another valid input of the same shape and type) and every output
buffer with a sentinel.  arm() enqueues on the side stream a delay and, behind it, the copies of the REAL inputs over the decoys.
A call that honours its stream reads the real inputs and its consumer (a clone enqueued on the side stream) sees their result;
a kernel, memset or read-back issued on another stream runs during the delay, reads the decoy (or stale status words) and is
found out.  Witnesses -- clones of the inputs enqueued on the null stream and on a second side stream -- must still hold the
decoy afterwards: that is what shows that the delay held and that the streams do not share a hardware queue.

Nothing here can wait forever: the delay is torch.cuda._sleep (a bounded spin on the device clock) or, without it, a chain of
element-wise kernels."""
import time

import numpy as np
import pytest
import torch

SENTINEL = 0xA5
FLOOR_MS = 20.0          # the shortest delay a case uses
CEILING_MS = 400.0       # ... and the longest (ten times a warm call that a busy host stretched)
MARGIN = 10.0            # delay >= MARGIN x the warm host-side duration of the case's own call


class Delay:
    """A device-side delay of a given length on the current stream, calibrated once with HIP events."""

    def __init__(self):
        torch.cuda.synchronize()
        self.sleep = getattr(torch.cuda, "_sleep", None)
        if self.sleep is not None:
            self.unit = 20_000_000                                   # cycles
            self.sleep(1000)
        else:                                                        # a chain of element-wise passes over 256 MiB
            self.block = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
            self.unit = 8                                            # passes
            self._enqueue(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        self._enqueue(self.unit)
        b.record()
        b.synchronize()
        self.units_per_ms = self.unit / a.elapsed_time(b)
        print("[stream harness] %s: %.0f units per ms" % ("torch.cuda._sleep cycles" if self.sleep is not None else "element-wise passes", self.units_per_ms))

    def _enqueue(self, units):
        if self.sleep is not None:
            self.sleep(int(units))
        else:
            for _ in range(int(units)):
                self.block.add_(1.0)

    def enqueue(self, ms):
        self._enqueue(max(1, int(ms * self.units_per_ms + 0.5)))


def independent(delay, a, b):
    """a sleeping stream `a` does not hold back work on stream `b` (they do not share a hardware queue).  Decided without
    waiting for a time: once b's event has completed, a's sleep has completed too if and only if b stood behind it."""
    torch.cuda.synchronize()
    done_a, done_b = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(a):
        delay.enqueue(5.0)
        done_a.record()
    with torch.cuda.stream(b):
        done_b.record()
    done_b.synchronize()
    free = not done_a.query()
    torch.cuda.synchronize()
    return free


def pick_streams(delay, count=2, candidates=12):
    """`count` side streams that share a hardware queue neither with the null stream nor with each other.  The runtime deals
    its few hardware queues (4 by default) out to streams as they are created, so two streams taken blindly share one every
    few tries, and a witness behind the delay would show nothing.  Fails (no skip) when the runtime offers no such set."""
    null = torch.cuda.default_stream()
    picked = []
    for _ in range(candidates):
        c = torch.cuda.Stream()
        with torch.cuda.stream(c):
            torch.zeros(1, device="cuda")                        # (first use: the stream has its queue now)
        if all(independent(delay, c, o) and independent(delay, o, c) for o in [null] + picked):
            picked.append(c)
            if len(picked) == count:
                return picked
    pytest.fail("no %d side streams among %d that run beside the null stream and beside each other: fewer than %d hardware "
                "queues (GPU_MAX_HW_QUEUES)?" % (count, candidates, count + 1))


def to_device(a):
    """numpy array -> device bytes (uint8 tensor; .data_ptr() is what the C ABI takes)"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.nbytes == b.nbytes and np.array_equal(a.view(np.uint8).reshape(-1), b.view(np.uint8).reshape(-1))


def same_or_nan(a, b):
    """bit-equal, or NaN in both (the restatements' NaNs carry numpy's payload, the kernels' the device's)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return same(a, b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


class _Input:
    def __init__(self, name, decoy, real):
        decoy, real = np.ascontiguousarray(decoy), np.ascontiguousarray(real)
        assert decoy.shape == real.shape and decoy.dtype == real.dtype, name
        assert not same(decoy, real), "%s: the decoy equals the real input" % name
        self.name, self.dtype, self.shape = name, real.dtype, real.shape
        self.buf, self.decoy, self.real = to_device(decoy), to_device(decoy), to_device(real)


class Case:
    """One call (or one sequence of calls) on `side`.  `other` is the second side stream of the witnesses (None: the null stream
    alone, for the tests that need both side streams for library calls)."""

    def __init__(self, delay, side, other=None):
        self.delay = delay
        self.side = side
        self.other = other
        self.ins, self.outs, self.seen, self.clones = {}, {}, [], {}
        self.warm_ms, self.delay_ms = 0.0, FLOOR_MS

    def input(self, name, decoy, real):
        self.ins[name] = _Input(name, decoy, real)
        return self.ins[name].buf.data_ptr()

    def output(self, name, nbytes):
        self.outs[name] = torch.full((max(int(nbytes), 1),), SENTINEL, dtype=torch.uint8, device="cuda")
        return self.outs[name].data_ptr()

    def ptr(self, name):
        return (self.ins[name].buf if name in self.ins else self.outs[name]).data_ptr()

    def restore(self):
        for i in self.ins.values():
            i.buf.copy_(i.decoy)
        for o in self.outs.values():
            o.fill_(SENTINEL)
        torch.cuda.synchronize()

    def warm(self, call):
        """one undelayed call on the decoys: the handle's scratch is allocated, its first-use tables are uploaded, and the
        warm host-side duration of the call sizes the delay"""
        torch.cuda.synchronize()
        call()
        self.side.synchronize()
        self.restore()
        t0 = time.perf_counter()
        call()
        self.side.synchronize()
        self.warm_ms = (time.perf_counter() - t0) * 1e3
        self.restore()
        self.delay_ms = min(CEILING_MS, max(FLOOR_MS, MARGIN * self.warm_ms))

    def arm(self):
        torch.cuda.synchronize()
        print("[stream harness] warm call %.3f ms on the host, delay %.1f ms" % (self.warm_ms, self.delay_ms))
        with torch.cuda.stream(self.side):
            self.delay.enqueue(self.delay_ms)
            for i in self.ins.values():
                i.buf.copy_(i.real, non_blocking=True)
        self.witness("when the delayed producer had been enqueued")

    def witness(self, when):
        for i in self.ins.values():
            self.seen.append((when, "the null stream", i, i.buf.clone()))
            if self.other is not None:
                with torch.cuda.stream(self.other):
                    self.seen.append((when, "the second side stream", i, i.buf.clone()))

    def consume(self, also=()):
        """the consumer: clones of the outputs (and of the inputs a call updates in place) enqueued on the side stream"""
        with torch.cuda.stream(self.side):
            for name in list(self.outs) + list(also):
                self.clones[name] = (self.ins[name].buf if name in self.ins else self.outs[name]).clone()

    def finish(self):
        """wait for everything, check the witnesses, return {name: bytes the consumer saw}; the buffers themselves must hold
        the same bytes once everything has finished"""
        self.side.synchronize()
        if self.other is not None:
            self.other.synchronize()
        torch.cuda.synchronize()
        for when, where, i, t in self.seen:
            if not torch.equal(t, i.decoy):
                pytest.fail("witness of input '%s' on %s, taken %s, does not hold the decoy: the delay of %.1f ms (warm call %.2f ms) "
                            "did not hold, or that stream shares a hardware queue with the side stream -- this case showed nothing"
                            % (i.name, where, when, self.delay_ms, self.warm_ms))
        got = {}
        for name, t in self.clones.items():
            buf = self.ins[name].buf if name in self.ins else self.outs[name]
            assert torch.equal(t, buf), "'%s' changed after the side stream's consumer read it" % name
            got[name] = t.cpu().numpy()
        return got


def view(raw, dtype, shape=None):
    a = raw.view(dtype)
    return a if shape is None else a[:int(np.prod(shape))].reshape(shape)


def expect(what, got, real, decoy=None, eq=same):
    """got must be the reference of the REAL input; the reference of the decoy must differ from it, or the case could not tell"""
    if decoy is not None:
        assert not eq(real, decoy), "%s: the reference of the decoy equals the reference of the real input" % what
    if eq(got, real):
        return
    g = np.ascontiguousarray(got).view(np.uint8)
    if decoy is not None and eq(got, decoy):
        why = "it is the result of the DECOY: the work ran ahead of the producer on its stream"
    elif bool(np.all(g == SENTINEL)):
        why = "it still holds the sentinel: the consumer on the side stream ran ahead of the work"
    else:
        why = "it is neither the real input's result nor the decoy's (%d of %d bytes are the sentinel)" % (int((g == SENTINEL).sum()), g.size)
    pytest.fail("%s differs from the reference of the real input: %s" % (what, why))
