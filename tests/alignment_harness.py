"""Buffers at chosen byte offsets inside sentinel bands, for the off-alignment tests.

A buffer under test is the payload of an ARENA: a 256-byte-aligned uint8 array whose every other byte holds SENTINEL.  The payload
starts LEAD + shift bytes into the arena; BAND sentinel bytes lie in front of the arena and at least BAND behind the payload, so a
store that strays by up to 4 KiB either way lands in bytes that are checked.  The arena is a torch tensor on the GPU
(DeviceArena) or a numpy array (HostArena: the CPU test of the checking itself); both check their bands with check_bands below.

    a = DeviceArena(nbytes, shift)       a.ptr is what the library gets
    a.write(array)                       payload <- the array's bytes
    ... the call ...
    a.check("build_device out+4")        both bands intact, or AssertionError naming the first changed byte
    a.read(np.float32, shape)            the payload, read back from the same offset
"""
import numpy as np

from alignment_cases import BAND, LEAD, SENTINEL


def check_bands(front, back, what):
    """front / back: uint8 numpy arrays, the bytes in front of the payload and behind it.  Raises AssertionError naming how many
    bytes changed and where the nearest one lies relative to the payload."""
    bad_f, bad_b = np.flatnonzero(front != SENTINEL), np.flatnonzero(back != SENTINEL)
    if bad_f.size == 0 and bad_b.size == 0:
        return
    msg = []
    if bad_f.size:
        msg.append("%d byte(s) IN FRONT of the buffer changed, the nearest %d byte(s) before its first (now 0x%02X)"
                   % (bad_f.size, front.size - int(bad_f[-1]), int(front[bad_f[-1]])))
    if bad_b.size:
        msg.append("%d byte(s) BEHIND the buffer changed, the nearest %d byte(s) past its last (now 0x%02X)"
                   % (bad_b.size, int(bad_b[0]) + 1, int(back[bad_b[0]])))
    raise AssertionError("%s: %s" % (what, "; ".join(msg)))


class _Arena:
    """store = [BAND sentinel][arena: LEAD + shift sentinel | payload | >= BAND sentinel]; subclasses provide the storage"""

    def __init__(self, nbytes, shift):
        self.nbytes, self.shift = int(nbytes), int(shift)
        assert 0 <= self.shift < LEAD
        self.start = BAND + LEAD + self.shift                          # of the payload, in the store
        self.total = (self.start + self.nbytes + BAND + 255) // 256 * 256
        self._allocate()
        assert self.arena_address % 256 == 0, "the arena is not 256-byte aligned"
        self.ptr = self.arena_address + LEAD + self.shift

    def check(self, what):
        front, back = self._bands()
        assert front.size >= BAND and back.size >= BAND
        check_bands(front, back, "%s (payload %d bytes at a 256-byte boundary + %d)" % (what, self.nbytes, self.shift))

    def read(self, dtype, shape=None):
        a = self._payload().view(dtype)
        return a if shape is None else a.reshape(shape)


class HostArena(_Arena):
    def _allocate(self):
        raw = np.full(self.total + 256, SENTINEL, np.uint8)
        off = (-raw.ctypes.data) % 256
        self.store = raw[off:off + self.total]
        self.arena_address = self.store.ctypes.data + BAND

    def write(self, a):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert b.size == self.nbytes
        self.store[self.start:self.start + self.nbytes] = b

    def _bands(self):
        return self.store[:self.start], self.store[self.start + self.nbytes:]

    def _payload(self):
        return self.store[self.start:self.start + self.nbytes].copy()


class DeviceArena(_Arena):
    def _allocate(self):
        import torch
        self.store = torch.full((self.total,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.arena = self.store[BAND:]
        self.arena_address = self.arena.data_ptr()

    def write(self, a):
        import torch
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert b.size == self.nbytes
        self.store[self.start:self.start + self.nbytes] = torch.from_numpy(b.copy()).cuda()

    def fill(self, byte):
        self.store[self.start:self.start + self.nbytes] = byte

    def _bands(self):
        import torch
        torch.cuda.synchronize()
        return self.store[:self.start].cpu().numpy(), self.store[self.start + self.nbytes:].cpu().numpy()

    def _payload(self):
        import torch
        torch.cuda.synchronize()
        return self.store[self.start:self.start + self.nbytes].cpu().numpy()


class Buffers:
    """The arenas of one call: b = Buffers(shifts); b.put(name, array) / b.out(name, nbytes) return device addresses; b.check(what)
    checks every band; b.get(name, dtype, shape) reads a payload back."""

    def __init__(self, shifts, arena=DeviceArena):
        self.shifts, self.arena, self.a = shifts, arena, {}

    def put(self, name, array):
        arr = np.ascontiguousarray(array)
        self.a[name] = self.arena(arr.nbytes, self.shifts[name])
        self.a[name].write(arr)
        return self.a[name].ptr

    def out(self, name, nbytes):
        """an output: its payload starts as sentinel too, so a voxel the call does not write shows"""
        self.a[name] = self.arena(nbytes, self.shifts[name])
        return self.a[name].ptr

    def check(self, what):
        for name, a in self.a.items():
            a.check("%s, buffer '%s'" % (what, name))

    def get(self, name, dtype, shape=None):
        return self.a[name].read(dtype, shape)
