"""CPU: the band check of alignment_harness.py on numpy arenas -- the same checking function the GPU tests call -- and the case
table of alignment_cases.py."""
import numpy as np
import pytest

import alignment_cases as C
import alignment_harness as H


@pytest.mark.parametrize("shift", sorted({s for row in C.SHIFTS.values() for s in row}))
def test_an_intact_arena_passes_and_the_payload_sits_at_the_shift(shift):
    payload = np.arange(1000, dtype=np.uint8)
    a = H.HostArena(payload.size, shift)
    assert a.arena_address % 256 == 0 and a.ptr == a.arena_address + C.LEAD + shift
    assert a.ptr - a.store.ctypes.data >= C.BAND and a.store.size - (a.start + a.nbytes) >= C.BAND
    a.write(payload)
    a.check("intact")
    assert np.array_equal(a.read(np.uint8), payload)
    assert a.store.ctypes.data + a.start == a.ptr                   # the payload is read back from the address the library got


@pytest.mark.parametrize("where,offset,words", [("front", -1, "IN FRONT of the buffer changed, the nearest 1 byte(s) before"),
                                                ("back", 0, "BEHIND the buffer changed, the nearest 1 byte(s) past"),
                                                ("far-front", -(C.BAND + C.LEAD), "the nearest %d byte(s) before" % (C.BAND + C.LEAD)),
                                                ("far-back", C.BAND - 1, "the nearest %d byte(s) past" % C.BAND)])
def test_one_changed_byte_next_to_the_buffer_is_reported(where, offset, words):
    a = H.HostArena(1000, 4)
    a.write(np.zeros(1000, np.uint8))
    at = a.start + (offset if offset < 0 else a.nbytes + offset)
    a.store[at] ^= 0x01                                              # one bit of one byte
    with pytest.raises(AssertionError) as e:
        a.check("one byte")
    assert "1 byte(s) " in str(e.value) and words in str(e.value)
    assert ("IN FRONT" in str(e.value)) == (offset < 0) and ("BEHIND" in str(e.value)) == (offset >= 0)
    a.store[at] ^= 0x01
    a.check("restored")


def test_a_payload_that_holds_the_sentinel_is_no_excuse():
    """the bands are told from the payload by position, not by value"""
    b = H.Buffers({"x": 3, "y": 0}, arena=H.HostArena)
    b.put("x", np.full(64, C.SENTINEL, np.uint8))
    b.out("y", 32)
    b.check("both intact")
    b.a["x"].store[b.a["x"].start + 64] = 0
    with pytest.raises(AssertionError, match="buffer 'x'.*BEHIND"):
        b.check("x overrun")


def test_the_case_table_is_complete():
    for entry, ptrs in C.POINTERS.items():
        for name, (kind, widest, predicate, narrow) in ptrs.items():
            assert kind in C.SHIFTS and widest in (1, 4, 8, 16)
            # an access wider than the pointer's own type has a predicate in front of it and a narrow arm behind it
            element = {"bytes": 1, "doubles": 8}.get(kind, 4)
            if widest > element:
                assert not predicate.startswith("none") and narrow != "-", (entry, name)
        labels = [label for label, _ in C.moves(entry)]
        assert labels[0] == "control" and labels[-1] == "all-off" and len(set(labels)) == len(labels)
        for label, shifts in C.moves(entry)[1:-1]:
            assert sum(1 for s in shifts.values() if s) == 1, (entry, label)     # one pointer at a time
    assert all(0 in row for row in C.SHIFTS.values())
    assert list(C.SHAPES) == sorted(C.SHAPES, key=lambda s: s[2])                # scalar shapes first, the widest rows last
