"""Display export on record layouts other than "occupancy at 0, key at 4" (include/sdfgpu.h "Display export": every field a 4-byte
word at its offset, any stride that is a multiple of 4): strides that are no power of two, the occupancy behind the key, both
fields in one word, and the refusals of check_cell_layout.  The words of a record that are neither field come from
display_restated.filler_words: floats of every occupancy class and keys of the case's own pool, so a kernel that reads the wrong
word gives another answer.  Every result bit-equal to tests/display_restated.py, host and device forms, scan order and grouped.

cells_of itself is pinned without a GPU against records built by hand."""
import numpy as np
import pytest

import display_cases as C
import display_restated as R
from sdf_tools_amd import capi

gpu_test = pytest.mark.gpu
OCC, KEY = capi.DISPLAY_OCCUPANCY, capi.DISPLAY_KEY_FIELD
SHAPES = [(5, 6, 7), (3, 4, 65), (17, 16, 33)]
LAYOUTS = [(12, 0, 8), (12, 8, 0), (20, 16, 4), (24, 4, 20), (32, 28, 0), (16, 12, 8), (8, 4, 0)]      # (stride, occupancy offset, key offset)
POOL = np.array([0, 2 ** 31, 2 ** 32 - 1, 2 ** 32 - 2, 9, 0x3F800000], np.uint32)                       # (the last one: the bits of 1.0f)


# ---- cells_of, no GPU -----------------------------------------------------------------------------------------------------------
def _by_hand(occ, key, stride, occ_off, key_off, filler):
    """the records one byte string at a time"""
    out = bytearray()
    for i, (o, k) in enumerate(zip(occ.reshape(-1), key.reshape(-1))):
        rec = bytearray(np.asarray(filler.reshape(-1, stride // 4)[i], "<u4").tobytes())
        rec[occ_off:occ_off + 4] = np.float32(o).tobytes()
        rec[key_off:key_off + 4] = np.uint32(k).tobytes()
        out += rec
    return bytes(out)


def test_cells_of_places_the_fields_at_their_offsets():
    rng = np.random.default_rng(1)
    shape = (2, 3, 4)
    occ = rng.choice(C.OCC_VALUES, size=shape)
    key = rng.choice(POOL, size=shape)
    for stride, occ_off, key_off in LAYOUTS + [(8, 0, 4), (16, 0, 4)]:
        filler = R.filler_words(rng, shape, stride, POOL)
        cells = R.cells_of(occ, key, stride, key_off, occ_off, filler)
        assert cells.dtype == np.uint32 and cells.shape == shape + (stride // 4,) and cells.flags.c_contiguous
        assert cells.tobytes() == _by_hand(occ, key, stride, occ_off, key_off, filler)
        # a record array with the fields swapped, or the occupancy left at offset 0, is another byte string
        if occ_off != key_off:
            assert R.cells_of(occ, key, stride, occ_off, key_off, filler).tobytes() != cells.tobytes()
        # the default filler and the default offsets are the old records
        plain = R.cells_of(occ, key, stride, key_off, occ_off)
        others = [w for w in range(stride // 4) if w * 4 not in (occ_off, key_off)]
        assert (plain[..., others] == R.FILLER_WORD).all()
    old = R.cells_of(occ, key, 16)
    assert old.tobytes() == _by_hand(occ, key, 16, 0, 4, np.full(shape + (4,), R.FILLER_WORD, np.uint32))
    one = R.cells_of(occ, occ.view(np.uint32), 4, 0, 0)
    assert one.tobytes() == occ.tobytes()


def test_cells_of_check_notices_a_misplaced_field():
    rng = np.random.default_rng(2)
    shape = (2, 3, 4)
    occ = rng.choice(C.OCC_VALUES[:6], size=shape)
    key = rng.choice(POOL[1:5], size=shape)
    filler = R.filler_words(rng, shape, 12, POOL)
    cells = R.cells_of(occ, key, 12, 0, 8, filler)                  # key at 0, occupancy at 8
    assert cells.tobytes() == _by_hand(occ, key, 12, 8, 0, filler)
    for wrong in ((12, 0, 8), (12, 4, 0), (12, 8, 4)):              # (stride, occ_off, key_off): swapped, occupancy in the filler, key in it
        with pytest.raises(AssertionError):
            assert cells.tobytes() == _by_hand(occ, key, *wrong, filler)
    for bad in (dict(stride=6), dict(occupancy_offset=12), dict(key_offset=2)):
        with pytest.raises(AssertionError):
            R.cells_of(occ, key, **dict(dict(stride=12, key_offset=0, occupancy_offset=8), **bad))


def test_the_filler_holds_every_class_and_the_keys():
    rng = np.random.default_rng(3)
    f = R.filler_words(rng, (17, 16, 33), 20, POOL)
    assert f.shape == (17, 16, 33, 5) and f.dtype == np.uint32
    have = set(int(v) for v in np.unique(f))
    assert have == set(int(v) for v in POOL) | {0, 0x3F000000, 0x3F800000, 0x7FC00000, R.FILLER_WORD}
    assert sorted(set(R.occ_class(f.view(np.float32)).reshape(-1).tolist())) == [R.F, R.E, R.U, R.N]


# ---- the layouts on the GPU -----------------------------------------------------------------------------------------------------
def _case(shape, seed):
    rng = np.random.default_rng(seed)
    return rng, rng.choice(C.OCC_VALUES, size=shape), rng.choice(POOL, size=shape)


@gpu_test
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "stride%d_occ%d_key%d" % l)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_layout(gpu, shape, layout):
    rng, occ, keys = _case(shape, sum(shape) + sum(layout))

    def filler(stride):
        return R.filler_words(rng, shape, stride, POOL)
    # options that read both fields: the key rule with a class mask, the occupancy rule with the surface rule (which reads the
    # occupancy of the 26 neighbours, each at its own record)
    idx, _ = C.check(gpu, occ, keys, KEY, class_mask=5, draw_zero=False, layouts=[layout], filler=filler)
    assert 0 < len(idx) < occ.size
    C.check(gpu, occ, keys, KEY, class_mask=2, draw_keys=[0, 9, 2 ** 32 - 2], layouts=[layout], filler=filler)
    idx, _ = C.check(gpu, occ, keys, OCC, class_mask=7, surface_only=True, layouts=[layout], filler=filler)
    assert len(idx) > 0
    C.check(gpu, occ, keys, OCC, class_mask=6, layouts=[layout], filler=filler)


@gpu_test
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_one_word_records(gpu, shape):
    """stride 4: the record is the occupancy; under the key rule the same word is the key"""
    rng, occ, _ = _case(shape, sum(shape) + 4)
    as_keys = occ.view(np.uint32)                                   # (cells_of stores the key last: the one word must be the occupancy)
    assert R.cells_of(occ, as_keys, 4, 0, 0).tobytes() == occ.tobytes()
    idx, _ = C.check(gpu, occ, as_keys, OCC, class_mask=7, surface_only=True, layouts=[(4, 0, 0)])
    assert len(idx) > 0
    C.check(gpu, occ, as_keys, OCC, class_mask=5, layouts=[(4, 0, 0)])
    idx, k = C.check(gpu, occ, as_keys, KEY, class_mask=5, layouts=[(4, 0, 0)])
    assert len(np.unique(k)) >= 3 and 0 < len(idx) < occ.size       # (1.0, 0.75, 0.50000006 are F; 0.5 and NaN fall under U)
    C.check(gpu, occ, as_keys, KEY, class_mask=7, draw_zero=False, layouts=[(4, 0, 0)])
    C.check(gpu, occ, as_keys, KEY, class_mask=2, draw_keys=sorted(int(v) for v in np.unique(as_keys)[::2]), layouts=[(4, 0, 0)])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@gpu_test
def test_layout_refusals(gpu):
    shape = (2, 3, 4)
    n = 24
    d_cells = C.dev(np.zeros(n * 32, np.uint8))
    bad = [("stride 6", OCC, 6, 0, 0), ("stride 0", OCC, 0, 0, 0), ("occupancy_offset = stride", OCC, 12, 12, 0),
           ("occupancy_offset = 2", OCC, 12, 2, 4), ("occupancy_offset = 2, key rule", KEY, 12, 2, 4), ("key_offset = stride", KEY, 12, 0, 12),
           ("key_offset = 2", KEY, 12, 0, 2), ("stride 6, key rule", KEY, 6, 0, 0)]
    for what, rule, stride, occ_off, key_off in bad:
        for grouped in (False, True):
            idx, k, gk, go = C.words(n), C.words(n), C.words(n), C.words(n + 1)
            with pytest.raises(capi.SdfGpuError) as e:
                gpu.display_select_cells_device(d_cells.data_ptr(), shape, rule, stride, occ_off, key_off, grouped=grouped, d_indices=idx.data_ptr(),
                                                d_keys=k.data_ptr(), capacity=n, d_group_keys=gk.data_ptr(), d_group_offsets=go.data_ptr(),
                                                group_capacity=n)
            assert e.value.code == -1, what
            for t in (idx, k, gk, go):
                assert (t.cpu().numpy().view(np.uint32) == C.SENTINEL).all(), "%s: a refused call stored results" % what
        with pytest.raises(capi.SdfGpuError) as e:                  # the count-only form is refused as well
            gpu.display_select_cells_device(d_cells.data_ptr(), shape, rule, stride, occ_off, key_off)
        assert e.value.code == -1, what
        if stride:                                                  # the host form (its wrapper wants shape * stride bytes)
            with pytest.raises(capi.SdfGpuError) as e:
                gpu.display_select_cells(np.zeros(n * stride, np.uint8), shape, rule, stride, occ_off, key_off)
            assert e.value.code == -1, what


@gpu_test
def test_occupancy_rule_ignores_the_key_offset(gpu):
    """include/sdfgpu.h: under SDFGPU_DISPLAY_OCCUPANCY "key_offset is not used" -- one outside the record, or off its alignment, is
    accepted and changes nothing"""
    shape = (5, 6, 7)
    rng, occ, keys = _case(shape, 11)
    for stride, occ_off, key_at in ((12, 8, 0), (8, 0, 4), (4, 0, 0)):
        cells = R.cells_of(occ, keys if stride > 4 else occ.view(np.uint32), stride, key_at, occ_off, R.filler_words(rng, shape, stride, POOL))
        for grouped in (False, True):
            want = C.reference(occ, keys, OCC, grouped, class_mask=7, surface_only=True)
            for key_off in (stride, stride + 4, 2, 1 << 40):
                for run in (C.run_host, C.run_device):
                    got = run(gpu, cells, shape, OCC, stride, grouped, offsets=(occ_off, key_off), class_mask=7, surface_only=True)
                    C.same("occupancy rule, %d-byte records, key_offset %d" % (stride, key_off), got, want)
