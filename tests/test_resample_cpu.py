"""Resample without a GPU: the restatement (tests/resample_restated.cpp: the contract's loop over VoxelGrid's public members) pinned
to hand-derived answers.  It is the yardstick of the GPU kernels (tests/test_gpu_resample.py compares the two byte for byte).

Identity origin, cell size 0.25 (every product below is exact in binary), payload = linear index + 1 in the record's index word,
so the source cell that a result cell holds can be read off.  Each check is also run on a corrupted result and must raise."""
import math

import numpy as np
import pytest

import resample_restated as R

CELL = 0.25
SIZES = [4, 8, 16]


def _index_word(cells):
    """the word that holds linear index + 1: word 0 of a 4-byte record, word 1 of the others"""
    w = np.ascontiguousarray(cells).view(np.uint32)
    return w[..., 0 if w.shape[-1] == 1 else 1].astype(np.int64)


def _run(shape, ratio, cb):
    src = R.payload(shape, cb, seed=3)
    return src, R.restated(src, CELL, np.eye(4), CELL * ratio, R.oob_record(cb))


def _source_of(shape, per_axis):
    """linear index + 1 of the source cell whose per-axis indices are given (broadcast over the result)"""
    x, y, z = np.meshgrid(*per_axis, indexing="ij")
    return (x * shape[1] + y) * shape[2] + z + 1


def _holds_whole_records(src, res, want_index):
    """every result record equals, in all its bytes, the source record with that linear index + 1"""
    got = _index_word(res.cells)
    assert np.array_equal(got, want_index), "result cells hold other source cells than the contract names"
    flat = src.reshape(-1, src.shape[-1])
    assert np.array_equal(res.cells.reshape(-1, src.shape[-1]), flat[want_index.reshape(-1) - 1]), "a record was not copied whole"


def _corrupted(res, where=None):
    cells = res.cells.copy()
    i = tuple(s // 2 for s in res.shape) if where is None else where
    cells[i + (cells.shape[-1] - 1,)] ^= 0x40
    cells[i + (4 if cells.shape[-1] > 4 else 0,)] ^= 0x01              # (the index word)
    return res._replace(cells=cells)


def _raises_on_corruption(check, res, where=None):
    check(res)
    with pytest.raises(AssertionError):
        check(_corrupted(res, where))


@pytest.mark.parametrize("cb", SIZES)
def test_factor_two_keeps_the_last_cell_of_each_block(cb):
    """8^3 at x 2: result (X, Y, Z) holds source (2X + 1, 2Y + 1, 2Z + 1), the last of its eight in scan order"""
    src, res = _run((8, 8, 8), 2.0, cb)

    def check(r):
        assert r.shape == (4, 4, 4) and r.written == 64
        a = 2 * np.arange(4) + 1
        _holds_whole_records(src, r, _source_of((8, 8, 8), (a, a, a)))
    _raises_on_corruption(check, res)


@pytest.mark.parametrize("cb", SIZES)
def test_ragged_factor_three(cb):
    """7 x 5 x 3 at x 3: the result is 3 x 2 x 1 (ceil); a result cell holds source min(3 I + 2, n - 1) per axis, so the last cell
    along x holds source x = 6"""
    shape = (7, 5, 3)
    src, res = _run(shape, 3.0, cb)

    def check(r):
        assert r.shape == (3, 2, 1) and r.written == 6
        per_axis = [np.minimum(3 * np.arange(m) + 2, n - 1) for m, n in zip(r.shape, shape)]
        assert per_axis[0][-1] == 6
        _holds_whole_records(src, r, _source_of(shape, per_axis))
        assert np.all((_index_word(r.cells)[2] - 1) // (5 * 3) == 6)
    _raises_on_corruption(check, res, (2, 1, 0))


@pytest.mark.parametrize("cb", SIZES)
def test_refining_leaves_holes(cb):
    """4^3 at x 0.5: the result is 8^3; source centre i + 0.5 lands in result cell 2 i + 1, so exactly the cells whose three indices
    are odd are written, by source (X // 2, Y // 2, Z // 2); every other cell holds the OOB record's bits"""
    shape = (4, 4, 4)
    src, res = _run(shape, 0.5, cb)
    oob = R.oob_record(cb)

    def check(r):
        assert r.shape == (8, 8, 8) and r.written == 64
        odd = np.arange(8) % 2 == 1
        written = odd[:, None, None] & odd[None, :, None] & odd[None, None, :]
        assert np.array_equal(r.cells[~written], np.broadcast_to(oob, (int((~written).sum()), cb))), "a hole does not hold the OOB record"
        a = np.arange(8) // 2
        want = _source_of(shape, (a, a, a))
        flat = src.reshape(-1, cb)
        assert np.array_equal(r.cells[written], flat[want[written] - 1])
    _raises_on_corruption(check, res, (3, 5, 1))
    with pytest.raises(AssertionError):
        check(_corrupted(res, (2, 5, 1)))                          # (a hole)


@pytest.mark.parametrize("cb", SIZES)
@pytest.mark.parametrize("shape,ratio", [((5, 4, 3), 40.0), ((4, 4, 4), 4.0), ((1, 1, 1), 1.5)])
def test_one_result_cell_holds_the_last_source_cell(cb, shape, ratio):
    """new_resolution at or above the grid's size: 1 x 1 x 1 holding the last source cell"""
    src, res = _run(shape, ratio, cb)

    def check(r):
        assert r.shape == (1, 1, 1) and r.written == 1
        assert np.array_equal(r.cells.reshape(-1), src.reshape(-1, cb)[-1])
    _raises_on_corruption(check, res)


@pytest.mark.parametrize("cb", SIZES)
def test_same_resolution_is_a_copy(cb):
    shape = (6, 3, 5)
    src, res = _run(shape, 1.0, cb)

    def check(r):
        assert r.shape == shape and r.written == 90
        assert np.array_equal(r.cells, src)
    _raises_on_corruption(check, res)


def test_result_geometry_is_the_grids_own():
    """the inverse transform and 1 / cell that the restatement reports are those of a grid built by the metric-size constructor"""
    origin = R.origins()["general"]
    src = R.payload((3, 4, 5), 8)
    res = R.restated(src, CELL, origin, 0.1, R.oob_record(8))
    assert res.shape == (math.ceil(0.75 / 0.1), math.ceil(1.0 / 0.1), math.ceil(1.25 / 0.1))
    assert np.array_equal(res.inv_cell, np.full(3, 1.0 / 0.1))
    assert np.allclose(res.inverse @ origin, np.eye(4), atol=1e-15)
    assert np.array_equal(res.inverse[3], [0.0, 0.0, 0.0, 1.0])


@pytest.mark.parametrize("bad", [0.0, -0.25, math.nan, math.inf, -math.inf])
def test_bad_resolution_throws(bad):
    with pytest.raises(ValueError):
        R.restated(R.payload((2, 2, 2), 8), CELL, np.eye(4), bad, R.oob_record(8))
