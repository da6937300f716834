"""GPU: the contour select on grids that catch 32-bit arithmetic in k_dp_contour -- 645 x 645 x 646 records of 16 bytes (4.3 GB: byte
offsets past 2^32) and 1290 x 1290 x 1291 records of 8 bytes (2 148 353 100 voxels: drawn indices past 2^31).

The scene (built on the device in x chunks, no host copy) is the closed form of tests/contour_restated.py: solid boxes of SIZE^3 cells
on a lattice of PERIOD cells, clipped by the grid's far faces, each with its own id; free cells have id 0.  A box cell is drawn iff
along some axis it has an in-grid neighbour outside its box.  tests/test_contour_cpu.py pins lattice_contour_count, lattice_drawn
and lattice_key against by_neighbours on small replicas.  Here the total must equal the closed-form count, the indices must ascend
strictly, every one of them must be a drawn cell by the closed form (with the count, that makes the sets equal) and every key the id
of its box.  The tests skip when the device has too little free memory."""
import numpy as np
import pytest
import torch

import contour_restated as CR

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
ONE = 0x3F800000
PERIOD, SIZE = 40, 30
SLACK = 3 << 30


def test_the_cases_are_where_the_issue_puts_them():
    assert 645 * 645 * 646 * 16 > 2 ** 32 > 645 * 645 * 646
    assert 2 ** 31 < 1290 * 1290 * 1291 < 2 ** 32
    for shape in ((645, 645, 646), (1290, 1290, 1291)):
        assert all(0 < s % PERIOD < SIZE for s in shape)                    # the last box along every axis is clipped by the grid's face
    # the voxels past index 2^31 all lie in the last x plane, which a (clipped) box must reach
    assert 2 ** 31 // (1290 * 1291) == 1289 and 1289 % PERIOD < SIZE


@pytest.fixture(scope="module")
def big():
    from sdf_tools_amd import capi
    ctx = capi.SdfGpu(0)
    yield ctx
    ctx.close()
    torch.cuda.empty_cache()


def _need(nbytes):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip("needs %.1f GB of free device memory, %.1f GB are free" % (nbytes / 1e9, free / 1e9))


def _build(shape, words, occ_word, key_word, chunk=32):
    """int32 [nx, ny, nz, words]: the lattice scene's records; the other words hold a filler"""
    dev = torch.device("cuda", 0)
    nx, ny, nz = shape
    cells = torch.full(shape + (words,), 0x7B7B7B7B, dtype=torch.int32, device=dev)
    ax = [torch.arange(n, dtype=torch.int64, device=dev) for n in shape]
    cy, cz = -(-ny // PERIOD), -(-nz // PERIOD)
    iy, iz = (ax[1] % PERIOD < SIZE).view(1, -1, 1), (ax[2] % PERIOD < SIZE).view(1, 1, -1)
    by, bz = (ax[1] // PERIOD).view(1, -1, 1), (ax[2] // PERIOD).view(1, 1, -1)
    for xa in range(0, nx, chunk):
        x = ax[0][xa:xa + chunk].view(-1, 1, 1)
        inside = (x % PERIOD < SIZE) & iy & iz
        number = ((x // PERIOD) * cy + by) * cz + bz + 1
        cells[xa:xa + chunk, :, :, occ_word] = torch.where(inside, ONE, 0).to(torch.int32)
        cells[xa:xa + chunk, :, :, key_word] = torch.where(inside, number, 0).to(torch.int32)
    torch.cuda.synchronize()
    return cells


def _check(big, shape, words, occ_word, key_word):
    n = int(np.prod(shape))
    want = CR.lattice_contour_count(shape, PERIOD, SIZE)
    _need(n * words * 4 + n // 8 + want * 40 + SLACK)
    cells = _build(shape, words, occ_word, key_word)
    args = (cells.data_ptr(), shape, 3, words * 4, occ_word * 4, key_word * 4)
    total, _ = big.display_select_contour_device(*args)
    print("\n[contour-large] %s: total %d, expected %d" % (shape, total, want))
    assert total == want
    for reach in (1, 0):
        assert big.display_select_contour_device(cells.data_ptr(), shape, reach, *args[3:])[0] == (want if reach else 0)
    idx = torch.full((total + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    keys = torch.full((total + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    t, _ = big.display_select_contour_device(*args, d_indices=idx.data_ptr(), d_keys=keys.data_ptr(), capacity=total)
    assert t == total and int(idx[total]) == SENTINEL and int(keys[total]) == SENTINEL, "a word behind an output was written"
    got = idx[:total].to(torch.int64) & 0xFFFFFFFF
    assert bool((got[1:] > got[:-1]).all()), "the indices ascend strictly"
    assert int(got[-1]) < n
    assert bool(CR.lattice_drawn(shape, PERIOD, SIZE, got).all()), "every index is a drawn cell of the closed form"
    assert bool(((keys[:total].to(torch.int64) & 0xFFFFFFFF) == CR.lattice_key(shape, PERIOD, got)).all()), "keys"
    probe = torch.tensor([0, SIZE - 1, SIZE, shape[2] * (SIZE - 1) + 5], dtype=torch.int64, device=got.device)    # a grid corner, a z face, a free cell, a y face
    assert torch.isin(probe, got).tolist() == [False, True, False, True]
    past = int((got >= 2 ** 31).sum())
    del cells, idx, keys, got
    torch.cuda.empty_cache()
    return total, past


def test_records_past_4_gib(big):
    total, _ = _check(big, (645, 645, 646), 4, 0, 2)
    assert total > 10 ** 6


def test_drawn_indices_past_2_31(big):
    shape = (1290, 1290, 1291)
    total, past = _check(big, shape, 2, 0, 1)
    n = int(np.prod(shape))
    every = torch.arange(2 ** 31, n, dtype=torch.int64)
    assert past == int(CR.lattice_drawn(shape, PERIOD, SIZE, every).sum()) > 0
