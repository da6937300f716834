"""GPU: sdfgpu_resample_cells_device past the 32-bit limits, 4-byte cells, identity origin.

(a) a source of 2064 x 1448 x 1440 = 4 303 656 960 cells (more than 2^32: the 64-bit winner words, source indices and byte offsets
    past 2^32, a launch over two grid dimensions), resolution 1 -> 8: the result is 258 x 181 x 180 and cell (X, Y, Z) holds source
    (8X + 7, 8Y + 7, 8Z + 7), the last of its 512 in scan order.
(b) a result of 1620 x 1280 x 1040 = 2 156 544 000 cells (more than 2^31), from 162 x 128 x 104 at resolution 1 -> 0.1: written
    exactly where all three indices are 5 mod 10, by source (X // 10, Y // 10, Z // 10), the fill record elsewhere; the count is
    162 * 128 * 104.

The payload of source cell `lin` is (lin * 2654435761 + 1) mod 2^32.  Both closed forms are evaluated by torch in x chunks and are
first pinned on small grids, without a GPU, against the restatement (tests/resample_restated.cpp), where a corrupted result must
make them raise.  The GPU tests skip when the device has too little free memory."""
import math

import numpy as np
import pytest
import torch

import resample_restated as R

gpu_test = pytest.mark.gpu
FILL = 0x7FDEAD01


def _payload(lin):
    """int64 tensor of linear indices -> the 4-byte payload as int32 bit patterns (the product wraps modulo 2^64, which keeps its
    low 32 bits)"""
    v = (lin * 2654435761 + 1) & 0xFFFFFFFF
    return torch.where(v >= (1 << 31), v - (1 << 32), v).to(torch.int32)


def _axis(a, b, device):
    return torch.arange(a, b, dtype=torch.int64, device=device)


def _coarse_expected(shape, f, x0, x1, device):
    """result planes [x0, x1) of a source `shape` (multiples of f) coarsened by the integer factor f"""
    nx, ny, nz = shape
    x, y, z = _axis(x0, x1, device) * f + f - 1, _axis(0, ny // f, device) * f + f - 1, _axis(0, nz // f, device) * f + f - 1
    return _payload((x.view(-1, 1, 1) * ny + y.view(1, -1, 1)) * nz + z.view(1, 1, -1))


def _fine_expected(shape, f, x0, x1, device):
    """result planes [x0, x1) of a source `shape` refined by the integer factor f (even: the centres fall on index f / 2 mod f)"""
    nx, ny, nz = shape
    out = torch.full((x1 - x0, ny * f, nz * f), FILL - (1 << 32) if FILL >= (1 << 31) else FILL, dtype=torch.int32, device=device)
    xs = [x for x in range(x0, x1) if x % f == f // 2]
    if xs:
        x = torch.tensor([v // f for v in xs], dtype=torch.int64, device=device)
        y, z = _axis(0, ny, device), _axis(0, nz, device)
        rows = torch.tensor([v - x0 for v in xs], dtype=torch.int64, device=device)
        sub = out[rows]
        sub[:, f // 2::f, f // 2::f] = _payload((x.view(-1, 1, 1) * ny + y.view(1, -1, 1)) * nz + z.view(1, 1, -1))
        out[rows] = sub
    return out


def _check_chunks(name, got, expected, chunk):
    """got: int32 device tensor [mx, my, mz]; expected(x0, x1) -> int32 tensor of those planes"""
    for x0 in range(0, got.shape[0], chunk):
        x1 = min(got.shape[0], x0 + chunk)
        a, b = got[x0:x1], expected(x0, x1)
        if not bool(torch.equal(a, b)):
            bad = (a != b).nonzero()[:3].tolist()
            raise AssertionError("%s: planes %d..%d: %d cells differ, first %s" % (
                name, x0, x1, int((a != b).sum()), [[v[0] + x0] + v[1:] for v in bad]))


def _source_cpu(shape):
    n = int(np.prod(shape))
    return _payload(torch.arange(n, dtype=torch.int64)).numpy().view(np.uint8).reshape(tuple(shape) + (4,))


def _fill_bytes():
    return np.array([FILL], np.uint32).view(np.uint8)


# ---- the closed forms against the restatement, no GPU ---------------------------------------------------------------------------
def test_coarse_closed_form_is_the_restatement():
    shape, f = (16, 24, 8), 8
    res = R.restated(_source_cpu(shape), 1.0, np.eye(4), 8.0, _fill_bytes())
    assert res.shape == (2, 3, 1) and res.written == 6
    got = torch.from_numpy(res.cells.view(np.int32).reshape(res.shape).copy())
    _check_chunks("coarse", got, lambda a, b: _coarse_expected(shape, f, a, b, "cpu"), 1)
    got[1, 2, 0] ^= 4
    with pytest.raises(AssertionError):
        _check_chunks("coarse", got, lambda a, b: _coarse_expected(shape, f, a, b, "cpu"), 1)


def test_fine_closed_form_is_the_restatement():
    shape, f = (3, 4, 2), 10
    res = R.restated(_source_cpu(shape), 1.0, np.eye(4), 0.1, _fill_bytes())
    assert res.shape == (30, 40, 20) and res.written == 24
    got = torch.from_numpy(res.cells.view(np.int32).reshape(res.shape).copy())
    _check_chunks("fine", got, lambda a, b: _fine_expected(shape, f, a, b, "cpu"), 7)
    for at in ((15, 25, 5), (15, 25, 6)):                          # (a written cell, a hole)
        bad = got.clone()
        bad[at] ^= 1
        with pytest.raises(AssertionError):
            _check_chunks("fine", bad, lambda a, b: _fine_expected(shape, f, a, b, "cpu"), 7)


def test_the_large_results_have_the_stated_sizes():
    """VoxelGrid's ceil(size / resolution) for the two large cases, in the doubles the constructor uses"""
    assert [int(math.ceil(n * 1.0 / 8.0)) for n in (2064, 1448, 1440)] == [258, 181, 180]
    assert [int(math.ceil(n * 1.0 / 0.1)) for n in (162, 128, 104)] == [1620, 1280, 1040]
    assert 1.0 / 0.1 == 10.0


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """A context of its own: its winner words go when the module ends."""
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


@gpu_test
def test_source_past_2_32_cells(big):
    shape, f = (2064, 1448, 1440), 8
    n = math.prod(shape)
    assert n > 2 ** 32
    rshape = tuple(s // f for s in shape)
    _need(n * 4 + math.prod(rshape) * 12 + (3 << 30))
    dev = torch.device("cuda", 0)
    src = torch.empty(shape, dtype=torch.int32, device=dev)
    y, z = _axis(0, shape[1], dev), _axis(0, shape[2], dev)
    for x0 in range(0, shape[0], 16):
        x = _axis(x0, min(shape[0], x0 + 16), dev)
        src[x0:x0 + 16] = _payload((x.view(-1, 1, 1) * shape[1] + y.view(1, -1, 1)) * shape[2] + z.view(1, 1, -1))
    dst = torch.full(rshape, 0x5A5A5A5A, dtype=torch.int32, device=dev)
    written = big.resample_cells_device(src.data_ptr(), shape, 1.0, np.eye(4), np.eye(4), 1.0 / 8.0, dst.data_ptr(), rshape, _fill_bytes(), 4,
                                        count=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert written == math.prod(rshape)
    _check_chunks("source past 2^32 cells", dst, lambda a, b: _coarse_expected(shape, f, a, b, dev), 64)


@gpu_test
def test_result_past_2_31_cells(big):
    shape, f = (162, 128, 104), 10
    rshape = tuple(s * f for s in shape)
    n = math.prod(rshape)
    assert n > 2 ** 31
    _need(n * 8 + (3 << 30))                                       # the result, its winner words, the check's chunks
    dev = torch.device("cuda", 0)
    src = _payload(torch.arange(math.prod(shape), dtype=torch.int64, device=dev)).view(shape)
    dst = torch.full(rshape, 0x5A5A5A5A, dtype=torch.int32, device=dev)
    written = big.resample_cells_device(src.data_ptr(), shape, 1.0, np.eye(4), np.eye(4), 1.0 / 0.1, dst.data_ptr(), rshape, _fill_bytes(), 4,
                                        count=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert written == 162 * 128 * 104
    _check_chunks("result past 2^31 cells", dst, lambda a, b: _fine_expected(shape, f, a, b, dev), 20)
