"""GPU: Resample through the C ABI (host and device form), both grid classes and pysdf_tools, every byte of every result cell
against the restatement (tests/resample_restated.cpp, pinned by tests/test_resample_cpu.py).

Shapes: 1 x 1 x 1, a line, small odd boxes, a 2-D grid, 40^3 and 64 x 48 x 65 (several workgroups, the last one ragged).  Ratios
new / old resolution: 2, 3, 4, 1.5, 7/3, 0.75, 0.5, 1.0 and one above the grid's size (and 0.25 under the quarter turn).  Origins:
identity, a translation, a quarter turn about z built from a quaternion and a general rotation with a translation.  Under a
rotation the result's own inverse transform undoes the origin only up to rounding, and at ratios 0.5 and 0.25 every source
centre sits exactly on a result cell boundary: which side it falls on is decided by that noise alone, so these cases pass only
when the device rounds every product and sum as the host does.  The cell size 0.05 is not a binary fraction.
Payloads (resample_restated.payload): the index word holds linear index + 1, so the winner is visible; occupancies include 0.5,
-0.0, a quiet and a signalling NaN with payloads; 16-byte records carry distinct object ids and segments; the fill record has a
bit pattern of its own."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import resample_restated as R
from sdf_tools_amd import capi
from sdf_tools_amd._bindings import load_pysdf_tools

pytestmark = pytest.mark.gpu
m = load_pysdf_tools()

CELL = 0.05
SHAPES = [(1, 1, 1), (1, 1, 37), (13, 7, 5), (33, 1, 20), (40, 40, 40), (64, 48, 65)]
RATIOS = [2.0, 3.0, 4.0, 1.5, 7.0 / 3.0, 0.75, 0.5, 1.0, "above"]
ORIGINS = R.origins()
INVALID = -1


def _resolution(shape, ratio):
    return CELL * (max(shape) + 3) if ratio == "above" else CELL * ratio


@functools.lru_cache(maxsize=None)
def _source(shape, cb):
    return R.payload(shape, cb, seed=sum(shape) + cb)


@functools.lru_cache(maxsize=None)
def _want(shape, cb, origin, ratio):
    return R.restated(_source(shape, cb), CELL, ORIGINS[origin], _resolution(shape, ratio), R.oob_record(cb))


def _same(what, got, want):
    got, want = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1))
        raise AssertionError("%s: %d of %d result cells differ, first at %s: got %s, want %s" % (
            what, len(bad), got[..., 0].size, bad[0].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist()))


def _host(ctx, shape, cb, origin, want):
    return ctx.resample_cells(_source(shape, cb), shape, CELL, ORIGINS[origin], want.inverse, want.inv_cell, want.shape,
                              R.oob_record(cb), cb)


def _device(ctx, shape, cb, origin, want, offset=0, count=True):
    """the device form on torch buffers; offset: bytes by which the SOURCE pointer is moved off its 256-byte alignment"""
    src = _source(shape, cb).reshape(-1)
    d_src = torch.zeros(src.size + 64, dtype=torch.uint8, device="cuda")
    d_src[offset:offset + src.size] = torch.from_numpy(src).cuda()
    n_dst = int(np.prod(want.shape)) * cb
    d_dst = torch.full((n_dst + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    written = ctx.resample_cells_device(d_src.data_ptr() + offset, shape, CELL, ORIGINS[origin], want.inverse, want.inv_cell,
                                        d_dst.data_ptr(), want.shape, R.oob_record(cb), cb, count=count,
                                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy()
    assert bool((out[n_dst:] == 0xA5).all()), "bytes behind the result were written"
    return out[:n_dst].reshape(want.shape + (cb,)), written


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", list(ORIGINS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_form_every_ratio_and_record_size(gpu, shape, origin):
    for ratio in RATIOS:
        for cb in (4, 8, 16):
            want = _want(shape, cb, origin, ratio)
            got, written = _host(gpu, shape, cb, origin, want)
            what = "host form %s %s x %s %d-byte" % (shape, origin, ratio, cb)
            _same(what, got, want.cells)
            assert written == want.written, (what, written, want.written)


@pytest.mark.parametrize("origin", list(ORIGINS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_form_every_ratio(gpu, shape, origin):
    for i, ratio in enumerate(RATIOS):
        cb = (4, 8, 16)[i % 3] if shape != (64, 48, 65) else (16, 4, 8)[i % 3]
        want = _want(shape, cb, origin, ratio)
        got, written = _device(gpu, shape, cb, origin, want)
        what = "device form %s %s x %s %d-byte" % (shape, origin, ratio, cb)
        _same(what, got, want.cells)
        assert written == want.written, (what, written, want.written)


@pytest.mark.parametrize("shape", [(13, 7, 5), (33, 1, 20), (40, 40, 40)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("origin", ["quarter-turn", "general"])
def test_centres_on_cell_boundaries_under_a_rotation(gpu, shape, origin):
    """ratios 0.5 and 0.25: p * (1 / new_resolution) of every source centre is an integer up to the noise of the two transforms"""
    for ratio, cb in ((0.5, 8), (0.5, 16), (0.25, 8), (0.25, 4)):
        want = _want(shape, cb, origin, ratio)
        got, written = _host(gpu, shape, cb, origin, want)
        _same("host form %s %s x %s" % (shape, origin, ratio), got, want.cells)
        assert written == want.written
        got, written = _device(gpu, shape, cb, origin, want)
        _same("device form %s %s x %s" % (shape, origin, ratio), got, want.cells)
        assert written == want.written


def test_the_quarter_turn_is_decided_by_rounding_noise():
    """what makes the case above a test: under the quarter turn at ratio 0.5 the restatement does NOT write the cells the exact
    arithmetic would (all indices odd), so an implementation that rounds differently lands elsewhere"""
    shape, cb = (13, 7, 5), 8
    want = _want(shape, cb, "quarter-turn", 0.5)
    exact = _want(shape, cb, "identity", 0.5)
    assert want.shape == exact.shape
    assert not np.array_equal(want.cells, exact.cells)


@pytest.mark.parametrize("cb,offset", [(8, 4), (16, 4), (16, 8), (4, 4), (16, 12)])
def test_device_source_off_its_alignment(gpu, cb, offset):
    """a source pointer that is only 4-byte (or 8-byte) aligned: the gather falls back to narrower accesses"""
    shape, origin = (13, 7, 5), "general"
    for ratio in (2.0, 0.75):
        want = _want(shape, cb, origin, ratio)
        got, written = _device(gpu, shape, cb, origin, want, offset=offset)
        _same("device form, source + %d bytes, %d-byte records, x %s" % (offset, cb, ratio), got, want.cells)
        assert written == want.written


def test_device_form_without_the_count_returns_none(gpu):
    want = _want((13, 7, 5), 8, "translation", 3.0)
    got, written = _device(gpu, (13, 7, 5), 8, "translation", want, count=False)
    assert written is None
    _same("device form, no count", got, want.cells)


def test_under_red_zones(monkeypatch):
    """SDFGPU_REDZONE=1 in the environment of sdfgpu_create: the winner words, the counter and the staging buffers carry canaries
    and every call ends with their check"""
    monkeypatch.setenv("SDFGPU_REDZONE", "1")
    ctx = capi.SdfGpu(0)
    try:
        for shape, cb, origin, ratio in [((64, 48, 65), 16, "general", 2.0), ((13, 7, 5), 8, "quarter-turn", 0.5), ((1, 1, 37), 4, "identity", 3.0),
                                         ((33, 1, 20), 8, "translation", 7.0 / 3.0), ((1, 1, 1), 16, "identity", 1.0)]:
            want = _want(shape, cb, origin, ratio)
            got, written = _host(ctx, shape, cb, origin, want)
            _same("red zones, host form %s" % (shape,), got, want.cells)
            got, written = _device(ctx, shape, cb, origin, want)
            _same("red zones, device form %s" % (shape,), got, want.cells)
            assert written == want.written
        ctx.redzone_check()
    finally:
        ctx.close()


def test_argument_errors_leave_the_output_alone(gpu):
    shape, cb = (4, 3, 2), 8
    src = _source(shape, cb).copy()
    want = _want(shape, cb, "identity", 2.0)
    d3, d16 = ctypes.c_double * 3, ctypes.c_double * 16
    cell, inv_cell = d3(CELL, CELL, CELL), d3(*want.inv_cell)
    origin, inverse = d16(*np.eye(4).reshape(-1)), d16(*want.inverse.reshape(-1))
    fill = R.oob_record(cb)
    out = np.full(want.shape + (cb,), 0xA5, np.uint8)
    d_src, d_out = torch.from_numpy(src.reshape(-1)).cuda(), torch.full((out.size,), 0xA5, dtype=torch.uint8, device="cuda")
    L, h = gpu._lib, gpu._h

    def host(src_p=src.ctypes.data, bytes_=cb, dims=shape, cell_=cell, origin_=origin, inverse_=inverse, inv_=inv_cell, dst_p=out.ctypes.data,
             rdims=want.shape, fill_=fill.ctypes.data):
        return L.sdfgpu_resample_cells(h, src_p, bytes_, *dims, cell_, origin_, inverse_, inv_, dst_p, *rdims, fill_, None)

    def device(src_p=d_src.data_ptr(), bytes_=cb, dims=shape, cell_=cell, origin_=origin, inverse_=inverse, inv_=inv_cell,
               dst_p=d_out.data_ptr(), rdims=want.shape, fill_=fill.ctypes.data):
        return L.sdfgpu_resample_cells_device(h, src_p, bytes_, *dims, cell_, origin_, inverse_, inv_, dst_p, *rdims, fill_, None, None)

    for form in (host, device):
        bad = [dict(bytes_=0), dict(bytes_=12), dict(bytes_=32), dict(dims=(0, 3, 2)), dict(dims=(4, -1, 2)), dict(dims=(4, 3, 0)),
               dict(rdims=(0, 2, 1)), dict(rdims=(2, 2, -5)), dict(src_p=None), dict(dst_p=None), dict(cell_=None), dict(origin_=None),
               dict(inverse_=None), dict(inv_=None), dict(fill_=None)]
        bad.append(dict(dst_p=src.ctypes.data) if form is host else dict(dst_p=d_src.data_ptr()))
        if form is device:
            bad += [dict(src_p=d_src.data_ptr() + 2), dict(dst_p=d_out.data_ptr() + 1)]
        for kw in bad:
            assert form(**kw) == INVALID, kw
            assert L.sdfgpu_last_error(h).decode() != "", kw
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all()) and bool((d_out == 0xA5).all()), "a refused call wrote its output"
        assert np.array_equal(src, _source(shape, cb)) and np.array_equal(d_src.cpu().numpy(), src.reshape(-1))
        assert L.sdfgpu_resample_cells(None, None, 0, 0, 0, 0, *([None] * 5), 0, 0, 0, None, None) == INVALID
    assert host() == 0 and device() == 0
    torch.cuda.synchronize()
    _same("after the refusals, host form", out, want.cells)
    _same("after the refusals, device form", d_out.cpu().numpy().reshape(out.shape), want.cells)


# ---- the classes, through pysdf_tools -----------------------------------------------------------------------------------------------
OOB8 = np.array([np.float32(0.7).view(np.uint32), 0xFEEDF00D], np.uint32).view(np.uint8)
OOB16 = np.array([np.float32(0.7).view(np.uint32), 0xFEEDF00D, 0xCAFEBABE, 0x0BADC0DE], np.uint32).view(np.uint8)


def _grid(cb, shape, origin, frame):
    if cb == 8:
        g = m.CollisionMapGrid(m.Isometry3d(ORIGINS[origin]), frame, CELL, *shape, m.COLLISION_CELL(0.7, 0xFEEDF00D))
    else:
        g = m.TaggedObjectCollisionMapGrid(m.Isometry3d(ORIGINS[origin]), frame, CELL, *shape,
                                           m.TAGGED_OBJECT_COLLISION_CELL(0.7, 0xCAFEBABE, 0xFEEDF00D, 0x0BADC0DE))
    g.SetRawCellsNumpy(_source(shape, cb))
    return g


@pytest.mark.parametrize("origin", list(ORIGINS))
@pytest.mark.parametrize("cb", [8, 16], ids=["CollisionMapGrid", "TaggedObjectCollisionMapGrid"])
def test_classes_resample(cb, origin):
    oob = OOB8 if cb == 8 else OOB16
    for shape in SHAPES:
        g = _grid(cb, shape, origin, "frame of %s" % (shape,))
        assert np.array_equal(g.GetRawCellsNumpy(), _source(shape, cb))
        if shape == (13, 7, 5):
            g.UpdateConnectedComponents()                       # (valid components on the source do not carry over)
            g_cells = g.GetRawCellsNumpy()
        else:
            g_cells = _source(shape, cb)
        for ratio in RATIOS if shape != (64, 48, 65) else (2.0, 7.0 / 3.0, 0.5):
            want = R.restated(g_cells, CELL, ORIGINS[origin], _resolution(shape, ratio), oob)
            r = g.Resample(_resolution(shape, ratio))
            what = "%s %s x %s" % (type(g).__name__, shape, ratio)
            assert (r.GetNumXCells(), r.GetNumYCells(), r.GetNumZCells()) == want.shape, what
            _same(what, r.GetRawCellsNumpy(), want.cells)
            assert r.GetFrame() == g.GetFrame() and r.GetResolution() == _resolution(shape, ratio), what
            assert r.GetNumConnectedComponents() == (0, False), what
            if cb == 16:
                assert r.GetNumConvexSegments() == (0, False) and not r.AreConvexSegmentsValid(), what
            # outside the result: the source's OOB record
            cell, inside = r.GetValueByIndex(-1, 0, 0)
            assert not inside and np.float32(cell.occupancy) == np.float32(0.7) and cell.component == 0xFEEDF00D, what
        assert np.array_equal(g.GetRawCellsNumpy(), g_cells), "Resample changed its source"


@pytest.mark.parametrize("cb", [8, 16], ids=["CollisionMapGrid", "TaggedObjectCollisionMapGrid"])
@pytest.mark.parametrize("bad", [0.0, -0.05, float("nan"), float("inf")])
def test_classes_refuse_a_bad_resolution(cb, bad):
    g = _grid(cb, (3, 2, 2), "identity", "f")
    with pytest.raises(ValueError):
        g.Resample(bad)
