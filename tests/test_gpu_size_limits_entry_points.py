"""GPU: the entry points and tiers of include/sdfgpu.h that test_gpu_size_limits.py leaves out, at linear voxel indices past 2^31
and byte or element offsets past 2^32.

* the marching sweeps on a far-field scene at 3072 x 1024 x 1024 (boxes and single voxels in free space, and the inverse);
* bits in (sdfgpu_build_bits_device), nz a multiple of 32 and not;
* cells in (sdfgpu_classify_cells_device, sdfgpu_build_cells_device), 8- and 16-byte records;
* voxelisation into the byte mask and into the bit field, clear_first on and off;
* the full-field gradient, float32 (vector and scalar kernel) and float64;
* point queries (sdfgpu_query_points_device, sdfgpu_query_points) on 1300 x 1300 x 1272;
* one host-to-host build (sdfgpu_build_bits: 384 MiB in, 12 GiB out).

Every expectation is a closed form evaluated by torch on the device in int64 (or the restatements of tests/analysis_scenes.py), in
x chunks, and every closed form is first pinned on the CPU -- the tests without the gpu marker below -- against the oracle or
the restatement it stands for, on small grids, where a corrupted field must make it raise.  All comparisons are bit for bit."""
import math
import time

import numpy as np
import pytest

import analysis_scenes as A
from oracle import oracle as O
from sdf_tools_amd import capi, synth
from test_gpu_size_limits import (BIG, STRIDES, _Extrema, _expected_chunk, _finish_table, _lattice_check, _lattice_mask,
                                  _sites_reference, _used_device_bytes, _vb_sq)

gpu_test = pytest.mark.gpu


@pytest.fixture(scope="module")
def big():
    """A context of its own for the largest grids: its scratch fields go when the module ends."""
    import torch
    ctx = capi.SdfGpu(0)
    ctx.set_option("dense_retry", 0)
    yield ctx
    ctx.close()
    torch.cuda.empty_cache()


def _device():
    import torch
    return torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream


def _line(what, shape, times, peak):
    print("\n[size-limits] %s %s build times (s): %s; device memory in use %.2f GB" % (
        what, "x".join(map(str, shape)), ", ".join("%s %.3f" % t for t in times), peak / 1e9))


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _same_bits_chunks(name, got, want, chunk=128):
    """Two device float32 fields of one shape, bit for bit, in x chunks."""
    import torch
    for x0 in range(0, got.shape[0], chunk):
        a, b = got[x0:x0 + chunk].view(torch.int32), want[x0:x0 + chunk].view(torch.int32)
        if not bool(torch.equal(a, b)):
            bad = (a != b).nonzero()[:3].tolist()
            raise AssertionError("%s: x chunk %d: %d voxels differ, first %s" % (
                name, x0, int((a != b).sum()), [[v[0] + x0] + v[1:] for v in bad]))


# ---- A. boxes in free space: the closed form ------------------------------------------------------------------------------------------
# (x0, x1, y0, y1, z0, z1), half open.  One box across x = 2048 (linear index 2^31), one in the last x planes that reaches three grid
# faces, one at the origin's far y side, single voxels at linear indices 2^31 - 1 and 2^31, at the last plane and in free space.
# y and z are 1024 long, so their longest empty stretch is a whole row (1024); along x most rows are empty for more than 2000.
BOXES_BIG = [(2040, 2056, 500, 520, 100, 140), (3060, 3072, 0, 10, 1000, 1024), (0, 4, 1000, 1024, 0, 3), (700, 701, 3, 4, 1020, 1021),
             (2047, 2048, 1023, 1024, 1023, 1024), (2048, 2049, 0, 1, 0, 1), (3071, 3072, 1023, 1024, 0, 1)]


def _boxes_apart(shape, boxes):
    """Every box inside the grid, not the whole grid, and at least two voxels from every other one on some axis (so the voxel beyond
    each face that is not a grid face belongs to the other class)."""
    for b in boxes:
        assert all(0 <= b[2 * a] < b[2 * a + 1] <= shape[a] for a in range(3)), b
        assert any(b[2 * a] > 0 or b[2 * a + 1] < shape[a] for a in range(3)), b
    for i, p in enumerate(boxes):
        for q in boxes[i + 1:]:
            assert any(p[2 * a] - q[2 * a + 1] >= 2 or q[2 * a] - p[2 * a + 1] >= 2 for a in range(3)), (p, q)


def _box_axis(n, lo, hi, a, b, device):
    """For the coordinates [a, b) of an axis of n voxels and the box side [lo, hi): the distance to the side from outside (0 inside),
    the distance from inside to the nearest voxel beyond an end of the side (2^20 where both ends are grid faces), and inside."""
    import torch
    i = torch.arange(a, b, dtype=torch.int64, device=device)
    out = torch.clamp(torch.maximum(lo - i, i - (hi - 1)), min=0)
    none = torch.full_like(i, 1 << 20)
    face = torch.minimum((i - lo + 1) if lo > 0 else none, (hi - i) if hi < n else none)
    return out, face, (i >= lo) & (i < hi)


def _box_check(shape, boxes, inverse, vb, res, sdf, chunk=64):
    """Compare a device field with the exact field of solid axis-aligned boxes: a voxel outside every box is at the least, over the
    boxes, of the sum of its squared per-axis distances to the box's sides; a voxel inside a box is at its least distance to a face
    of that box that is not a grid face.  inverse: the boxes are the free voxels.  Returns the extrema."""
    import torch
    _boxes_apart(shape, boxes)
    nx, ny, nz = shape
    dev = sdf.device
    table = torch.from_numpy(_finish_table(sum((n - 1) ** 2 for n in shape) + 1, res)).to(dev)
    yz = [(_box_axis(ny, b[2], b[3], 0, ny, dev), _box_axis(nz, b[4], b[5], 0, nz, dev)) for b in boxes]
    vby = _vb_sq(ny, 0, ny, dev) if vb else None
    vbz = _vb_sq(nz, 0, nz, dev) if vb else None
    ext = _Extrema()
    for x0 in range(0, nx, chunk):
        x1 = min(nx, x0 + chunk)
        Dout, Dface, inbox = None, None, None
        for b, ((oy, fy, iy), (oz, fz, iz)) in zip(boxes, yz):
            ox, fx, ix = _box_axis(nx, b[0], b[1], x0, x1, dev)
            d = (ox * ox).view(-1, 1, 1) + (oy * oy).view(1, -1, 1) + (oz * oz).view(1, 1, -1)
            Dout = d if Dout is None else torch.minimum(Dout, d)
            ins = ix.view(-1, 1, 1) & iy.view(1, -1, 1) & iz.view(1, 1, -1)
            face = torch.minimum(torch.minimum(fx.view(-1, 1, 1), fy.view(1, -1, 1)), fz.view(1, 1, -1))
            Dface = torch.where(ins, face * face, torch.zeros_like(d) if Dface is None else Dface)
            inbox = ins if inbox is None else inbox | ins
            del d, ins, face
        filled = ~inbox if inverse else inbox
        vbx = _vb_sq(nx, x0, x1, dev) if vb else None
        terms = [t.view(*v) for t, v in ((vbx, (-1, 1, 1)), (vby, (1, -1, 1)), (vbz, (1, 1, -1))) if t is not None]
        want, Dc = _expected_chunk(Dface if inverse else Dout, filled, Dout if inverse else Dface, table, terms)
        got = sdf[x0:x1]
        eq = got.view(torch.int32) == want.view(torch.int32)
        if not bool(eq.all()):
            bad = (~eq).nonzero()[:3].tolist()
            raise AssertionError("x chunk %d: %d voxels differ, first %s" % (x0, int((~eq).sum()), [[v[0] + x0] + v[1:] for v in bad]))
        ext.add(Dc, filled)
        del Dout, Dface, inbox, filled, want, Dc, got, eq
    return ext.value(res)


def _box_mask(shape, boxes, inverse, device):
    import torch
    m = torch.full(shape, 1 if inverse else 0, dtype=torch.uint8, device=device)
    for b in boxes:
        m[b[0]:b[1], b[2]:b[3], b[4]:b[5]] = 0 if inverse else 1
    return m


SMALL_BOXES = {
    (23, 30, 40): [(10, 14, 5, 9, 3, 8), (20, 23, 0, 3, 36, 40), (0, 2, 27, 30, 0, 1), (5, 6, 20, 21, 30, 31), (11, 12, 29, 30, 39, 40),
                   (12, 13, 0, 1, 0, 1)],
    (17, 9, 34): [(0, 17, 3, 5, 10, 12), (4, 9, 8, 9, 30, 34), (16, 17, 0, 1, 0, 1)],
    (1, 15, 23): [(0, 1, 5, 8, 3, 9), (0, 1, 12, 15, 20, 23), (0, 1, 0, 1, 22, 23)],
    (6, 1, 1): [(2, 4, 0, 1, 0, 1)],
}


def test_box_closed_form_matches_the_oracle():
    import torch
    res = 0.01
    for shape, boxes in SMALL_BOXES.items():
        for inverse in (False, True):
            for vb in (False, True):
                m = _box_mask(shape, boxes, inverse, "cpu").numpy()
                ex, ex_ext, _ = O.exact_sdf(m, res, vb)
                t = torch.from_numpy(ex)
                assert _box_check(shape, boxes, inverse, vb, res, t, chunk=4) == ex_ext, (shape, inverse, vb)
                t[boxes[0][0], boxes[0][2], boxes[0][4]] *= 2
                with pytest.raises(AssertionError):
                    _box_check(shape, boxes, inverse, vb, res, t, chunk=4)
    # boxes of one voxel are point sites: the two closed forms agree with each other
    shape, sites = (13, 11, 14), [(0, 0, 0), (12, 10, 13), (6, 5, 7), (0, 5, 2), (12, 5, 2)]
    boxes = [(x, x + 1, y, y + 1, z, z + 1) for x, y, z in sites]
    for inverse in (False, True):
        t = torch.from_numpy(O.exact_sdf(_box_mask(shape, boxes, inverse, "cpu").numpy(), res)[0])
        assert _box_check(shape, boxes, inverse, False, res, t, chunk=5) == _sites_reference(shape, sites, inverse, res, t, chunk=5)
    _boxes_apart(BIG, BOXES_BIG)
    assert any(b[0] < 2048 < b[1] for b in BOXES_BIG) and any(b[1] == BIG[0] for b in BOXES_BIG)
    assert (2047 * BIG[1] + 1023) * BIG[2] + 1023 == 2 ** 31 - 1


@gpu_test
def test_far_field_scene_on_the_sweep_tier_past_2_31_voxels(big):
    """Seven boxes and single voxels in 3 * 2^30 voxels of free space, and the inverse scene, with and without the virtual border:
    the far-field planner refuses grids of 2^31 voxels, so the marching sweeps scan outward over up to a whole row in z and y and
    over more than 2000 planes in x, at linear indices past 2^31.  Every voxel and the extrema against the closed form."""
    import torch
    shape, res = BIG, 0.01
    dev, stream = _device()
    torch.cuda.empty_cache()
    base, peak, times = _used_device_bytes(), 0, []
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    for inverse in (False, True):
        m_t = _box_mask(shape, BOXES_BIG, inverse, dev)
        for vb in (False, True):
            big.set_option("policy_reset", 1)
            out.fill_(7.0)
            dt = _timed(lambda: big.build_device(m_t.data_ptr(), shape, out.data_ptr(), res, vb, stream))
            times.append(("boxes%s%s" % (" inverse" if inverse else "", " vb" if vb else ""), dt))
            peak = max(peak, _used_device_bytes() - base)
            ext, path = big.get_extrema(), big.last_path()
            assert not path["far_y"] and not path["far_x"], path
            want_ext = _box_check(shape, BOXES_BIG, inverse, vb, res, out)
            assert ext == want_ext, (inverse, vb, ext, want_ext)
        del m_t
    del out
    torch.cuda.empty_cache()
    _line("far-field scene, marching sweeps", shape, times, peak)


# ---- B. bits in ---------------------------------------------------------------------------------------------------------------------
def _pack_bits_torch(mask_flat):
    """Flat uint8 mask whose length is a multiple of 32 -> int32 words, bit (v & 31) of word (v >> 5) = voxel v."""
    import torch
    m = (mask_flat.view(-1, 32) != 0).to(torch.int64)
    w = (m << torch.arange(32, dtype=torch.int64, device=m.device)).sum(dim=1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def _pack_mask_bits(mask, chunk=1 << 27):
    """The linear bit field of a device mask of any shape whose voxel count is a multiple of 32, packed in chunks."""
    import torch
    flat = mask.view(-1)
    n = flat.numel()
    assert n % 32 == 0 and chunk % 32 == 0
    w = torch.empty(n // 32, dtype=torch.int32, device=mask.device)
    for v0 in range(0, n, chunk):
        w[v0 // 32:(min(n, v0 + chunk)) // 32] = _pack_bits_torch(flat[v0:v0 + chunk])
    return w


def _lattice_bits(shape, inverse, device):
    """The bit field of the point lattice of _lattice_mask from the word pattern of one z row (nz a multiple of 32)."""
    import torch
    nx, ny, nz = shape
    assert nz % 32 == 0
    row = (np.arange(nz) % STRIDES[2] == 0).astype(np.uint8)
    pat = torch.from_numpy(capi.pack_bits_host(row).view(np.int32).copy()).to(device)
    w = torch.zeros((nx, ny, nz // 32), dtype=torch.int32, device=device)
    w[0::STRIDES[0], 0::STRIDES[1], :] = pat
    if inverse:
        w.bitwise_not_()
    return w


def test_bit_fields_match_pack_bits_host():
    for shape in ((11, 15, 64), (1, 8, 32), (6, 7, 96)):
        for inverse in (False, True):
            m = _lattice_mask(shape, inverse, "cpu")
            want = capi.pack_bits_host(m.numpy())
            assert np.array_equal(_lattice_bits(shape, inverse, "cpu").numpy().view(np.uint32).reshape(-1), want), (shape, inverse)
            assert np.array_equal(_pack_mask_bits(m, chunk=64).numpy().view(np.uint32), want), (shape, inverse)
    for shape in ((4, 8, 31), (32, 3, 5), (1, 1, 64)):              # rows that are not whole words
        m = synth.bernoulli_mask(shape, 0.5, 3)
        import torch
        got = _pack_mask_bits(torch.from_numpy(m), chunk=32).numpy().view(np.uint32)
        assert np.array_equal(got, capi.pack_bits_host(m)), shape
        got[0] ^= 1
        assert not np.array_equal(got, capi.pack_bits_host(m))


BIG_ODD_NZ = (3072, 1024, 1023)                                    # 3 * 2^20 rows of 1023 voxels: rows start inside words


@gpu_test
def test_bits_in_past_2_31_voxels(big):
    """sdfgpu_build_bits_device at 3072 x 1024 x 1024 (the lattice without the virtual border and its inverse with it -- two of the
    four combinations -- every voxel against the closed form), at 3072 x 1024 x 1023 (rows that start inside words; 3.2e9 voxels;
    the lattice with the border only) and on Bernoulli(0.5) without the border, bit-equal to the byte-mask build of the same scene
    on a second handle, extrema included."""
    import torch
    shape, res = BIG, 0.01
    dev, stream = _device()
    torch.cuda.empty_cache()
    base, peak, times = _used_device_bytes(), 0, []
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    for inverse, vb in ((False, False), (True, True)):
        bits = _lattice_bits(shape, inverse, dev)
        big.set_option("policy_reset", 1)
        out.fill_(7.0)
        dt = _timed(lambda: big.build_bits_device(bits.data_ptr(), shape, out.data_ptr(), res, vb, stream))
        times.append(("lattice bits" + (" inverse vb" if inverse else ""), dt))
        peak = max(peak, _used_device_bytes() - base)
        ext = big.get_extrema()
        del bits
        want_ext = _lattice_check(shape, inverse, vb, res, out)
        assert ext == want_ext, (inverse, vb, ext, want_ext)
    # nz = 1023
    odd = BIG_ODD_NZ
    assert math.prod(odd) > 2 ** 31 and math.prod(odd) % 32 == 0 and odd[2] % 32
    m_t = _lattice_mask(odd, False, dev)
    bits = _pack_mask_bits(m_t)
    del m_t
    out_odd = out.view(-1)[:math.prod(odd)].view(odd)
    out_odd.fill_(7.0)
    big.set_option("policy_reset", 1)
    dt = _timed(lambda: big.build_bits_device(bits.data_ptr(), odd, out_odd.data_ptr(), res, True, stream))
    times.append(("lattice bits vb %s" % "x".join(map(str, odd)), dt))
    peak = max(peak, _used_device_bytes() - base)
    ext = big.get_extrema()
    del bits
    want_ext = _lattice_check(odd, False, True, res, out_odd)
    assert ext == want_ext, (odd, ext, want_ext)
    del out_odd
    # Bernoulli(0.5) against the byte-mask build
    nx = shape[0]
    m_t = torch.empty(shape, dtype=torch.uint8, device=dev)
    for x0 in range(0, nx, 256):
        m_t[x0:x0 + 256] = synth.bernoulli_mask_torch(shape, 0.5, 11, x_range=(x0, min(nx, x0 + 256)), device=dev)
    bits = _pack_mask_bits(m_t)
    big.set_option("policy_reset", 1)
    out.fill_(7.0)
    dt = _timed(lambda: big.build_bits_device(bits.data_ptr(), shape, out.data_ptr(), res, False, stream))
    times.append(("bernoulli 0.5 bits", dt))
    ext = big.get_extrema()
    other = capi.SdfGpu(0)
    try:
        other.set_option("dense_retry", 0)
        out2 = torch.full(shape, 9.0, dtype=torch.float32, device=dev)
        dt = _timed(lambda: other.build_device(m_t.data_ptr(), shape, out2.data_ptr(), res, False, stream))
        times.append(("bernoulli 0.5 bytes", dt))
        peak = max(peak, _used_device_bytes() - base)
        assert ext == other.get_extrema(), (ext, other.get_extrema())
        assert math.isfinite(ext[0]) and math.isfinite(ext[1])
        _same_bits_chunks("bits build vs byte build", out, out2)
    finally:
        other.close()
    del out, out2, m_t, bits
    torch.cuda.empty_cache()
    _line("bits in", shape, times, peak)


# ---- C. cells in ----------------------------------------------------------------------------------------------------------------------
# the occupancies of test_host_side_classification_matches_the_device_classifier (test_gpu_parity.py)
OCC_VALUES = np.array([0.0, 0.25, 0.5, 0.50000006, 0.75, 1.0, -10000.0, np.nan], np.float32)
CELL_LAYOUTS = {8: (2, 0), 16: (4, 2)}                             # stride -> (words per record, word of the occupancy)


def _cell_kind(shape, x0, x1, device):
    """Which of OCC_VALUES the cell (x, y, z) holds, int64 [x1 - x0, ny, nz].  The terms in x >> 8 and x >> 9 break the period of
    the others in x (32 planes): a record read at its byte offset modulo 2^32 -- 2^29 cells or 512 planes at stride 8, 256 planes
    at stride 16 -- holds another kind (+7 or +3 modulo 8).  Without them a classifier with a 32-bit offset passed this test."""
    import torch
    _, ny, nz = shape
    x = torch.arange(x0, x1, dtype=torch.int64, device=device).view(-1, 1, 1)
    y = torch.arange(ny, dtype=torch.int64, device=device).view(1, -1, 1)
    z = torch.arange(nz, dtype=torch.int64, device=device).view(1, 1, -1)
    return (x + 3 * y + 5 * z + ((x * y + y * z + z * x) >> 2) + 3 * (x >> 8) + (x >> 9)) & 7


def _cell_records(shape, x0, x1, stride, device):
    """Records of x planes [x0, x1) as int32 [x1 - x0, ny, nz, stride / 4]: the occupancy in its word, another of OCC_VALUES in
    word 0 where that is not the occupancy's, garbage in the rest."""
    import torch
    words, occ_word = CELL_LAYOUTS[stride]
    k = _cell_kind(shape, x0, x1, device)
    occ_bits = torch.from_numpy(OCC_VALUES.view(np.int32).copy()).to(device)
    rec = torch.empty(tuple(k.shape) + (words,), dtype=torch.int32, device=device)
    z = torch.arange(shape[2], dtype=torch.int64, device=device).view(1, 1, -1)
    for w in range(words):
        if w == occ_word:
            rec[..., w] = occ_bits[k]
        elif w == 0:
            rec[..., w] = occ_bits[(k + 3) & 7]
        else:
            rec[..., w] = ((k * 0x9E3779B1 + z * 7919 + w * 0x01234567) & 0x7FFFFFFF).to(torch.int32)
    return rec


def _cells_mask_check(shape, nx_used, unknown, mask, chunk=64):
    """The classifier's byte mask of the first nx_used x planes against the formula: OCC_VALUES[kind] > 0.5, or == 0.5 when unknown
    cells count as filled."""
    import torch
    filled = torch.from_numpy(((OCC_VALUES > 0.5) | (bool(unknown) & (OCC_VALUES == 0.5))).astype(np.uint8)).to(mask.device)
    for x0 in range(0, nx_used, chunk):
        x1 = min(nx_used, x0 + chunk)
        want = filled[_cell_kind(shape, x0, x1, mask.device)]
        got = mask[x0:x1]
        if not bool(torch.equal(got, want)):
            bad = (got != want).nonzero()[:3].tolist()
            raise AssertionError("x chunk %d: %d mask bytes differ, first %s" % (x0, int((got != want).sum()), [[v[0] + x0] + v[1:] for v in bad]))


def test_cell_formula_matches_the_oracle_classifier():
    import torch
    assert OCC_VALUES[3] == np.nextafter(np.float32(0.5), np.float32(1.0))
    for stride in (8, 16):                                           # a byte offset taken modulo 2^32 reads another kind, everywhere
        wrap = (2 ** 32 // stride) // (BIG[1] * BIG[2])
        tiny = (BIG[0], 3, 5)
        k = _cell_kind(tiny, 0, BIG[0], "cpu")
        assert wrap in (512, 256) and bool((k[wrap:] != k[:-wrap]).all()), stride
    for shape in ((9, 12, 10), (1, 20, 33), (16, 5, 8)):
        kinds = _cell_kind(shape, 0, shape[0], "cpu").numpy()
        assert set(np.unique(kinds).tolist()) == set(range(8)), shape         # every occupancy occurs
        for stride in (8, 16):
            words, occ_word = CELL_LAYOUTS[stride]
            rec = torch.cat([_cell_records(shape, x0, min(shape[0], x0 + 4), stride, "cpu") for x0 in range(0, shape[0], 4)]).numpy()
            assert rec.shape == shape + (words,) and rec.dtype == np.int32
            pair = np.ascontiguousarray(rec[..., occ_word:occ_word + 2]).view(np.float32)
            for unknown in (False, True):
                want = O.classify_cells(pair, unknown)
                _cells_mask_check(shape, shape[0], unknown, torch.from_numpy(want), chunk=4)
                bad = want.copy()
                bad[shape[0] - 1, 2, 3] ^= 1
                with pytest.raises(AssertionError):
                    _cells_mask_check(shape, shape[0], unknown, torch.from_numpy(bad), chunk=4)
            if occ_word:                                                     # word 0 alone would classify differently
                decoy = np.ascontiguousarray(rec[..., 0:2]).view(np.float32)
                assert not np.array_equal(O.classify_cells(decoy, False), O.classify_cells(pair, False))


@gpu_test
@pytest.mark.parametrize("stride", [8, 16])
def test_cells_in_past_2_32_bytes(big, stride):
    """{float32 occupancy, uint32 garbage} at stride 8 and a 16-byte record with the occupancy at offset 8, built on the device:
    sdfgpu_classify_cells_device at 1024^3 cells (byte offsets past 2^32) and at 3 * 2^30 cells, both values of unknown_is_filled,
    every mask byte against the formula; sdfgpu_build_cells_device at 3 * 2^30 cells bit-equal to sdfgpu_build_device on that mask."""
    import torch
    shape, res = BIG, 0.01
    nx, ny, nz = shape
    n = math.prod(shape)
    words, occ_word = CELL_LAYOUTS[stride]
    dev, stream = _device()
    torch.cuda.empty_cache()
    need = n * stride + n + 2 * 4 * n + 6 * n + (6 << 30)            # records, mask, two fields, the library's scratch, chunks
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %.1f GB of free device memory, %.1f GB are free" % (need / 1e9, free / 1e9))
    base, times = _used_device_bytes(), []
    rec = torch.empty(shape + (words,), dtype=torch.int32, device=dev)
    for x0 in range(0, nx, 64):
        rec[x0:x0 + 64] = _cell_records(shape, x0, min(nx, x0 + 64), stride, dev)
    mask = torch.empty(shape, dtype=torch.uint8, device=dev)
    unknown_build = stride == 8
    for cells_x in (1024, nx):
        assert cells_x * ny * nz * stride > 2 ** 32
        for unknown in ((False, True) if unknown_build else (True, False)):       # (the last mask is the build's)
            mask.fill_(0xEE)
            dt = _timed(lambda: big.classify_cells_device(rec.data_ptr(), cells_x * ny * nz, mask.data_ptr(), stride, 4 * occ_word,
                                                          unknown, stream))
            times.append(("classify %d planes unknown=%d" % (cells_x, unknown), dt))
            _cells_mask_check(shape, cells_x, unknown, mask)
            assert bool((mask[cells_x:] == 0xEE).all())                           # nothing written past n_cells
    out = torch.full(shape, 7.0, dtype=torch.float32, device=dev)
    big.set_option("policy_reset", 1)
    dt = _timed(lambda: big.build_cells_device(rec.data_ptr(), shape, out.data_ptr(), stride, 4 * occ_word, unknown_build, res,
                                               False, stream))
    times.append(("build_cells", dt))
    ext = big.get_extrema()
    peak = _used_device_bytes() - base
    del rec
    torch.cuda.empty_cache()
    out2 = torch.full(shape, 9.0, dtype=torch.float32, device=dev)
    big.set_option("policy_reset", 1)
    dt = _timed(lambda: big.build_device(mask.data_ptr(), shape, out2.data_ptr(), res, False, stream))
    times.append(("build on the mask", dt))
    assert ext == big.get_extrema(), (ext, big.get_extrema())
    _same_bits_chunks("cells build vs mask build", out, out2)
    del out, out2, mask
    torch.cuda.empty_cache()
    _line("cells in, stride %d" % stride, shape, times, peak)


# ---- D. voxelisation ------------------------------------------------------------------------------------------------------------------
VOX_ORIGIN, VOX_RES = (-8.0, 16.0, 4.0), 0.5                       # every point below is exact in float32 and in the kernel's doubles


def _voxel_points(shape, n_each, device, seed=3):
    """(points float32 [n, 3], cells int64 [m]): points with known cells, shuffled, and the linear indices of the points that land in
    the grid (duplicates kept).  In grid units u = (p - origin) / res: cell centres (u = c + 0.5) of random cells, of cells in the
    last 8 x planes and of the cells at linear indices 0, 2^31 - 1, 2^31 (where the grid has them) and n - 1; repeats of the
    first centres; points on the lower faces of their cell (u = c on one, two or three axes); u = -0.5 on an axis, which truncates
    to cell 0; and points that must be dropped: u = n (the grid's upper face), u = -1, far outside, NaN and both infinities."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    nx, ny, nz = shape
    dims = torch.tensor(shape, dtype=torch.int64, device=device)

    def cells(n, xlo=0):
        return torch.stack([torch.randint(xlo, nx, (n,), generator=g, device=device), torch.randint(0, ny, (n,), generator=g, device=device),
                            torch.randint(0, nz, (n,), generator=g, device=device)], 1)

    def lin(c):
        return (c[:, 0] * ny + c[:, 1]) * nz + c[:, 2]

    fixed = [v for v in (0, 2 ** 31 - 1, 2 ** 31, nx * ny * nz - 1) if v < nx * ny * nz]
    fixed = torch.tensor([[v // (ny * nz), (v // nz) % ny, v % nz] for v in fixed], dtype=torch.int64, device=device)
    centres = torch.cat([cells(n_each), cells(n_each, max(0, nx - 8)), fixed])
    centres = torch.cat([centres, centres[:n_each // 4]])
    kept_c = [centres]
    kept_u = [centres.double() + 0.5]
    on_face = cells(n_each // 4)
    which = torch.randint(1, 8, (len(on_face),), generator=g, device=device)             # a non-empty set of axes
    axes = torch.stack([(which >> a) & 1 for a in range(3)], 1).bool()
    kept_c.append(on_face)
    kept_u.append(torch.where(axes, on_face.double(), on_face.double() + 0.5))
    low = cells(n_each // 8)
    axis = torch.randint(0, 3, (len(low),), generator=g, device=device)
    hit = torch.nn.functional.one_hot(axis, 3).bool()
    low = torch.where(hit, torch.zeros_like(low), low)
    kept_c.append(low)
    kept_u.append(torch.where(hit, torch.full_like(low, -0.5, dtype=torch.float64), low.double() + 0.5))
    drop_u = []
    for value in (None, -1.0, -3.5, 1e7, math.nan, math.inf, -math.inf):
        c = cells(n_each // 16)
        axis = torch.randint(0, 3, (len(c),), generator=g, device=device)
        hit = torch.nn.functional.one_hot(axis, 3).bool()
        bad = dims.double().expand(len(c), 3) if value is None else torch.full((len(c), 3), value, dtype=torch.float64, device=device)
        drop_u.append(torch.where(hit, bad, c.double() + 0.5))
    u = torch.cat(kept_u + drop_u)
    origin = torch.tensor(VOX_ORIGIN, dtype=torch.float64, device=device)
    p64 = origin + u * VOX_RES
    p = p64.float()
    finite = torch.isfinite(p64)
    assert bool((p.double()[finite] == p64[finite]).all())                                # exact in float32
    perm = torch.randperm(len(p), generator=g, device=device)
    return p[perm].contiguous(), lin(torch.cat(kept_c))


def _numpy_voxelize(points, shape):
    """scripts/3d_sdf_demo_rviz.py:22-29 on float32 points, dropping what falls outside: the sorted unique linear indices."""
    with np.errstate(invalid="ignore"):
        f = (points.astype(np.float64) - np.asarray(VOX_ORIGIN)) / VOX_RES
        ok = np.isfinite(f).all(axis=1)
        idx = f[ok].astype(np.int64)                                                      # truncation toward zero
    ok = ((idx >= 0) & (idx < np.asarray(shape))).all(axis=1)
    idx = idx[ok]
    return np.unique((idx[:, 0] * shape[1] + idx[:, 1]) * shape[2] + idx[:, 2])


def test_voxel_points_land_in_their_cells():
    for shape in ((40, 33, 48), (1, 17, 64), (9, 1, 5)):
        p, want = _voxel_points(shape, 4000, "cpu")
        got = _numpy_voxelize(p.numpy(), shape)
        assert np.array_equal(got, np.unique(want.numpy())), shape
        assert len(want) > len(got)                                                        # duplicates are there
    p, want = _voxel_points((40, 33, 48), 4000, "cpu")
    u = (p.numpy().astype(np.float64) - np.asarray(VOX_ORIGIN)) / VOX_RES
    assert np.isnan(u).any() and np.isinf(u).any() and (u == 40).any() and (u == -1).any() and (u == -0.5).any()
    assert ((u == np.floor(u)) & np.isfinite(u) & (u >= 0) & (u < 33)).any()


def _count_bits(words, chunk=1 << 26):
    """Set bits of an int32 device tensor, through a byte table."""
    import torch
    table = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int64, device=words.device)
    b = words.view(-1).view(torch.uint8)
    return sum(int(table[b[i:i + chunk].long()].sum()) for i in range(0, b.numel(), chunk))


def _count_nonzero(t, chunk=1 << 28):
    flat = t.view(-1)
    return sum(int((flat[i:i + chunk] != 0).sum()) for i in range(0, flat.numel(), chunk))


@gpu_test
def test_voxelize_past_2_31_cells(big):
    """About six million points into 3072 x 1024 x 1024: the byte mask (cell indices past 2^31) and the bit field (bit indices past 2^31),
    clear_first on over a buffer of garbage and off over a pattern that must survive.  The set voxels are exactly the expected
    cells: their count equals the number of unique expected cells and every expected cell is set."""
    import torch
    shape = BIG
    n = math.prod(shape)
    dev, stream = _device()
    torch.cuda.empty_cache()
    base = _used_device_bytes()
    p, cells = _voxel_points(shape, 2_000_000, dev)
    want = torch.unique(cells)
    assert int((want >= 2 ** 31).sum()) > 1_000_000 and int(want[0]) == 0 and int(want[-1]) == n - 1
    assert bool((want == 2 ** 31 - 1).any()) and bool((want == 2 ** 31).any())
    times = []
    # bytes
    mask = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    dt = _timed(lambda: big.voxelize_points_device(p.data_ptr(), len(p), VOX_ORIGIN, VOX_RES, shape, mask.data_ptr(), True, stream))
    times.append(("bytes clear", dt))
    assert _count_nonzero(mask) == len(want)
    assert bool((mask[want] == 1).all())
    pat = torch.arange(5, n, 9973, dtype=torch.int64, device=dev)                      # a pattern of sevens
    mask.zero_()
    mask[pat] = 7
    dt = _timed(lambda: big.voxelize_points_device(p.data_ptr(), len(p), VOX_ORIGIN, VOX_RES, shape, mask.data_ptr(), False, stream))
    times.append(("bytes keep", dt))
    both = int(torch.isin(pat, want).sum())
    assert _count_nonzero(mask) == len(want) + len(pat) - both
    assert bool((mask[want] == 1).all())
    assert int((mask[pat] == 7).sum()) == len(pat) - both and bool((mask[pat] != 0).all())
    peak = _used_device_bytes() - base
    del mask
    # bits
    bits = torch.full((n // 32,), -1, dtype=torch.int32, device=dev)
    dt = _timed(lambda: big.voxelize_points_bits_device(p.data_ptr(), len(p), VOX_ORIGIN, VOX_RES, shape, bits.data_ptr(), True, stream))
    times.append(("bits clear", dt))

    def bit_set(v):
        return (bits[v >> 5].long() >> (v & 31)) & 1

    assert _count_bits(bits) == len(want)
    assert bool((bit_set(want) == 1).all())
    pat = torch.arange(3, n // 32, 1009, dtype=torch.int64, device=dev) * 32 + 16       # bit 16 of every 1009th word
    bits.zero_()
    bits[pat >> 5] = 1 << 16
    dt = _timed(lambda: big.voxelize_points_bits_device(p.data_ptr(), len(p), VOX_ORIGIN, VOX_RES, shape, bits.data_ptr(), False, stream))
    times.append(("bits keep", dt))
    both = int(torch.isin(pat, want).sum())
    assert _count_bits(bits) == len(want) + len(pat) - both
    assert bool((bit_set(want) == 1).all()) and bool((bit_set(pat) == 1).all())
    del bits
    torch.cuda.empty_cache()
    print("\n[size-limits] voxelise %d points (%d cells) into %s, times (s): %s; device memory in use %.2f GB" % (
        len(p), len(want), "x".join(map(str, shape)), ", ".join("%s %.4f" % t for t in times), peak / 1e9))


# ---- E. the full-field gradient -------------------------------------------------------------------------------------------------------
def _torch_gradient(f, x0, x1, res, edge):
    """analysis_scenes.grid_gradient restated in torch for the x planes [x0, x1) of the device field f, from those planes and one
    more on each side: float64 [x1 - x0, ny, nz, 3]."""
    import torch
    shape = tuple(f.shape)
    dev = f.device
    ranges = [torch.arange(x0, x1, device=dev)] + [torch.arange(n, device=dev) for n in shape[1:]]
    views = [(-1, 1, 1), (1, -1, 1), (1, 1, -1)]
    interior = None
    for ax, n in enumerate(shape):
        t = ((ranges[ax] > 0) & (ranges[ax] < n - 1)).view(views[ax])
        interior = t if interior is None else interior & t
    inv2 = 1.0 / (2.0 * res)
    centre = f[x0:x1]
    out = torch.empty(tuple(centre.shape) + (3,), dtype=torch.float64, device=dev)
    nan = torch.full((), math.nan, dtype=torch.float64, device=dev)
    for ax, n in enumerate(shape):
        i = ranges[ax]
        lo, hi = torch.clamp(i - 1, min=0), torch.clamp(i + 1, max=n - 1)
        if ax == 0:
            fl, fh = f.index_select(0, lo), f.index_select(0, hi)
        else:
            fl, fh = centre.index_select(ax, lo), centre.index_select(ax, hi)
        inner = (fh - fl).double() * inv2
        w = (hi - lo).view(views[ax])
        scale = torch.where(w > 0, 1.0 / (w.double() * res), torch.zeros((), dtype=torch.float64, device=dev))
        shell = torch.where(w > 0, (fh.double() - fl.double()) * scale, torch.zeros((), dtype=torch.float64, device=dev))
        out[..., ax] = torch.where(interior, inner, shell if edge else nan)
        del fl, fh, inner, shell
    return out


def _gradient_check(f, res, edge, got, chunk=32):
    """A device gradient [nx, ny, nz, 3] (float64, or float32: the float64 values narrowed once) against _torch_gradient, bit for
    bit (two NaNs are equal)."""
    import torch
    ints = torch.int64 if got.dtype == torch.float64 else torch.int32
    for x0 in range(0, f.shape[0], chunk):
        x1 = min(f.shape[0], x0 + chunk)
        want = _torch_gradient(f, x0, x1, res, edge).to(got.dtype)
        g = got[x0:x1]
        eq = (g.view(ints) == want.view(ints)) | (torch.isnan(g) & torch.isnan(want))
        if not bool(eq.all()):
            bad = (~eq).nonzero()[:3].tolist()
            raise AssertionError("x chunk %d: %d components differ, first %s" % (x0, int((~eq).sum()), [[v[0] + x0] + v[1:] for v in bad]))
        del want, g, eq


def test_torch_gradient_matches_the_numpy_restatement():
    import torch
    rng = np.random.default_rng(2)
    for shape in ((12, 9, 10), (1, 7, 12), (9, 11, 1), (33, 5, 8), (2, 2, 2)):
        f = (rng.integers(-40, 41, shape) * 0.125).astype(np.float32)
        f[rng.random(shape) < 0.03] = np.inf
        for res in (0.01, 0.25, 0.03):
            for edge in (True, False):
                want = A.grid_gradient(f, res, edge)
                for dt in (np.float64, np.float32):
                    t = torch.from_numpy(want.astype(dt))
                    _gradient_check(torch.from_numpy(f), res, edge, t, chunk=5)
                    t[shape[0] - 1, shape[1] - 1, 0, 2] = 123.0
                    with pytest.raises(AssertionError):
                        _gradient_check(torch.from_numpy(f), res, edge, t, chunk=5)


GRAD_SCALAR_SHAPE = (3075, 1024, 1023)


@gpu_test
def test_full_gradient_past_2_32_output_elements(big):
    """sdfgpu_gradient_device on the 3072 x 1024 x 1024 field of the point lattice: 9.7e9 output elements, float32 (nz % 4 == 0,
    ny nz / 4 = 2^18 groups per plane and 16-byte aligned buffers: the vector kernel k_gradient_f32x4, with 1 / (2 res) = 50 exact
    in float32) and float64 (k_gradient<double>).  The library does not report which float32 kernel ran; the other one,
    k_gradient<float>, takes every field whose nz is not a multiple of 4, so the same 12 GiB of floats are read again as a
    3075 x 1024 x 1023 field (a gradient is defined for any floats), without edge gradients.  Every component against the torch
    restatement of analysis_scenes.grid_gradient.  Of the vector kernel only k_gradient_f32x4<true> (the float32 scale) with
    nz / 4 a power of two (gshift = 8, the shift in place of the division) runs here: its <false> variant (1 / (2 res) not exact
    in float32) and the gshift = -1 division are not taken past 2^31; they share the 64-bit index and store arithmetic below the
    row decomposition, and test_gpu_analysis_edges.py covers them at small sizes."""
    import torch
    shape, res = BIG, 0.01
    n = math.prod(shape)
    dev, stream = _device()
    torch.cuda.empty_cache()
    base, times = _used_device_bytes(), []
    assert 3 * n > 2 ** 32 and shape[2] % 4 == 0 and GRAD_SCALAR_SHAPE[2] % 4 and 2 ** 31 < math.prod(GRAD_SCALAR_SHAPE) <= n
    m_t = _lattice_mask(shape, False, dev)
    f = torch.empty(shape, dtype=torch.float32, device=dev)
    big.set_option("policy_reset", 1)
    big.build_device(m_t.data_ptr(), shape, f.data_ptr(), res, False, stream)
    torch.cuda.synchronize()
    del m_t
    _lattice_check(shape, False, False, res, f)
    peak = 0
    for f64 in (False, True):
        g = torch.full(shape + (3,), -7.0, dtype=torch.float64 if f64 else torch.float32, device=dev)
        assert f.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
        dt = _timed(lambda: big.gradient_device(f.data_ptr(), shape, g.data_ptr(), res, True, f64, stream))
        times.append(("float64" if f64 else "float32 vector", dt))
        peak = max(peak, _used_device_bytes() - base)
        _gradient_check(f, res, True, g)
        del g
        torch.cuda.empty_cache()
    s = GRAD_SCALAR_SHAPE
    ns = math.prod(s)
    fs = f.view(-1)[:ns].view(s)
    g = torch.full((3 * ns + 8,), -7.0, dtype=torch.float32, device=dev)
    dt = _timed(lambda: big.gradient_device(fs.data_ptr(), s, g.data_ptr(), res, False, False, stream))
    times.append(("float32 scalar %s" % "x".join(map(str, s)), dt))
    assert bool((g[3 * ns:] == -7.0).all())                                       # nothing written past the last element
    _gradient_check(fs, res, False, g[:3 * ns].view(s + (3,)))
    del g, f, fs
    torch.cuda.empty_cache()
    _line("full-field gradient", shape, times, peak)


# ---- F. point queries -----------------------------------------------------------------------------------------------------------------
def _query_points_cropped(field, lo, res, g, oob=np.inf, edge=False):
    """analysis_scenes.query_points for points whose cells lie at least two cells inside the low faces of the crop
    field[lo[0]:, lo[1]:, lo[2]:] -- `field` has the whole grid's shape but only that crop holds data: the distance through
    estimate_distance on the whole array (it reads the surrounding cells alone), the gradient through grid_gradient on the crop
    (whose high faces are the grid's)."""
    g = np.asarray(g, np.float64)
    n = len(g)
    dist, grad, flags = np.full(n, oob, np.float64), np.full((n, 3), np.nan), np.zeros(n, np.uint8)
    with np.errstate(invalid="ignore"):
        fi = np.floor(g * (1.0 / res))
        inside = np.all(fi >= 0.0, axis=1) & np.all(fi < np.asarray(field.shape, np.float64), axis=1)
    idx = fi[inside].astype(np.int64)
    assert (idx >= np.asarray(lo) + 2).all()
    dist[inside] = A.estimate_distance(field, res, g[inside])
    crop = np.ascontiguousarray(field[lo[0]:, lo[1]:, lo[2]:])
    c = idx - np.asarray(lo)
    full = A.grid_gradient(crop, res, edge)[c[:, 0], c[:, 1], c[:, 2]]
    with np.errstate(invalid="ignore"):
        grad[inside] = np.stack([1.0 * full[:, 0] + 0.0 * full[:, 1] + 0.0 * full[:, 2], 0.0 * full[:, 0] + 1.0 * full[:, 1] + 0.0 * full[:, 2],
                                 0.0 * full[:, 0] + 0.0 * full[:, 1] + 1.0 * full[:, 2]], 1)
    have = np.ones(len(idx), bool) if edge else A._interior(idx, field.shape)
    flags[inside] = 1 | np.where(have, 2, 0).astype(np.uint8)
    return dist, grad, flags


def _query_cloud(shape, lo, res, n, seed):
    """Grid-frame points in the last cells of every axis (their eight surrounding cells at least three cells above `lo`), on cell
    faces and centres, on the grid's high faces, and outside beyond them."""
    rng = np.random.default_rng(seed)
    hi = np.asarray(shape, np.float64)
    deep = np.column_stack([rng.uniform(hi[0] - 1, hi[0], n), rng.uniform(lo[1] + 4, hi[1], n), rng.uniform(lo[2] + 4, hi[2], n)])
    any_x = np.column_stack([rng.uniform(lo[0] + 4, hi[0] + 0.5, n // 2), rng.uniform(lo[1] + 4, hi[1] + 0.5, n // 2),
                             rng.uniform(lo[2] + 4, hi[2] + 0.5, n // 2)])
    snapped = np.floor(any_x[: n // 4] * 2) / 2                                    # cell faces and centres
    corner = np.array([[hi[0] - 0.5, hi[1] - 0.5, hi[2] - 0.5], [hi[0] - 1e-9, hi[1] - 1e-9, hi[2] - 1e-9], [hi[0], hi[1] - 1, hi[2] - 1]])
    return deep, np.concatenate([deep, any_x, snapped, corner]) * res


def _same_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64 if a.dtype == np.float64 else np.uint8) ==
                                               b.view(np.uint64 if b.dtype == np.float64 else np.uint8)) | _both_nan(a, b)))


def _differences(a, b):
    """For a failure message: how many entries differ, the first few of them and the largest finite difference."""
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(invalid="ignore"):
        bad = ~((a == b) | _both_nan(a, b))
        where = np.argwhere(bad)[:3].tolist()
        gap = np.abs(a[bad].astype(np.float64) - b[bad].astype(np.float64))
    return "%d differ, first at %s, largest finite difference %r" % (int(bad.sum()), where, float(np.nanmax(gap[np.isfinite(gap)], initial=0.0)))


def _both_nan(a, b):
    return (np.isnan(a) & np.isnan(b)) if a.dtype == np.float64 else np.zeros(a.shape, bool)


def test_cropped_query_restatement_matches_the_whole_field():
    res = 0.01
    for shape, lo in (((20, 19, 17), (6, 5, 4)), ((30, 12, 14), (20, 0, 0)), ((9, 16, 15), (0, 4, 3))):
        sdf = O.exact_sdf(synth.bernoulli_mask(shape, 0.2, sum(shape)), res)[0]
        held = np.full(shape, np.float32(1e30))                                    # (only the crop holds the field)
        held[lo[0]:, lo[1]:, lo[2]:] = sdf[lo[0]:, lo[1]:, lo[2]:]
        deep, g = _query_cloud(shape, lo, res, 400, 3)
        for edge in (False, True):
            want = A.query_points(sdf, res, g, np.inf, edge)
            got = _query_points_cropped(held, lo, res, g, np.inf, edge)
            assert all(_same_nan(a, b) for a, b in zip(got, want)), (shape, edge)
            assert {0, 1, 3} <= set(want[2].tolist()) if not edge else {0, 3} <= set(want[2].tolist())
        held[shape[0] - 1, shape[1] - 1, shape[2] - 1] += 1.0
        assert not _same_nan(_query_points_cropped(held, lo, res, g)[0], want[0])


QUERY_SHAPE, QUERY_LO = (1300, 1300, 1272), (1278, 896, 868)


@gpu_test
def test_point_queries_past_2_31_cells(big):
    """sdfgpu_query_points_device and sdfgpu_query_points on a 1300 x 1300 x 1272 field (2.15e9 cells): points whose eight
    surrounding cells all have linear indices past 2^31, points on the high faces and outside.  Distances, gradients and flags of
    every point bit-equal to the restated EstimateDistance / gradient on the downloaded last planes, edge gradients off and on."""
    import torch
    shape, lo, res = QUERY_SHAPE, QUERY_LO, 0.01
    dev, stream = _device()
    torch.cuda.empty_cache()
    base = _used_device_bytes()
    mt = torch.zeros(shape, dtype=torch.uint8, device=dev)
    mt[1285:, 900:1100, 600:1000] = 1
    mt[1290:1296, 1200:1290, 1100:1260] = 1
    mt[:, :, :2] = 1
    f = torch.empty(shape, dtype=torch.float32, device=dev)
    big.set_option("policy_reset", 1)
    t_build = _timed(lambda: big.build_device(mt.data_ptr(), shape, f.data_ptr(), res, False, stream))
    del mt
    peak = _used_device_bytes() - base
    held = np.empty(shape, np.float32)                                             # (pages outside the crop are never touched)
    held[lo[0]:, lo[1]:, lo[2]:] = f[lo[0]:, lo[1]:, lo[2]:].cpu().numpy()
    deep, g = _query_cloud(shape, lo, res, 4000, 4)
    c = np.floor(deep) - 1
    assert ((c[:, 0] * shape[1] + c[:, 1]) * shape[2] + c[:, 2] > 2 ** 31).all()
    n = len(g)
    dp = torch.from_numpy(np.ascontiguousarray(g)).to(dev)
    times = [("build", t_build)]
    for edge in (False, True):
        want = _query_points_cropped(held, lo, res, g, np.inf, edge)
        assert (want[2][:len(deep)] == 3).all() or not edge
        dist = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        grad = torch.full((n, 3), -1.0, dtype=torch.float64, device=dev)
        flags = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        dt = _timed(lambda: big.query_points_device(f.data_ptr(), shape, res, dp.data_ptr(), n, dist.data_ptr(), grad.data_ptr(),
                                                    flags.data_ptr(), None, None, math.inf, edge, stream))
        times.append(("device edge=%d" % edge, dt))
        got = (dist.cpu().numpy(), grad.cpu().numpy(), flags.cpu().numpy())
        for name, a, b in zip(("distance", "gradient", "flags"), got, want):
            assert _same_nan(a, b), ("device", name, edge, _differences(a, b))
        t0 = time.perf_counter()
        got = big.query_points(f.data_ptr(), shape, res, g, None, None, math.inf, edge)
        times.append(("host edge=%d" % edge, time.perf_counter() - t0))
        for name, a, b in zip(("distance", "gradient", "flags"), got, want):
            assert _same_nan(a, b), ("host", name, edge, _differences(a, b))
    assert np.isfinite(want[0][:len(deep)]).all() and (want[2] == 0).any()
    del f, dp
    torch.cuda.empty_cache()
    _line("point queries (%d points)" % n, shape, times, peak)


# ---- G. host to host ------------------------------------------------------------------------------------------------------------------
def _host_available_bytes():
    with open("/proc/meminfo") as fh:
        for line in fh:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


@gpu_test
def test_host_bits_build_past_2_31_voxels(big):
    """sdfgpu_build_bits at 3072 x 1024 x 1024 on the point lattice: 384 MiB of host bits in, 12 GiB of host floats out through the
    staged upload and download (offsets of up to 12 GiB).  The host field equals the device-resident build of the same bits, which
    is checked against the closed form on every voxel; the extrema equal too."""
    import torch
    shape, res = BIG, 0.01
    nx, ny, nz = shape
    n = math.prod(shape)
    need = 4 * n + n // 8 + (6 << 30)
    have = _host_available_bytes()
    if have < need:
        pytest.skip("needs %.1f GB of free host memory, %.1f GB are available" % (need / 1e9, have / 1e9))
    dev, stream = _device()
    torch.cuda.empty_cache()
    base = _used_device_bytes()
    row = (np.arange(nz) % STRIDES[2] == 0).astype(np.uint8)
    bits = np.zeros((nx, ny, nz // 32), np.uint32)
    bits[0::STRIDES[0], 0::STRIDES[1], :] = capi.pack_bits_host(row)
    d_bits = torch.from_numpy(bits.view(np.int32)).to(dev)
    assert bool(torch.equal(d_bits, _lattice_bits(shape, False, dev)))
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    big.set_option("policy_reset", 1)
    t_dev = _timed(lambda: big.build_bits_device(d_bits.data_ptr(), shape, out.data_ptr(), res, True, stream))
    ext = big.get_extrema()
    del d_bits
    assert ext == _lattice_check(shape, False, True, res, out)
    t0 = time.perf_counter()
    host, host_ext = big.build_bits(bits.reshape(-1), shape, res, True)
    t_host = time.perf_counter() - t0
    peak = _used_device_bytes() - base
    assert host_ext == ext, (host_ext, ext)
    for x0 in range(0, nx, 128):
        got = torch.from_numpy(host[x0:x0 + 128]).to(dev).view(torch.int32)
        want = out[x0:x0 + 128].view(torch.int32)
        if not bool(torch.equal(got, want)):
            bad = (got != want).nonzero()[:3].tolist()
            raise AssertionError("x chunk %d: %d voxels of the host field differ, first %s" % (
                x0, int((got != want).sum()), [[v[0] + x0] + v[1:] for v in bad]))
    del out, host
    torch.cuda.empty_cache()
    _line("host bits build", shape, [("device", t_dev), ("host to host", t_host)], peak)
