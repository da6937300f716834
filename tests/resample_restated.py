"""Loader of tests/resample_restated.cpp, the yardstick of Resample (the contract's loop over VoxelGrid's public members), and the
scenes the Resample tests share.  Host code only: compiled once per process with g++ -O2 -ffp-contract=off against include/."""
import collections
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = []

Restated = collections.namedtuple("Restated", "cells written shape inverse inv_cell")


def _lib():
    if not _LIB:
        out = os.path.join(tempfile.mkdtemp(prefix="resample_restated_"), "resample_restated.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fPIC", "-shared",
                               "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "resample_restated.cpp"), "-o", out])
        L = ctypes.CDLL(out)
        d, i64, vp, ci = ctypes.c_double, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
        L.rr_resample.restype = ci
        L.rr_resample.argtypes = [ci, i64, i64, i64, d, vp, d, vp, vp, vp, vp, vp, vp, i64, vp, ctypes.c_char_p, ci]
        _LIB.append(L)
    return _LIB[0]


def as_records(a, cell_bytes):
    """any array of nx * ny * nz records -> uint8 [nx, ny, nz, cell_bytes] (the leading three axes are the grid's)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], a.shape[1], a.shape[2], cell_bytes)


def restated(cells, cell, origin, new_resolution, oob):
    """cells: uint8 [nx, ny, nz, cell_bytes]; cell: the source resolution; origin: 4 x 4; oob: cell_bytes bytes.  Returns
    Restated(cells uint8 [mx, my, mz, cell_bytes], written, (mx, my, mz), the result's inverse origin transform 4 x 4, its
    1 / cell sizes).  Raises ValueError where the grid's constructor throws std::invalid_argument."""
    L = _lib()
    cells = np.ascontiguousarray(cells, np.uint8)
    nx, ny, nz, cb = cells.shape
    o = np.ascontiguousarray(origin, np.float64).reshape(16)
    oob = np.ascontiguousarray(oob).view(np.uint8).reshape(-1)
    assert oob.size == cb
    dims, inv, inv_cell = np.zeros(3, np.int64), np.zeros(16, np.float64), np.zeros(3, np.float64)
    written = ctypes.c_uint64(0)
    msg = ctypes.create_string_buffer(256)

    def call(dst, cap):
        rc = L.rr_resample(cb, nx, ny, nz, float(cell), o.ctypes.data, float(new_resolution), cells.ctypes.data, oob.ctypes.data,
                           dims.ctypes.data, inv.ctypes.data, inv_cell.ctypes.data, dst, cap, ctypes.byref(written), msg, 256)
        if rc == 1:
            raise ValueError(msg.value.decode())
        assert rc in (0, 2), rc
        return rc
    # one pass when the guessed capacity (the constructor's ceil(size / resolution), one cell to spare per axis) holds the result
    cap = 1
    if new_resolution > 0.0 and math.isfinite(new_resolution):
        for n in (nx, ny, nz):
            cap *= int(math.ceil(n * float(cell) / float(new_resolution))) + 1
    buf = np.empty(cap * cb, np.uint8)
    if call(buf.ctypes.data, cap) == 2:
        buf = np.empty(int(np.prod(dims)) * cb, np.uint8)
        assert call(buf.ctypes.data, int(np.prod(dims))) == 0
    shape = tuple(int(v) for v in dims)
    out = buf[:int(np.prod(shape)) * cb].reshape(shape + (cb,)).copy()
    return Restated(out, int(written.value), shape, inv.reshape(4, 4).copy(), inv_cell.copy())


# ---- origins ----------------------------------------------------------------------------------------------------------------------
def quaternion_origin(q, t=(0.0, 0.0, 0.0)):
    """4 x 4 from a quaternion (w, x, y, z), normalised here, with Eigen's toRotationMatrix products, and a translation"""
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    m = np.eye(4)
    m[0, :3] = [1.0 - (tyy + tzz), txy - twz, txz + twy]
    m[1, :3] = [txy + twz, 1.0 - (txx + tzz), tyz - twx]
    m[2, :3] = [txz - twy, tyz + twx, 1.0 - (txx + tyy)]
    m[:3, 3] = t
    return m


def origins():
    """identity; a translation; a quarter turn about z from a quaternion (its entries carry residues of some 1e-16, so that source
    centres which sit exactly on a result cell boundary are placed by rounding noise); a general rotation with a translation"""
    ident = np.eye(4)
    trans = np.eye(4)
    trans[:3, 3] = (0.1, -0.37, 2.3)
    quarter = quaternion_origin((math.cos(math.pi / 4), 0.0, 0.0, math.sin(math.pi / 4)))
    general = quaternion_origin((0.83, -0.21, 0.4, 0.32), (-1.7, 0.45, 0.9))
    return {"identity": ident, "translation": trans, "quarter-turn": quarter, "general": general}


# ---- payloads ---------------------------------------------------------------------------------------------------------------------
OCCUPANCIES = np.array([0x00000000, 0x3F000000, 0x3F800000, 0x80000000, 0x7FC12345, 0xFFA00001, 0x3F000001, 0x3EFFFFFF], np.uint32)
#               0.0, 0.5, 1.0, -0.0, a quiet NaN with a payload, a signalling one, the neighbours of 0.5


def payload(shape, cell_bytes, seed=0):
    """uint8 [nx, ny, nz, cell_bytes]: 4 bytes: linear index + 1; 8 bytes: {an occupancy of OCCUPANCIES, linear index + 1};
    16 bytes: {occupancy, linear index + 1, a distinct object id, a distinct segment}"""
    n = int(np.prod(shape))
    lin = np.arange(1, n + 1, dtype=np.uint64)
    rng = np.random.default_rng(seed)
    w = np.zeros((n, cell_bytes // 4), np.uint32)
    if cell_bytes == 4:
        w[:, 0] = lin.astype(np.uint32)
    else:
        w[:, 0] = OCCUPANCIES[rng.integers(0, len(OCCUPANCIES), n)]
        w[:, 1] = lin.astype(np.uint32)
    if cell_bytes == 16:
        w[:, 2] = (lin * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32)
        w[:, 3] = (np.uint64(0xFFFFFFFF) - lin).astype(np.uint32)
    return w.view(np.uint8).reshape(tuple(shape) + (cell_bytes,))


def oob_record(cell_bytes):
    """a fill record that no payload holds: an occupancy NaN with a payload of its own and all-ones-ish words"""
    return np.array([0x7FDEAD01, 0xFEEDF00D, 0xCAFEBABE, 0x0BADC0DE][:cell_bytes // 4], np.uint32).view(np.uint8).copy()
