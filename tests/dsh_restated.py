"""The contract of the dynamic spatial hashed map (include/sdfgpu.h "Dynamic spatial hashed map") restated in
Python: a dict of chunks with numpy arrays, index arithmetic in float64 and int64, operations applied one at a time in list order.
It is the judge of tests/test_gpu_dsh*.py.  Records are uint64 and are compared as bytes; nothing here runs on a GPU.

The contract is this project's own (arc_utilities' DynamicSpatialHashedVoxelGrid is not available to it): UNVERIFIED against that class."""
import numpy as np

NOT_FOUND, FOUND_IN_CHUNK, FOUND_IN_CELL = 0, 1, 2
NOT_SET, SET_CHUNK, SET_CELL = 0, 1, 2
CHUNK_BIAS = 1 << 20
MAX_CHUNK_CELLS = 32768
EMPTY_KEY = (1 << 64) - 1


def record(occupancy, component=0):
    """COLLISION_CELL {float occupancy; uint32 component} -> the uint64 the map moves (occupancy in the low word)"""
    return int(np.array([occupancy], np.float32).view(np.uint32)[0]) | (int(component) & 0xFFFFFFFF) << 32


def record_bits(occupancy_bits, component=0):
    return (int(occupancy_bits) & 0xFFFFFFFF) | (int(component) & 0xFFFFFFFF) << 32


def occupancy(records):
    return (np.asarray(records, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)


def floor_div(i, n):
    """floor(i / n) for n > 0 on Python ints (whose // already floors) -- spelt out as the C code must"""
    q = abs(i) // n
    if i >= 0:
        return q
    return -q - (1 if abs(i) % n else 0)


def pack_key(c):
    cx, cy, cz = (int(v) + CHUNK_BIAS for v in c)
    assert all(0 <= v < (1 << 21) for v in (cx, cy, cz))
    return cx << 42 | cy << 21 | cz


def unpack_key(key):
    return ((key >> 42) - CHUNK_BIAS, ((key >> 21) & 0x1FFFFF) - CHUNK_BIAS, (key & 0x1FFFFF) - CHUNK_BIAS)


def chunk_in_range(c):
    return -CHUNK_BIAS <= c < CHUNK_BIAS


def classify(records, unknown_is_filled):
    """the CollisionMapGrid predicate on records"""
    occ = occupancy(records)
    return (occ > np.float32(0.5)) | (bool(unknown_is_filled) & (occ == np.float32(0.5)))


def pack_bits(filled):
    f = np.asarray(filled, bool).reshape(-1)
    padded = np.zeros((f.size + 31) // 32 * 32, np.uint8)
    padded[:f.size] = f
    return np.packbits(padded.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint32)


class Map:
    def __init__(self, inverse_origin=None, cell_size=1.0, chunk_dims=(16, 16, 16), default=0):
        self.inverse = np.eye(4) if inverse_origin is None else np.array(inverse_origin, np.float64).reshape(4, 4)
        assert cell_size > 0 and np.isfinite(cell_size)
        self.inv_cell = np.float64(1.0) / np.float64(cell_size)
        self.n = tuple(int(v) for v in chunk_dims)
        assert all(v >= 1 for v in self.n) and int(np.prod(self.n)) <= MAX_CHUNK_CELLS
        self.default = int(default)
        self.chunks = {}                 # (c_x, c_y, c_z) -> ("chunk", record) | ("cells", uint64 [n_x, n_y, n_z])
        self.components_valid = False

    # ---- location -> cell ---------------------------------------------------------------------------------------------------------
    def global_cell(self, p):
        """the global cell index of a location as Python ints, or None for an invalid one"""
        p = np.asarray(p, np.float64)
        if not np.all(np.isfinite(p)):
            return None
        out = []
        with np.errstate(all="ignore"):
            for a in range(3):
                m = self.inverse[a]
                g = ((m[0] * p[0] + m[1] * p[1]) + m[2] * p[2]) + m[3]           # separate float64 products and sums, this order
                v = np.floor(g * self.inv_cell)
                if not np.isfinite(v) or not chunk_in_range(floor_div(int(v), self.n[a])):
                    return None
                out.append(int(v))
        return tuple(out)

    def split(self, i):
        c = tuple(floor_div(i[a], self.n[a]) for a in range(3))
        return c, tuple(i[a] - c[a] * self.n[a] for a in range(3))

    # ---- the three calls -------------------------------------------------------------------------------------------------------------
    def get_cell(self, i):
        c, l = self.split(i)
        if not all(chunk_in_range(v) for v in c) or c not in self.chunks:
            return self.default, NOT_FOUND
        kind, what = self.chunks[c]
        return (int(what), FOUND_IN_CHUNK) if kind == "chunk" else (int(what[l]), FOUND_IN_CELL)

    def get(self, p):
        i = self.global_cell(p)
        return (self.default, NOT_FOUND) if i is None else self.get_cell(i)

    def set_cell(self, p, value):
        i = self.global_cell(p)
        if i is None:
            return NOT_SET
        c, l = self.split(i)
        kind, what = self.chunks.get(c, ("chunk", self.default))
        if kind == "chunk":
            what = np.full(self.n, what, np.uint64)
            self.chunks[c] = ("cells", what)
        what[l] = np.uint64(value)
        self.components_valid = False
        return SET_CELL

    def set_chunk(self, p, value):
        i = self.global_cell(p)
        if i is None:
            return NOT_SET
        self.chunks[self.split(i)[0]] = ("chunk", int(value))
        self.components_valid = False
        return SET_CHUNK

    # ---- batches: one after the other, in list order ------------------------------------------------------------------------------
    def _values(self, value, n):
        return [int(value)] * n if np.ndim(value) == 0 else [int(v) for v in np.asarray(value, np.uint64).reshape(-1)]

    def set_cells(self, locations, value):
        loc = np.asarray(locations, np.float64).reshape(-1, 3)
        return np.array([self.set_cell(p, v) for p, v in zip(loc, self._values(value, len(loc)))], np.uint8)

    def set_chunks(self, locations, value):
        loc = np.asarray(locations, np.float64).reshape(-1, 3)
        return np.array([self.set_chunk(p, v) for p, v in zip(loc, self._values(value, len(loc)))], np.uint8)

    def insert_points(self, points, value):
        return self.set_cells(np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64), value)

    def get_batch(self, locations):
        loc = np.asarray(locations, np.float64).reshape(-1, 3)
        got = [self.get(p) for p in loc]
        return np.array([g[0] for g in got], np.uint64), np.array([g[1] for g in got], np.uint8)

    # ---- window and export -------------------------------------------------------------------------------------------------------------
    def window(self, lower, shape):
        """records uint64 [nx, ny, nz]: voxel (x, y, z) is Get at global cell lower + (x, y, z)"""
        out = np.empty(shape, np.uint64)
        for x in range(shape[0]):
            for y in range(shape[1]):
                for z in range(shape[2]):
                    out[x, y, z] = self.get_cell((int(lower[0]) + x, int(lower[1]) + y, int(lower[2]) + z))[0]
        return out

    def export(self):
        """(list of (c, state, record, first_cell) in ascending (c_x, c_y, c_z) order, cells uint64 [cell-filled chunks, n_x, n_y, n_z])"""
        chunks, cells = [], []
        for c in sorted(self.chunks):
            kind, what = self.chunks[c]
            if kind == "chunk":
                chunks.append((c, FOUND_IN_CHUNK, int(what), -1))
            else:
                chunks.append((c, FOUND_IN_CELL, 0, len(cells) * int(np.prod(self.n))))
                cells.append(what)
        return chunks, (np.stack(cells) if cells else np.zeros((0,) + self.n, np.uint64))

    def counts(self):
        kinds = [k for k, _ in self.chunks.values()]
        return kinds.count("chunk"), kinds.count("cells")

    # ---- display points (in double, as the C++ class computes them) ------------------------------------------------------------------------
    def grid_to_world(self, origin, g):
        """origin (4 x 4, the map's origin transform) times a grid-frame point, rows as ((m0 x + m1 y) + m2 z) + m3"""
        m = np.asarray(origin, np.float64).reshape(4, 4)
        return np.array([((m[a, 0] * g[0] + m[a, 1] * g[1]) + m[a, 2] * g[2]) + m[a, 3] for a in range(3)], np.float64)

    def cell_centre(self, origin, cell_size, i):
        cs = np.float64(cell_size)
        return self.grid_to_world(origin, [(np.float64(v) + 0.5) * cs for v in i])

    def chunk_centre(self, origin, cell_size, c):
        cs = np.float64(cell_size)
        return self.grid_to_world(origin, [(np.float64(c[a] * self.n[a]) + 0.5 * np.float64(self.n[a])) * cs for a in range(3)])
