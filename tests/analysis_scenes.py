"""Scenes aimed at the analysis kernels' internal paths, and vectorised numpy restatements of the per-voxel and per-point queries.

Scenes (uint8 masks [nx, ny, nz], 1 = filled):
  serpentine   one one-voxel path through the whole grid (one component whose chain crosses every tile of cc_plan)
  comb         one-voxel teeth along an axis, joined only by the plane at that axis' last index
  stripes      one-voxel lines along an axis (every line its own component, crossing every tile face on its axis)
  checkerboard (x + y + z) % 2
  nested_shells a solid shell, a free cavity, a solid core
  tori_chain   square one-voxel rings, alternately in the xy and xz planes, linked into chains along x (genus 1 each)
colliding_labels(): labels that share one slot of k_tp_vertex's LDS table (sdfgpu_topology.hip).

Restatements (float64 arithmetic in the reference's order; numpy never fuses a product with a sum):
  grid_gradient     GetGridAlignedGradient over the whole grid (reference sdf.hpp:432-526)
  estimate_distance EstimateDistance at grid-frame points inside the grid (sdf.hpp:773-961)
tests/test_analysis_scenes_cpu.py pins them to the loop forms and to the host headers."""
import numpy as np

TABLE_SLOTS = 1024           # sdfgpu_topology.hip kTableSlots
TABLE_PROBES = 16            # kTableProbes


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def serpentine(shape):
    """Rows along z at every (even x, even y), visited in boustrophedon order; consecutive rows are joined by one voxel at the z
    end the walk leaves from (alternating ends).  Rows two apart never touch, so the whole path is one component."""
    nx, ny, nz = shape
    m = np.zeros(shape, np.uint8)
    rows = []
    for i, x in enumerate(range(0, nx, 2)):
        ys = list(range(0, ny, 2))
        rows += [(x, y) for y in (ys if i % 2 == 0 else ys[::-1])]
    for k, (x, y) in enumerate(rows):
        m[x, y, :] = 1
        if k + 1 < len(rows):
            x2, y2 = rows[k + 1]
            m[(x + x2) // 2, (y + y2) // 2, nz - 1 if k % 2 == 0 else 0] = 1
    return m


def comb(shape, axis=0):
    """Teeth along `axis` at every position whose other two coordinates are both even, joined only by the plane at the axis' last
    index.  Without that plane every tooth is its own component."""
    m = stripes(shape, axis)
    sl = [slice(None)] * 3
    sl[axis] = shape[axis] - 1
    m[tuple(sl)] = 1
    return m


def stripes(shape, axis=0):
    """One-voxel lines along `axis` at every position whose other two coordinates are both even."""
    idx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    a, b = [idx[k] for k in range(3) if k != axis]
    return ((a % 2 == 0) & (b % 2 == 0)).astype(np.uint8)


def checkerboard(shape):
    x, y, z = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    return ((x + y + z) % 2).astype(np.uint8)


def nested_shells(shape, wall=1):
    """A box shell of thickness `wall` at the grid's faces, a free cavity, and a solid core (where the grid is large enough)."""
    m = np.ones(shape, np.uint8)
    lo, hi = [wall] * 3, [s - wall for s in shape]
    if all(h > l for l, h in zip(lo, hi)):
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 0
        clo, chi = [l + 2 for l in lo], [h - 2 for h in hi]
        if all(h > l for l, h in zip(clo, chi)):
            m[clo[0]:chi[0], clo[1]:chi[1], clo[2]:chi[2]] = 1
    return m


def _ring(m, x0, y0, z0, plane, side=7):
    """A square one-voxel ring with corner (x0, y0, z0) and `side` voxels per edge, in the xy or the xz plane."""
    s = side - 1
    if plane == "xy":
        m[x0:x0 + side, y0, z0] = m[x0:x0 + side, y0 + s, z0] = 1
        m[x0, y0:y0 + side, z0] = m[x0 + s, y0:y0 + side, z0] = 1
    else:
        m[x0:x0 + side, y0, z0] = m[x0:x0 + side, y0, z0 + s] = 1
        m[x0, y0, z0:z0 + side] = m[x0 + s, y0, z0:z0 + side] = 1


def tori_chain(shape, offset=0):
    """Linked square rings (side 7): xy rings at x = offset + 8 k, xz rings at x = offset + 8 k + 4, chains repeated over y and z.
    No two rings touch; each is one component with one hole.  Rings that would not fit are left out."""
    nx, ny, nz = shape
    m = np.zeros(shape, np.uint8)
    for yc in range(3, ny - 3, 9):
        for zc in range(3, nz - 3, 9):
            x = offset
            k = 0
            while x + 7 <= nx:
                if k % 2 == 0:
                    _ring(m, x, yc - 3, zc, "xy")
                else:
                    _ring(m, x, yc, zc - 3, "xz")
                x += 4
                k += 1
    return m


def colliding_labels(count, start=1, limit=1 << 24, slot=None):
    """`count` labels >= start whose k_tp_vertex table slot (c * 2654435761 mod 2^32) >> 22 is the same (the slot of `start`
    unless given).  Returns (labels, slot)."""
    if slot is None:
        slot = table_slot(start)
    c = np.arange(start, limit, dtype=np.uint64)
    hit = c[table_slot(c) == slot][:count]
    if len(hit) < count:
        raise ValueError("not enough colliding labels below the limit")
    return hit.astype(np.uint32), int(slot)


def table_slot(c):
    return ((np.asarray(c, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)


# ---- restatements ------------------------------------------------------------------------------------------------------------------
def grid_gradient(sdf, res, edge=True):
    """GetGridAlignedGradient at every voxel as float64 [nx, ny, nz, 3]; NaN where the reference returns no gradient (the boundary
    shell with edge gradients off).  Interior: fp32 difference times 1 / (2 res) in double; shell: double difference over the
    clamped interval (0 on a singleton axis)."""
    f = np.ascontiguousarray(sdf, np.float32)
    shape = f.shape
    out = np.empty(shape + (3,), np.float64)
    idx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    interior = np.ones(shape, bool)
    for ax, n in enumerate(shape):
        interior &= (idx[ax] > 0) & (idx[ax] < n - 1)
    inv2 = 1.0 / (2.0 * res)
    with np.errstate(invalid="ignore", over="ignore"):
        for ax, n in enumerate(shape):
            i = idx[ax]
            lo, hi = np.maximum(i - 1, 0), np.minimum(i + 1, n - 1)
            il, ih = list(idx), list(idx)
            il[ax], ih[ax] = lo, hi
            fl, fh = f[tuple(il)], f[tuple(ih)]
            inner = (fh - fl).astype(np.float64) * inv2
            w = hi - lo
            inc = w.astype(np.float64) * res
            with np.errstate(divide="ignore"):
                shell = np.where(w > 0, (fh.astype(np.float64) - fl.astype(np.float64)) * (1.0 / inc), 0.0)
            out[..., ax] = np.where(interior, inner, shell if edge else np.nan)
    return out


def axis_pairs(idx, off, n):
    """The neighbour pair of one axis (sdf.hpp:798-833): toward the offset's side, shifted inward at a grid face, collapsed on a
    singleton axis."""
    up = off >= 0.0
    lower = np.where(up, idx, idx - 1)
    upper = np.where(up, idx + 1, idx)
    face_hi = up & (upper >= n)
    lower = np.where(face_hi, idx - 1, lower)
    upper = np.where(face_hi, idx, upper)
    face_lo = ~up & (lower < 0)
    upper = np.where(face_lo, idx + 1, upper)
    lower = np.where(face_lo, idx, lower)
    lower = np.where(face_hi & (lower < 0), idx, lower)
    upper = np.where(face_lo & (upper >= n), idx, upper)
    return lower, upper


def estimate_distance(sdf, res, g):
    """EstimateDistance at grid-frame points g [n, 3] (float64) whose cells lie inside the grid."""
    f = np.asarray(sdf, np.float32)
    g = np.asarray(g, np.float64)
    idx = np.floor(g * (1.0 / res)).astype(np.int64)
    lower, upper = np.empty_like(idx), np.empty_like(idx)
    for ax in range(3):
        off = g[:, ax] - res * (idx[:, ax] + 0.5)
        lower[:, ax], upper[:, ax] = axis_pairs(idx[:, ax], off, f.shape[ax])
    half = res * 0.5

    def D(ix, iy, iz):                                      # :773-796
        d = f[ix, iy, iz].astype(np.float64)
        return np.where(d >= 0.0, d - half, d + half)

    lo_loc = res * (lower + 0.5)
    x0, y0, z0 = lower.T
    x1, y1, z1 = upper.T

    def bilinear(ll, lh, hl, hh):                           # :699-727 with the corner at lo_loc, side = res
        l1, h1, l2, h2 = lo_loc[:, 0], lo_loc[:, 0] + res, lo_loc[:, 1], lo_loc[:, 1] + res
        mult = 1.0 / ((h1 - l1) * (h2 - l2))
        a0, a1 = mult * (h1 - g[:, 0]), mult * (g[:, 0] - l1)
        return (a0 * ll + a1 * hl) * (h2 - g[:, 1]) + (a0 * lh + a1 * hh) * (g[:, 1] - l2)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mz = bilinear(D(x0, y0, z0), D(x0, y1, z0), D(x1, y0, z0), D(x1, y1, z0))
        pz = bilinear(D(x0, y0, z1), D(x0, y1, z1), D(x1, y0, z1), D(x1, y1, z1))
        return mz + (g[:, 2] - lo_loc[:, 2]) * ((pz - mz) * (1.0 / res))    # :745-771


def query_points(sdf, res, g, oob=np.inf, edge=False):
    """sdfgpu_query_points at grid-frame points g [n, 3] with an identity rotation: (distance [n], gradient [n, 3], flags [n]).  The
    rotation is applied all the same, as the kernel and the host's GetGradient do: a NaN component spreads to the others."""
    g = np.asarray(g, np.float64)
    n = len(g)
    dist = np.full(n, oob, np.float64)
    grad = np.full((n, 3), np.nan)
    flags = np.zeros(n, np.uint8)
    with np.errstate(invalid="ignore"):
        fi = np.floor(g * (1.0 / res))
        inside = np.all(fi >= 0.0, axis=1) & np.all(fi < np.asarray(sdf.shape, np.float64), axis=1)
    if inside.any():
        dist[inside] = estimate_distance(sdf, res, g[inside])
        idx = fi[inside].astype(np.int64)
        full = grid_gradient(sdf, res, edge)[idx[:, 0], idx[:, 1], idx[:, 2]]
        R = np.eye(3)                                       # rotated into the world frame as r0 g0 + r1 g1 + r2 g2 (0 * NaN is NaN)
        with np.errstate(invalid="ignore"):
            grad[inside] = np.stack([R[i, 0] * full[:, 0] + R[i, 1] * full[:, 1] + R[i, 2] * full[:, 2] for i in range(3)], 1)
        have = np.ones(len(idx), bool) if edge else _interior(idx, sdf.shape)     # (an interior gradient may be NaN: inf - inf)
        flags[inside] = 1 | np.where(have, 2, 0).astype(np.uint8)
    return dist, grad, flags


def _interior(idx, shape):
    return np.all(idx > 0, axis=1) & np.all(idx < np.asarray(shape) - 1, axis=1)
