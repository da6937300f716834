"""The shape rasteriser's decision procedure (include/sdfgpu.h "Shape rasteriser", sdf_tools_amd/csrc/sdfgpu_scene.hpp) restated in
numpy float64: operation for operation what sc_sphere, sc_box and sc_cylinder do, shortcuts included, vectorised over the voxels.
numpy never fuses a product with a sum, so the parenthesisation below is the rounding order.

What is NOT restated is the culling: a shape's world bounds inflated by the resolution against the bounds of a region's centres.
The slack (res - sqrt(3) res / 2 = 0.13 res) is many orders above the rounding of either side, so the culling changes no voxel;
restated() evaluates every shape at every voxel whose centre lies inside the same inflated bounds and nowhere else, which is the
same statement (the bounds test itself is repeated here with numpy's rounding, a difference only for centres within rounding of a
bound that is 0.13 res away from any cube that can touch the shape).

restated() returns the byte mask, the first-hit object ids and the packed bit field."""
import numpy as np

BOX, SPHERE, CYLINDER = 1, 2, 3


def centres(origin, res, shape):
    """[n, 3] world centres in linear order: origin * (res (x + .5), res (y + .5), res (z + .5), 1), rows as ((m0 v0 + m1 v1) + m2 v2) + m3"""
    o = np.asarray(origin, np.float64).reshape(4, 4)
    nx, ny, nz = shape
    x, y, z = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nz, dtype=np.float64), indexing="ij")
    g0, g1, g2 = res * (x.reshape(-1) + 0.5), res * (y.reshape(-1) + 0.5), res * (z.reshape(-1) + 0.5)
    return np.stack([((o[r, 0] * g0 + o[r, 1] * g1) + o[r, 2] * g2) + o[r, 3] for r in range(3)], 1)


def centres_of(origin, res, shape, linear):
    """the same for chosen linear indices (int64 array) of a grid that may be too large to enumerate"""
    o = np.asarray(origin, np.float64).reshape(4, 4)
    nx, ny, nz = shape
    v = np.asarray(linear, np.int64)
    t = v // nz
    z, x = v - t * nz, t // ny
    y = t - x * ny
    g0, g1, g2 = res * (x.astype(np.float64) + 0.5), res * (y.astype(np.float64) + 0.5), res * (z.astype(np.float64) + 0.5)
    return np.stack([((o[r, 0] * g0 + o[r, 1] * g1) + o[r, 2] * g2) + o[r, 3] for r in range(3)], 1)


def shape_valid(kind, dims, pose):
    nd = {BOX: 3, SPHERE: 1, CYLINDER: 2}.get(int(kind))
    if nd is None:
        return False
    d, p = np.asarray(dims, np.float64).reshape(-1), np.asarray(pose, np.float64).reshape(-1)
    return bool(np.isfinite(d[:nd]).all() and (d[:nd] >= 0.0).all() and np.isfinite(p[:12]).all())


def half_extents(kind, dims, pose):
    p = np.abs(np.asarray(pose, np.float64).reshape(4, 4))
    if kind == SPHERE:
        return np.array([dims[0]] * 3, np.float64)
    d = (dims[0] * 0.5, dims[1] * 0.5, dims[2] * 0.5) if kind == BOX else (dims[1], dims[1], dims[0] * 0.5)
    return np.array([(p[a, 0] * d[0] + p[a, 1] * d[1]) + p[a, 2] * d[2] for a in range(3)])


def sphere(dims, pose, c, h):
    p = np.asarray(pose, np.float64).reshape(4, 4)
    total = np.zeros(len(c))
    for a in range(3):
        d = np.maximum(np.abs(c[:, a] - p[a, 3]) - h, 0.0)
        total = total + d * d
    return total <= dims[0] * dims[0]


def box(dims, pose, c, h):
    p = np.asarray(pose, np.float64).reshape(4, 4)
    b = [dims[0] * 0.5, dims[1] * 0.5, dims[2] * 0.5]
    R, A = p[:3, :3], np.abs(p[:3, :3])
    t = [p[a, 3] - c[:, a] for a in range(3)]
    ok = np.ones(len(c), bool)
    for a in range(3):
        ok &= ~(np.abs(t[a]) > h + ((b[0] * A[a, 0] + b[1] * A[a, 1]) + b[2] * A[a, 2]))
    for j in range(3):
        tl = (t[0] * R[0, j] + t[1] * R[1, j]) + t[2] * R[2, j]
        ok &= ~(np.abs(tl) > h * ((A[0, j] + A[1, j]) + A[2, j]) + b[j])
    for a in range(3):
        a1, a2 = (a + 1) % 3, (a + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            tl = t[a2] * R[a1, j] - t[a1] * R[a2, j]
            rc = h * (A[a2, j] + A[a1, j])
            rb = b[j1] * A[a, j2] + b[j2] * A[a, j1]
            ok &= ~(np.abs(tl) > rc + rb)
    return ok


def _segment_dsq(ax, ay, bx, by):
    ex, ey = bx - ax, by - ay
    ee = ex * ex + ey * ey
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ee > 0.0, np.minimum(np.maximum(-(ax * ex + ay * ey) / ee, 0.0), 1.0), 0.0)
    qx, qy = ax + t * ex, ay + t * ey
    return qx * qx + qy * qy


def _clip(poly, count, sign, bound):
    """sc_clip over rows: poly [m, k, 3], count [m] -> (out [m, k + 1, 3], counts)"""
    m, k, _ = poly.shape
    out = np.zeros((m, k + 1, 3))
    n_out = np.zeros(m, np.int64)
    rows = np.arange(m)
    plane = sign * bound
    for i in range(k):
        live = i < count
        cur = poly[:, i]
        prv = poly[rows, np.where(i == 0, np.maximum(count - 1, 0), i - 1)]
        cin, pin = sign * cur[:, 2] <= bound, sign * prv[:, 2] <= bound
        cut = live & (cin != pin)
        if cut.any():
            r = rows[cut]
            u = (plane - prv[r, 2]) / (cur[r, 2] - prv[r, 2])
            out[r, n_out[r], 0] = prv[r, 0] + u * (cur[r, 0] - prv[r, 0])
            out[r, n_out[r], 1] = prv[r, 1] + u * (cur[r, 1] - prv[r, 1])
            out[r, n_out[r], 2] = plane
            n_out[r] += 1
        keep = live & cin
        if keep.any():
            r = rows[keep]
            out[r, n_out[r]] = cur[r]
            n_out[r] += 1
    return out, n_out


def cylinder(dims, pose, c, h):
    p = np.asarray(pose, np.float64).reshape(4, 4)
    hz, r = dims[0] * 0.5, dims[1]
    r2 = r * r
    d = [c[:, a] - p[a, 3] for a in range(3)]
    q = [(p[0, j] * d[0] + p[1, j] * d[1]) + p[2, j] * d[2] for j in range(3)]
    rho2 = q[0] * q[0] + q[1] * q[1]
    reach = 1.75 * h
    rr = r + reach
    rejected = (np.abs(q[2]) - hz > reach) | (rho2 > rr * rr)
    accepted = ~rejected & (np.abs(q[2]) <= hz) & (rho2 <= r2)
    result = accepted.copy()
    shell = np.flatnonzero(~rejected & ~accepted)
    if not len(shell):
        return result
    cs = c[shell]
    v = np.zeros((len(shell), 8, 3))
    for k in range(8):
        w = [(cs[:, a] + (h if (k >> a) & 1 else -h)) - p[a, 3] for a in range(3)]
        for j in range(3):
            v[:, k, j] = (p[0, j] * w[0] + p[1, j] * w[1]) + p[2, j] * w[2]
    best = np.full(len(shell), 1.0e300)
    for f in range(6):
        a = f >> 1
        a1, a2, base = (a + 1) % 3, (a + 2) % 3, (f & 1) << a
        corner = [base, base | (1 << a1), base | (1 << a1) | (1 << a2), base | (1 << a2)]
        one, n1 = _clip(v[:, corner], np.full(len(shell), 4), -1.0, hz)
        two, n2 = _clip(one, n1, 1.0, hz)
        rows = np.arange(len(shell))
        for k in range(6):
            live = k < n2
            if not live.any():
                break
            prev = np.where(k == 0, np.maximum(n2 - 1, 0), k - 1)
            dsq = _segment_dsq(two[rows, prev, 0], two[rows, prev, 1], two[:, k, 0], two[:, k, 1])
            best = np.where(live, np.minimum(best, dsq), best)
    by_edges = best <= r2
    lo, hi = np.full(len(shell), -1.0), np.full(len(shell), 1.0)
    alive = np.ones(len(shell), bool)
    for a in range(3):
        g = hz * p[a, 2]
        da = d[a][shell]
        if g == 0.0:
            alive &= ~(np.abs(da) > h)
        else:
            s1, s2 = (da - h) / g, (da + h) / g
            lo = np.maximum(lo, np.minimum(s1, s2))
            hi = np.minimum(hi, np.maximum(s1, s2))
    result[shell] = by_edges | (alive & (lo <= hi))
    return result


def hit(kind, dims, pose, c, h):
    if kind == SPHERE:
        return sphere(dims, pose, c, h)
    if kind == BOX:
        return box(dims, pose, c, h)
    if kind == CYLINDER:
        return cylinder(dims, pose, c, h)
    raise ValueError("shape type %r is refused" % (kind,))


def hits_at(shapes, c, res):
    """first-hit object ids (0: none) of records `shapes` (capi.SHAPE_DTYPE) at world centres c [n, 3]"""
    h = res * 0.5
    ids = np.zeros(len(c), np.uint32)
    hit_any = np.zeros(len(c), bool)
    c_lo, c_hi = (c.min(0), c.max(0)) if len(c) else (np.zeros(3), np.zeros(3))
    for s in shapes:
        kind, dims, pose = int(s["type"]), [float(v) for v in s["dims"]], np.asarray(s["pose"], np.float64)
        if not shape_valid(kind, dims, pose):
            raise ValueError("shape type %r is refused" % (kind,))
        e, t = half_extents(kind, dims, pose), pose.reshape(4, 4)[:3, 3]
        if np.any(t + (e + res) < c_lo) or np.any(t - (e + res) > c_hi):
            continue
        near = ~hit_any
        for a in range(3):
            near &= (c[:, a] >= t[a] - (e[a] + res)) & (c[:, a] <= t[a] + (e[a] + res))
        idx = np.flatnonzero(near)
        if not len(idx):
            continue
        got = idx[hit(kind, dims, pose, c[idx], h)]
        ids[got] = s["object_id"]
        hit_any[got] = True
    return hit_any, ids


def pack_bits(mask):
    flat = np.asarray(mask, np.uint8).reshape(-1)
    padded = np.zeros((flat.size + 31) // 32 * 32, np.uint8)
    padded[:flat.size] = flat
    return np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


def restated(shapes, origin, res, shape):
    """(mask uint8 [nx, ny, nz], object ids uint32 [nx, ny, nz], bits uint32 [ceil(n / 32)])"""
    filled, ids = hits_at(shapes, centres(origin, res, shape), res)
    mask = filled.astype(np.uint8).reshape(shape)
    return mask, ids.reshape(shape), pack_bits(mask)
