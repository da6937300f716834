// convex_segments_restated.cpp -- test infrastructure, never on the product path: a plain restatement of the reference's
// SignedDistanceField::ComputeLocalExtremaMap (src/sdf_tools/sdf.cpp:23-207) and TaggedObjectCollisionMapGrid::UpdateConvexSegments
// (src/sdf_tools/tagged_object_collision_map.cpp:552-654 over topology_computation.hpp:25-150) on flat arrays, which the GPU
// results are compared with bit for bit.
//
// Local extrema, as the reference walks them: cells are visited x -> y -> z; a cell whose stored extremum is not the sentinel
// (-inf, -inf, -inf) is skipped; a cell whose gradient is "effectively flat" (every |component| <= res * 0.06125) is its own
// extremum; otherwise the walk steps one cell at a time along the sign-corrected gradient (negated inside obstacles: sdf < 0),
// remembering the cells of its path in a hash set, until it
//   - steps onto a cell already on its path          -> that cell's location,
//   - steps out of the grid                           -> (+inf, +inf, +inf),
//   - steps onto a cell whose extremum is stored      -> the stored extremum,
//   - steps onto a cell whose gradient is flat        -> that cell's location,
// and then stores the result in every cell of its path.  The gradient is GetGradient(x, y, z, enable_edge_gradients = true):
// central differences (float subtraction, double scale) inside, clamped one-sided differences (double subtraction) on the
// boundary shell, rotated by q * ((0, g) * q^-1) with eigen_lite's Quaterniond arithmetic.  Locations are grid-frame cell
// centres, res * (i + 0.5).
//
// Convex segments: a cell takes part when (occupancy < 0.5f || object_id > 0) and its extremum is finite; the reference's
// scan-order breadth-first search joins two face neighbours that take part, carry the same object id and whose extrema lie
// closer than connected_threshold ((e1 - e2).norm(): 0 + dx dx + dy dy + dz dz, then sqrt).  Segments are numbered 1..K in scan
// order; other cells get 0.
//
// Compile without contraction (g++ -ffp-contract=off): the reference's products and sums are separate roundings.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <limits>
#include <unordered_map>
#include <vector>

namespace {

struct Quat {
    double w, x, y, z;
};

// eigen_lite.hpp Quaterniond::operator*, term by term in the same order
Quat mul(const Quat& a, const Quat& o) {
    return Quat{a.w * o.w - a.x * o.x - a.y * o.y - a.z * o.z, a.w * o.x + a.x * o.w + a.y * o.z - a.z * o.y,
                a.w * o.y - a.x * o.z + a.y * o.w + a.z * o.x, a.w * o.z + a.x * o.y - a.y * o.x + a.z * o.w};
}

Quat inverse(const Quat& q) {
    const double n = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
    return Quat{q.w / n, -q.x / n, -q.y / n, -q.z / n};
}

struct Idx {
    int64_t x, y, z;
    bool operator==(const Idx& o) const { return x == o.x && y == o.y && z == o.z; }
};

struct IdxHash {
    size_t operator()(const Idx& i) const {
        return std::hash<int64_t>()(((i.x + 1) << 42) ^ ((i.y + 1) << 21) ^ (i.z + 1));
    }
};

struct Field {
    const float* f;
    int64_t nx, ny, nz;
    double res;
    Quat q, qi;

    bool in(const Idx& i) const { return i.x >= 0 && i.y >= 0 && i.z >= 0 && i.x < nx && i.y < ny && i.z < nz; }
    float at(int64_t x, int64_t y, int64_t z) const { return f[(x * ny + y) * nz + z]; }
    int64_t lin(const Idx& i) const { return (i.x * ny + i.y) * nz + i.z; }

    // GetGradient(x, y, z, true)
    void gradient(const Idx& i, double g[3]) const {
        const int64_t x = i.x, y = i.y, z = i.z;
        double gx, gy, gz;
        if (x > 0 && y > 0 && z > 0 && x < nx - 1 && y < ny - 1 && z < nz - 1) {
            const double inv_twice_resolution = 1.0 / (2.0 * res);
            gx = (at(x + 1, y, z) - at(x - 1, y, z)) * inv_twice_resolution;
            gy = (at(x, y + 1, z) - at(x, y - 1, z)) * inv_twice_resolution;
            gz = (at(x, y, z + 1) - at(x, y, z - 1)) * inv_twice_resolution;
        } else {
            const int64_t lx = x - 1 < 0 ? 0 : x - 1, hx = x + 1 > nx - 1 ? nx - 1 : x + 1;
            const int64_t ly = y - 1 < 0 ? 0 : y - 1, hy = y + 1 > ny - 1 ? ny - 1 : y + 1;
            const int64_t lz = z - 1 < 0 ? 0 : z - 1, hz = z + 1 > nz - 1 ? nz - 1 : z + 1;
            const double ix = (double)(hx - lx) * res, iy = (double)(hy - ly) * res, iz = (double)(hz - lz) * res;
            gx = gy = gz = 0.0;
            if (ix > 0.0) gx = ((double)at(hx, y, z) - (double)at(lx, y, z)) * (1.0 / ix);
            if (iy > 0.0) gy = ((double)at(x, hy, z) - (double)at(x, ly, z)) * (1.0 / iy);
            if (iz > 0.0) gz = ((double)at(x, y, hz) - (double)at(x, y, lz)) * (1.0 / iz);
        }
        const Quat r = mul(q, mul(Quat{0.0, gx, gy, gz}, qi));
        g[0] = r.x; g[1] = r.y; g[2] = r.z;
    }

    bool flat(const double g[3]) const {
        const double s = res * 0.06125;
        return std::abs(g[0]) <= s && std::abs(g[1]) <= s && std::abs(g[2]) <= s;
    }

    Idx next(const Idx& i, const double g[3]) const {
        double w[3] = {g[0], g[1], g[2]};
        if (at(i.x, i.y, i.z) < 0.0) { w[0] = g[0] * -1.0; w[1] = g[1] * -1.0; w[2] = g[2] * -1.0; }
        const double s = res * 0.06125;
        Idx n = i;
        if (w[0] > s) n.x++; else if (w[0] < -s) n.x--;
        if (w[1] > s) n.y++; else if (w[1] < -s) n.y--;
        if (w[2] > s) n.z++; else if (w[2] < -s) n.z--;
        return n;
    }

    void loc(const Idx& i, double* e) const {
        e[0] = res * ((double)i.x + 0.5); e[1] = res * ((double)i.y + 0.5); e[2] = res * ((double)i.z + 0.5);
    }
};

const double kNegInf = -std::numeric_limits<double>::infinity();
const double kInf = std::numeric_limits<double>::infinity();

bool stored(const double* e) { return e[0] != kNegInf && e[1] != kNegInf && e[2] != kNegInf; }

void follow(const Field& F, double* map, const Idx& start) {
    if (stored(map + 3 * F.lin(start))) return;
    double g[3];
    F.gradient(start, g);
    if (F.flat(g)) { F.loc(start, map + 3 * F.lin(start)); return; }
    std::unordered_map<Idx, int8_t, IdxHash> path;
    Idx cur = start;
    path[cur] = 1;
    double e[3] = {kNegInf, kNegInf, kNegInf};
    for (;;) {
        cur = F.next(cur, g);
        if (path[cur] != 0) { F.loc(cur, e); break; }
        if (!F.in(cur)) { e[0] = e[1] = e[2] = kInf; break; }
        path[cur] = 1;
        const double* s = map + 3 * F.lin(cur);
        if (stored(s)) { e[0] = s[0]; e[1] = s[1]; e[2] = s[2]; break; }
        F.gradient(cur, g);
        if (F.flat(g)) { F.loc(cur, e); break; }
    }
    for (const auto& kv : path) {
        if (!F.in(kv.first)) continue;                  // (SetValue out of the grid does nothing)
        double* d = map + 3 * F.lin(kv.first);
        d[0] = e[0]; d[1] = e[1]; d[2] = e[2];
    }
}

}  // namespace

extern "C" {

// sdf: float [nx][ny][nz]; q: (w, x, y, z) of the origin rotation; out: double [nx][ny][nz][3]
int cx_extrema_restated(const float* sdf, int64_t nx, int64_t ny, int64_t nz, double res, const double* q, double* out) {
    Field F{sdf, nx, ny, nz, res, Quat{q[0], q[1], q[2], q[3]}, Quat{}};
    F.qi = inverse(F.q);
    const int64_t n = nx * ny * nz;
    for (int64_t i = 0; i < 3 * n; ++i) out[i] = kNegInf;
    for (int64_t x = 0; x < nx; ++x)
        for (int64_t y = 0; y < ny; ++y)
            for (int64_t z = 0; z < nz; ++z) follow(F, out, Idx{x, y, z});
    return 0;
}

// occupancy, object_id: [nx][ny][nz]; extrema: double [nx][ny][nz][3]; labels: uint32 out; returns K
uint32_t cx_segments_restated(const float* occupancy, const uint32_t* object_id, const double* extrema, int64_t nx, int64_t ny,
                              int64_t nz, double connected_threshold, uint32_t* labels) {
    const int64_t n = nx * ny * nz;
    auto in = [&](int64_t x, int64_t y, int64_t z) { return x >= 0 && y >= 0 && z >= 0 && x < nx && y < ny && z < nz; };
    auto lin = [&](int64_t x, int64_t y, int64_t z) { return (x * ny + y) * nz + z; };
    auto component = [&](int64_t x, int64_t y, int64_t z) -> int64_t {     // get_component_fn
        if (!in(x, y, z)) return -1;
        const int64_t i = lin(x, y, z);
        if (!(occupancy[i] < 0.5f || object_id[i] > 0u)) return -1;
        const double* e = extrema + 3 * i;
        if (std::isinf(e[0]) || std::isinf(e[1]) || std::isinf(e[2])) return -1;
        return (int64_t)labels[i];
    };
    auto connected = [&](int64_t a, int64_t b) {                             // are_connected_fn
        if (object_id[a] != object_id[b]) return false;
        const double* e1 = extrema + 3 * a;
        const double* e2 = extrema + 3 * b;
        const double dx = e1[0] - e2[0], dy = e1[1] - e2[1], dz = e1[2] - e2[2];
        double s = 0;
        s += dx * dx;
        s += dy * dy;
        s += dz * dz;
        return std::sqrt(s) < connected_threshold;
    };
    for (int64_t i = 0; i < n; ++i) labels[i] = 0u;
    std::vector<uint8_t> queued((size_t)n, 0);
    uint32_t k = 0;
    for (int64_t x = 0; x < nx; ++x)
        for (int64_t y = 0; y < ny; ++y)
            for (int64_t z = 0; z < nz; ++z) {
                if (component(x, y, z) != 0) continue;
                ++k;
                std::deque<int64_t> work;
                work.push_back(lin(x, y, z));
                queued[(size_t)lin(x, y, z)] = 1;
                while (!work.empty()) {
                    const int64_t c = work.front();
                    work.pop_front();
                    labels[c] = k;
                    const int64_t cx = c / (ny * nz), cy = (c / nz) % ny, cz = c % nz;
                    const int64_t nb[6][3] = {{cx - 1, cy, cz}, {cx + 1, cy, cz}, {cx, cy - 1, cz},
                                              {cx, cy + 1, cz}, {cx, cy, cz - 1}, {cx, cy, cz + 1}};
                    for (const auto& v : nb) {
                        if (component(v[0], v[1], v[2]) != 0) continue;
                        const int64_t j = lin(v[0], v[1], v[2]);
                        if (!connected(c, j) || queued[(size_t)j]) continue;
                        queued[(size_t)j] = 1;
                        work.push_back(j);
                    }
                }
            }
    return k;
}

}  // extern "C"
