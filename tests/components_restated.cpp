// components_restated.cpp -- test infrastructure, never on the product path: a plain restatement of the reference's connected
// components (src/sdf_tools/collision_map.cpp:564-618 over include/sdf_tools/topology_computation.hpp:25-150) that the GPU
// labels are compared with bit for bit.
//
// The reference scans x (outer), y, z (inner); every voxel not yet labelled starts the next component, which a breadth-first
// search over the 6 face neighbours of the same class fills.  Here the queue is a flat array and "queued" is the label itself
// (a voxel is labelled when it is queued), instead of a std::list and a hash map -- same visiting set, same numbering.
//   class(v) = filled[v] != 0 (callers pass occupancy > 0.5 already evaluated)
#include <cstddef>
#include <cstdint>
#include <vector>

extern "C" uint32_t cc_restated(const uint8_t* filled, int64_t nx, int64_t ny, int64_t nz, uint32_t* labels) {
    const int64_t n = nx * ny * nz, sy = nz, sx = ny * nz;
    for (int64_t v = 0; v < n; ++v) labels[v] = 0;
    std::vector<int64_t> queue;
    uint32_t k = 0;
    for (int64_t s = 0; s < n; ++s) {
        if (labels[s]) continue;
        ++k;
        const bool c = filled[s] != 0;
        queue.clear();
        queue.push_back(s);
        labels[s] = k;
        for (std::size_t head = 0; head < queue.size(); ++head) {
            const int64_t v = queue[head];
            const int64_t x = v / sx, y = (v / sy) % ny, z = v % nz;
            const int64_t nb[6] = {x > 0 ? v - sx : -1, x + 1 < nx ? v + sx : -1, y > 0 ? v - sy : -1,
                                   y + 1 < ny ? v + sy : -1, z > 0 ? v - 1 : -1, z + 1 < nz ? v + 1 : -1};
            for (int i = 0; i < 6; ++i) {
                const int64_t u = nb[i];
                if (u < 0 || labels[u] || (filled[u] != 0) != c) continue;
                labels[u] = k;
                queue.push_back(u);
            }
        }
    }
    return k;
}
