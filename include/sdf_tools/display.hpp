// display -- the shared body of the ExportForDisplay family of SignedDistanceField, CollisionMapGrid and TaggedObjectCollisionMapGrid
// (reference src/sdf_tools/sdf.cpp:504-640, collision_map.cpp:317-562, tagged_object_collision_map.cpp:661-1364): plain mirrors of
// the ROS message types the methods return, the in-tree palette, and the helpers that turn the GPU's selection (include/sdfgpu.h
// "Display export": drawn indices and keys, in scan order or grouped by key) into points and colours.
//
// The mirrors keep the field names and constants of visualization_msgs/Marker, MarkerArray, std_msgs/ColorRGBA and the
// geometry_msgs types they hold, for builds without ROS.
//
// GenerateUniqueColor: the reference takes per-id colours from arc_helpers::GenerateUniqueColor, which is not vendored in the
// reference checkout, so the colours here are the in-tree palette's and parity with the reference's palette is UNVERIFIED (like the
// wire formats).  One property is the reference's own (tagged_object_collision_map.cpp:705-706): id 0 has alpha 0 and is
// therefore never drawn.  InterpolateHotToCold (convex segments from 22 up) is not vendored either; the same palette stands in.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "arc_utilities/voxel_grid.hpp"
#include "sdf_tools/gpu_context.hpp"

namespace std_msgs {
struct ColorRGBA { float r = 0.0f, g = 0.0f, b = 0.0f, a = 0.0f; };
struct Header { uint32_t seq = 0; double stamp = 0.0; std::string frame_id; };
}  // namespace std_msgs

namespace geometry_msgs {
struct Point { double x = 0.0, y = 0.0, z = 0.0; };
struct Quaternion { double x = 0.0, y = 0.0, z = 0.0, w = 0.0; };
struct Vector3 { double x = 0.0, y = 0.0, z = 0.0; };
struct Pose { Point position; Quaternion orientation; };
}  // namespace geometry_msgs

namespace visualization_msgs {
struct Marker {
    enum : int32_t { ARROW = 0, CUBE = 1, SPHERE = 2, CYLINDER = 3, LINE_STRIP = 4, LINE_LIST = 5, CUBE_LIST = 6, SPHERE_LIST = 7, POINTS = 8,
                     TEXT_VIEW_FACING = 9, MESH_RESOURCE = 10, TRIANGLE_LIST = 11 };
    enum : int32_t { ADD = 0, MODIFY = 0, DELETE = 2, DELETEALL = 3 };
    std_msgs::Header header;
    std::string ns;
    int32_t id = 0;
    int32_t type = 0;
    int32_t action = 0;
    geometry_msgs::Pose pose;
    geometry_msgs::Vector3 scale;
    std_msgs::ColorRGBA color;
    double lifetime = 0.0;
    bool frame_locked = false;
    std::vector<geometry_msgs::Point> points;
    std::vector<std_msgs::ColorRGBA> colors;
    std::string text;
    std::string mesh_resource;
    bool mesh_use_embedded_materials = false;
};
struct MarkerArray { std::vector<Marker> markers; };
}  // namespace visualization_msgs

namespace sdf_tools {

// In-tree palette (UNVERIFIED against arc_helpers, see the head of this file): id 0 is transparent black; every other id gets a hue
// by the golden ratio, full saturation and value, and the caller's alpha.
inline std_msgs::ColorRGBA GenerateUniqueColor(const uint32_t id, const float alpha = 1.0f) {
    std_msgs::ColorRGBA c;
    if (id == 0u) return c;
    const double h = std::fmod((double)id * 0.6180339887498949, 1.0) * 6.0;
    const int sector = (int)h;
    const float f = (float)(h - (double)sector), q = 1.0f - f;
    switch (sector % 6) {
        case 0: c.r = 1.0f; c.g = f; break;
        case 1: c.r = q; c.g = 1.0f; break;
        case 2: c.g = 1.0f; c.b = f; break;
        case 3: c.g = q; c.b = 1.0f; break;
        case 4: c.r = f; c.b = 1.0f; break;
        default: c.r = 1.0f; c.b = q; break;
    }
    c.a = alpha;
    return c;
}

namespace display {

inline std_msgs::ColorRGBA MakeColor(const float r, const float g, const float b, const float a) {
    std_msgs::ColorRGBA c;
    c.r = r; c.g = g; c.b = b; c.a = a;
    return c;
}

// header, id, type, action, lifetime, frame_locked, pose and scale as every method of the family fills them; ns is the caller's
inline visualization_msgs::Marker MakeMarker(const std::string& frame, const std::string& ns, const Eigen::Isometry3d& origin,
                                             const double resolution) {
    visualization_msgs::Marker m;
    m.header.frame_id = frame;
    m.ns = ns;
    m.id = 1;
    m.type = visualization_msgs::Marker::CUBE_LIST;
    m.action = visualization_msgs::Marker::ADD;
    m.lifetime = 0.0;
    m.frame_locked = false;
    const Eigen::Vector3d t = origin.translation();
    const Eigen::Quaterniond q(origin.rotation());
    m.pose.position.x = t.x(); m.pose.position.y = t.y(); m.pose.position.z = t.z();
    m.pose.orientation.x = q.x(); m.pose.orientation.y = q.y(); m.pose.orientation.z = q.z(); m.pose.orientation.w = q.w();
    m.scale.x = resolution; m.scale.y = resolution; m.scale.z = resolution;
    return m;
}

// the cell records of a grid, as the C ABI takes them
struct Cells {
    const void* data = nullptr;
    size_t stride = 0, occupancy_offset = 0;
    int64_t nx = 0, ny = 0, nz = 0;
    Eigen::Vector3d cell_sizes;
    int64_t count() const { return nx * ny * nz; }
};

struct Selection {
    std::vector<uint32_t> indices, keys;               // the drawn voxels, in scan order or grouped
    std::vector<uint32_t> group_keys, group_offsets;   // grouped form: group g is [group_offsets[g], group_offsets[g + 1])
};

// One selection on the GPU: a count-only call sizes the buffers, the second call fills them.  call(handle, list, n_list, grouped, idx,
// keys, capacity, total, group_keys, group_offsets, group_capacity, groups) is the entry point with its own leading arguments bound;
// max_groups bounds the number of groups when it is known (0: one per drawn voxel at most).
template <typename Call>
inline Selection SelectThrough(const Cells& c, const std::vector<uint32_t>* draw_keys, const bool grouped, const size_t max_groups, Call call) {
    Selection s;
    s.group_offsets.assign(1, 0u);
    if (c.count() <= 0) return s;
    std::vector<uint32_t> sorted;
    if (draw_keys) {
        sorted = *draw_keys;
        std::sort(sorted.begin(), sorted.end());
        sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
        if (sorted.empty()) sorted.reserve(1);              // (an empty list is still a list: a non-null pointer)
    }
    const uint32_t* list = draw_keys ? sorted.data() : nullptr;
    const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
    const std::lock_guard<std::mutex> lock(ctx->mutex);
    int64_t total = 0, groups = 0;
    sdf_generation::ThrowOnStatus(ctx->handle, call(ctx->handle, list, (int64_t)sorted.size(), 0, nullptr, nullptr, 0, &total, nullptr, nullptr, 0, nullptr));
    if (total == 0) return s;
    s.indices.resize((size_t)total);
    s.keys.resize((size_t)total);
    if (grouped) {                                          // (at most one group per drawn voxel)
        const size_t gcap = max_groups ? max_groups : (size_t)total;
        s.group_keys.resize(gcap);
        s.group_offsets.resize(gcap + 1);
    }
    sdf_generation::ThrowOnStatus(ctx->handle, call(ctx->handle, list, (int64_t)sorted.size(), grouped ? 1 : 0, s.indices.data(), s.keys.data(), total, &total,
                                                    grouped ? s.group_keys.data() : nullptr, grouped ? s.group_offsets.data() : nullptr,
                                                    (int64_t)s.group_keys.size(), grouped ? &groups : nullptr));
    if (grouped) {
        s.group_keys.resize((size_t)groups);
        s.group_offsets.resize((size_t)groups + 1);
    }
    return s;
}

inline Selection SelectCells(const Cells& c, const int rule, const size_t key_offset, const int class_mask, const bool surface_only,
                             const std::vector<uint32_t>* draw_keys, const bool draw_zero, const bool grouped) {
    return SelectThrough(c, draw_keys, grouped, rule == SDFGPU_DISPLAY_OCCUPANCY ? 3 : 0,          // (three keys for the occupancy rule)
                         [&](sdfgpu_handle h, const uint32_t* list, int64_t n_list, int g, uint32_t* idx, uint32_t* keys, int64_t cap, int64_t* total,
                             uint32_t* gk, uint32_t* go, int64_t gcap, int64_t* groups) {
                             return sdfgpu_display_select_cells(h, c.data, c.stride, c.occupancy_offset, key_offset, c.nx, c.ny, c.nz, rule, class_mask,
                                                                surface_only ? 1 : 0, list, n_list, draw_zero ? 1 : 0, g, idx, keys, cap, total, gk, go,
                                                                gcap, groups);
                         });
}

// The object contours (include/sdfgpu.h "Display export: contours"): cells filled for their own key (unknown cells count as filled,
// key 0 is never drawn) with a cell that is not within squared offset `reach`.
inline Selection SelectContour(const Cells& c, const size_t key_offset, const int reach, const std::vector<uint32_t>* draw_keys, const bool grouped) {
    return SelectThrough(c, draw_keys, grouped, 0,
                         [&](sdfgpu_handle h, const uint32_t* list, int64_t n_list, int g, uint32_t* idx, uint32_t* keys, int64_t cap, int64_t* total,
                             uint32_t* gk, uint32_t* go, int64_t gcap, int64_t* groups) {
                             return sdfgpu_display_select_contour(h, c.data, c.stride, c.occupancy_offset, key_offset, c.nx, c.ny, c.nz, reach, 1, list,
                                                                  n_list, 0, g, idx, keys, cap, total, gk, go, gcap, groups);
                         });
}

// body(begin, end) over [0, n) on a few host threads (one below 2^16 elements): every element is written once, by one thread
template <typename Body>
inline void ParallelFor(const size_t n, Body body) {
    const size_t threads = n < ((size_t)1 << 16) ? 1 : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
    if (threads == 1) { body((size_t)0, n); return; }
    std::vector<std::thread> team;
    const size_t per = (n + threads - 1) / threads;
    for (size_t t = 0; t < threads; ++t) {
        const size_t lo = std::min(n, t * per), hi = std::min(n, lo + per);
        if (lo < hi) team.emplace_back([=]() { body(lo, hi); });
    }
    for (std::thread& th : team) th.join();
}

inline geometry_msgs::Point PointOf(const Cells& c, const uint32_t index) {     // VoxelGrid::GridIndexToLocationGridFrame
    const int64_t v = (int64_t)index, t = v / c.nz;
    geometry_msgs::Point p;
    p.x = c.cell_sizes.x() * ((double)(t / c.ny) + 0.5);
    p.y = c.cell_sizes.y() * ((double)(t % c.ny) + 0.5);
    p.z = c.cell_sizes.z() * ((double)(v % c.nz) + 0.5);
    return p;
}

// elements [first, last) of a selection appended to the marker: points from the indices, colours from color_of(key, index) when
// with_colors.  The storage is sized once from the count.
template <typename ColorOf>
inline void Append(visualization_msgs::Marker& m, const Cells& c, const Selection& s, const size_t first, const size_t last,
                   const bool with_colors, ColorOf color_of) {
    const size_t base = m.points.size(), n = last - first;
    m.points.resize(base + n);
    if (with_colors) m.colors.resize(base + n);
    ParallelFor(n, [&](const size_t lo, const size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            m.points[base + i] = PointOf(c, s.indices[first + i]);
            if (with_colors) m.colors[base + i] = color_of(s.keys[first + i], s.indices[first + i]);
        }
    });
}

// ---- the occupancy exports of both grid classes (collision_map.cpp:317-496, tagged_object_collision_map.cpp:1188-1233) -----------
inline int ClassMask(const std_msgs::ColorRGBA& collision, const std_msgs::ColorRGBA& free_color, const std_msgs::ColorRGBA& unknown) {
    return (collision.a > 0.0f ? SDFGPU_DISPLAY_FILLED : 0) | (free_color.a > 0.0f ? SDFGPU_DISPLAY_EMPTY : 0) |
           (unknown.a > 0.0f ? SDFGPU_DISPLAY_UNKNOWN : 0);
}

inline visualization_msgs::Marker ExportOccupancy(visualization_msgs::Marker m, const Cells& c, const std_msgs::ColorRGBA& collision,
                                                  const std_msgs::ColorRGBA& free_color, const std_msgs::ColorRGBA& unknown,
                                                  const bool surface_only) {
    const int mask = ClassMask(collision, free_color, unknown);
    if (mask == 0) return m;
    const Selection s = SelectCells(c, SDFGPU_DISPLAY_OCCUPANCY, 0, mask, surface_only, nullptr, true, false);
    const std_msgs::ColorRGBA table[3] = {collision, free_color, unknown};
    Append(m, c, s, 0, s.indices.size(), true, [&](const uint32_t key, uint32_t) { return table[key]; });
    return m;
}

// the three markers of the *Separate* forms from ONE grouped selection; a class whose colour is invisible keeps an empty marker
inline visualization_msgs::MarkerArray ExportOccupancySeparate(const visualization_msgs::Marker& proto, const Cells& c,
                                                               const std_msgs::ColorRGBA& collision, const std_msgs::ColorRGBA& free_color,
                                                               const std_msgs::ColorRGBA& unknown, const bool surface_only,
                                                               const char* const ns[3]) {
    visualization_msgs::MarkerArray out;
    for (int k = 0; k < 3; ++k) { out.markers.push_back(proto); out.markers.back().ns = ns[k]; }
    const int mask = ClassMask(collision, free_color, unknown);
    if (mask == 0) return out;
    const Selection s = SelectCells(c, SDFGPU_DISPLAY_OCCUPANCY, 0, mask, surface_only, nullptr, true, true);
    const std_msgs::ColorRGBA table[3] = {collision, free_color, unknown};
    for (size_t g = 0; g < s.group_keys.size(); ++g)
        Append(out.markers[s.group_keys[g]], c, s, s.group_offsets[g], s.group_offsets[g + 1], true,
               [&](const uint32_t key, uint32_t) { return table[key]; });
    return out;
}

// ExportConnectedComponentsForDisplay: every cell is drawn, so there is nothing to select; points and colours are filled from the
// records.  Unknown cells (occupancy == 0.5) are grey unless asked otherwise.
template <typename Cell>
inline visualization_msgs::Marker ExportComponents(visualization_msgs::Marker m, const Cells& c, const std::vector<Cell>& cells,
                                                   const bool color_unknown_components) {
    const size_t n = cells.size();
    m.points.resize(n);
    m.colors.resize(n);
    ParallelFor(n, [&](const size_t lo, const size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            m.points[i] = PointOf(c, (uint32_t)i);
            m.colors[i] = (cells[i].occupancy != 0.5f || color_unknown_components) ? GenerateUniqueColor(cells[i].component)
                                                                                   : MakeColor(0.5f, 0.5f, 0.5f, 1.0f);
        }
    });
    return m;
}

}  // namespace display
}  // namespace sdf_tools
