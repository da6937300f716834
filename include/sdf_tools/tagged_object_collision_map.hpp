// TaggedObjectCollisionMapGrid -- the SDF-producing subset of sdf_tools::TaggedObjectCollisionMapGrid
// (reference include/sdf_tools/tagged_object_collision_map.hpp): the 16-byte cell (:22-44), the cell-count
// constructor, SetValue, and the four callers of the SDF hot path
//   ExtractFreeAndNamedObjectsSignedDistanceField (:730-811), ExtractSignedDistanceField(objects_to_use)
//   (:813-856), MakeObjectSDFs (:875-891), MakeAllObjectSDFs (:893-915).
// plus (round 4) its wire type: SerializeSelf / DeserializeSelf in the reference's field order
// (src/sdf_tools/tagged_object_collision_map.cpp:23-75, :77-240), TCMZ / TCMR files (:242-307) and the
// TaggedObjectCollisionMap message pair (:309-339, msg/TaggedObjectCollisionMap.msg) -- byte format of the un-vendored
// arc_utilities serialisers: "wire-format parity unpinned", like the other two containers.
// The connected components (UpdateConnectedComponents, tagged_object_collision_map.cpp:340-380, same connectivity rule as
// CollisionMapGrid's) are computed on the GPU by sdfgpu_components_cells, and their topology (ComputeComponentTopology,
// :424-490) by sdfgpu_component_topology_cells, and the convex segments (UpdateConvexSegments, :552-654) by
// sdfgpu_convex_segments_cells, and the surface voxels of each component (ExtractComponentSurfaces, :492-550) by
// sdfgpu_component_surfaces_cells.  The display export (ExportForDisplay and its kin, :661-1364) selects on the GPU
// (include/sdfgpu.h "Display export", include/sdf_tools/display.hpp), the four ExportContourOnlyForDisplay overloads (:917-1180) included:
// a 26-neighbour stencil over the records stands in for their per-object SDFs (include/sdfgpu.h "Display export: contours").
// Every SDF is built on the GPU through sdfgpu_build_tagged_cells (device-side predicate).
#pragma once
#include <cstddef>
#include <cstdint>
#include <fstream>
#include <functional>
#include <iterator>
#include <limits>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "arc_utilities/serialization.hpp"
#include "arc_utilities/voxel_grid.hpp"
#include "arc_utilities/zlib_helpers.hpp"
#include "sdf_tools/component_surfaces.hpp"
#include "sdf_tools/component_topology.hpp"
#include "sdf_tools/display.hpp"
#include "sdf_tools/resample.hpp"
#include "sdf_tools/sdf.hpp"
#include "sdf_tools/sdf_generation.hpp"

namespace sdf_tools {

// Plain mirror of msg/TaggedObjectCollisionMap.msg for builds without ROS (field names kept).
struct TaggedObjectCollisionMap {
    struct Header { uint32_t seq = 0; double stamp = 0.0; std::string frame_id; } header;
    std::vector<uint8_t> serialized_map;
    bool is_compressed = false;
};

struct TAGGED_OBJECT_COLLISION_CELL {
    float occupancy;
    uint32_t component;
    uint32_t object_id;
    uint32_t convex_segment;
    TAGGED_OBJECT_COLLISION_CELL() : occupancy(0.0), component(0u), object_id(0u), convex_segment(0u) {}
    TAGGED_OBJECT_COLLISION_CELL(const float in_occupancy, const uint32_t in_object_id)
        : occupancy(in_occupancy), component(0u), object_id(in_object_id), convex_segment(0u) {}
    TAGGED_OBJECT_COLLISION_CELL(const float in_occupancy, const uint32_t in_object_id, const uint32_t in_component,
                                 const uint32_t in_convex_segment)
        : occupancy(in_occupancy), component(in_component), object_id(in_object_id), convex_segment(in_convex_segment) {}
};
static_assert(sizeof(TAGGED_OBJECT_COLLISION_CELL) == 16, "TAGGED_OBJECT_COLLISION_CELL must stay a 16-byte record");

class TaggedObjectCollisionMapGrid : public VoxelGrid::VoxelGrid<TAGGED_OBJECT_COLLISION_CELL> {
protected:
    uint32_t number_of_components_;
    uint32_t number_of_convex_segments_;
    std::string frame_;
    bool components_valid_;
    bool convex_segments_valid_;

    std::pair<SignedDistanceField, std::pair<double, double>> BuildWithFilter(
        const float oob_value, const int object_mode, const std::vector<uint32_t>& ids, const bool unknown_is_filled,
        const bool add_virtual_border, const bool cells_on_device = false) const {
        const Eigen::Vector3d cell_sizes = GetCellSizes();
        if ((cell_sizes.x() != cell_sizes.y()) || (cell_sizes.x() != cell_sizes.z()))
            throw std::invalid_argument("Grid must have uniform resolution");
        SignedDistanceField new_sdf(SignedDistanceField::ForBuild{}, GetOriginTransform(), frame_, cell_sizes.x(), GetNumXCells(),
                                    GetNumYCells(), GetNumZCells(), oob_value);
        double max_distance = 0.0, min_distance = 0.0;
        const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
        const std::lock_guard<std::mutex> lock(ctx->mutex);
        sdfgpu_handle h = ctx->handle;
        sdf_generation::ThrowOnStatus(
            h, sdfgpu_build_tagged_cells(h, cells_on_device ? nullptr : data_.data(), sizeof(TAGGED_OBJECT_COLLISION_CELL),
                                         offsetof(TAGGED_OBJECT_COLLISION_CELL, occupancy),
                                         offsetof(TAGGED_OBJECT_COLLISION_CELL, object_id), object_mode,
                                         ids.empty() ? nullptr : ids.data(), (int64_t)ids.size(), unknown_is_filled ? 1 : 0,
                                         GetNumXCells(), GetNumYCells(), GetNumZCells(), cell_sizes.x(),
                                         add_virtual_border ? 1 : 0, new_sdf.MutableDataForBuild(), &max_distance,
                                         &min_distance));
        return std::make_pair(std::move(new_sdf), std::make_pair(max_distance, min_distance));      // (moved: a copy of the field costs as much as its download)
    }

public:
    enum COMPONENT_TYPES : uint8_t { FILLED_COMPONENTS = 0x01, EMPTY_COMPONENTS = 0x02, UNKNOWN_COMPONENTS = 0x04 };

    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    using Base = ::VoxelGrid::VoxelGrid<TAGGED_OBJECT_COLLISION_CELL>;

    TaggedObjectCollisionMapGrid(const Eigen::Isometry3d& origin_transform, const std::string& frame, const double resolution,
                                 const int64_t x_cells, const int64_t y_cells, const int64_t z_cells,
                                 const TAGGED_OBJECT_COLLISION_CELL& oob_default_value)
        : Base(origin_transform, resolution, x_cells, y_cells, z_cells, oob_default_value), number_of_components_(0u),
          number_of_convex_segments_(0u), frame_(frame), components_valid_(false), convex_segments_valid_(false) {}
    TaggedObjectCollisionMapGrid(const std::string& frame, const double resolution, const int64_t x_cells, const int64_t y_cells,
                                 const int64_t z_cells, const TAGGED_OBJECT_COLLISION_CELL& oob_default_value)
        : Base(resolution, x_cells, y_cells, z_cells, oob_default_value), number_of_components_(0u),
          number_of_convex_segments_(0u), frame_(frame), components_valid_(false), convex_segments_valid_(false) {}
    // metric sizes (the reference's second constructor; Resample builds its result with it).  Only floating-point sizes select it, so
    // that integer literals keep meaning cell counts, as they did before this constructor existed.
    template <typename Size, typename = typename std::enable_if<std::is_floating_point<Size>::value>::type>
    TaggedObjectCollisionMapGrid(const Eigen::Isometry3d& origin_transform, const std::string& frame, const double resolution,
                                 const Size x_size, const Size y_size, const Size z_size,
                                 const TAGGED_OBJECT_COLLISION_CELL& oob_default_value)
        : Base(origin_transform, resolution, (double)x_size, (double)y_size, (double)z_size, oob_default_value), number_of_components_(0u),
          number_of_convex_segments_(0u), frame_(frame), components_valid_(false), convex_segments_valid_(false) {}
    TaggedObjectCollisionMapGrid()
        : Base(), number_of_components_(0u), number_of_convex_segments_(0u), frame_(""), components_valid_(false),
          convex_segments_valid_(false) {}

    Base* Clone() const override { return new TaggedObjectCollisionMapGrid(*this); }
    double GetResolution() const { return GetCellSizes().x(); }
    std::string GetFrame() const { return frame_; }
    void SetFrame(const std::string& f) { frame_ = f; }

    // ---- display export (reference tagged_object_collision_map.cpp:661-1364; include/sdf_tools/display.hpp) ---------------------------
    // Which cells are drawn and in which order comes from the GPU (include/sdfgpu.h "Display export", rule KEY_FIELD on object_id or
    // convex_segment, OCCUPANCY for the occupancy form); a cell whose colour has alpha <= 0 is not drawn, and the palette gives id 0
    // alpha 0.
    static std_msgs::ColorRGBA GenerateComponentColor(const uint32_t component, const float alpha = 1.0f) { return GenerateUniqueColor(component, alpha); }
    display::Cells DisplayCells() const {
        display::Cells c;
        c.data = data_.data(); c.stride = sizeof(TAGGED_OBJECT_COLLISION_CELL); c.occupancy_offset = offsetof(TAGGED_OBJECT_COLLISION_CELL, occupancy);
        c.nx = GetNumXCells(); c.ny = GetNumYCells(); c.nz = GetNumZCells(); c.cell_sizes = GetCellSizes();
        return c;
    }
    // (does not fill the namespace)
    visualization_msgs::Marker DefaultMarker() const { return display::MakeMarker(frame_, "", GetOriginTransform(), GetResolution()); }

private:
    static constexpr const char* kDisplayNs = "tagged_object_collision_map_display";
    visualization_msgs::Marker NamedMarker(const std::string& ns) const { visualization_msgs::Marker m = DefaultMarker(); m.ns = ns; return m; }
    display::Selection SelectObjects(const std::vector<uint32_t>* draw, const bool draw_zero, const bool grouped) const {
        return display::SelectCells(DisplayCells(), SDFGPU_DISPLAY_KEY_FIELD, offsetof(TAGGED_OBJECT_COLLISION_CELL, object_id), 7, false, draw,
                                    draw_zero, grouped);
    }
    // One marker per object from a grouped selection: `first` are the ids that get a marker up front, in that order (a repeated id
    // keeps its last place, as the reference's map does); the other drawn ids follow in the order of their first cell in the scan
    // when `others`.  Markers without points are pruned.
    template <typename ColorOf>
    visualization_msgs::MarkerArray UniqueNsMarkers(const display::Selection& s, const std::vector<uint32_t>& first, const bool others,
                                                    ColorOf color_of) const {
        std::map<uint32_t, size_t> group_of;
        for (size_t g = 0; g < s.group_keys.size(); ++g) group_of[s.group_keys[g]] = g;
        std::map<uint32_t, size_t> place;                                  // id -> its place among the up-front markers
        for (size_t i = 0; i < first.size(); ++i) place[first[i]] = i;
        std::vector<uint32_t> order;
        for (size_t i = 0; i < first.size(); ++i) if (place[first[i]] == i) order.push_back(first[i]);
        if (others) {
            std::vector<std::pair<uint32_t, uint32_t>> rest;               // (first index, id)
            for (size_t g = 0; g < s.group_keys.size(); ++g)
                if (!place.count(s.group_keys[g])) rest.emplace_back(s.indices[s.group_offsets[g]], s.group_keys[g]);
            std::sort(rest.begin(), rest.end());
            for (const auto& r : rest) order.push_back(r.second);
        }
        visualization_msgs::MarkerArray out;
        const display::Cells c = DisplayCells();
        for (const uint32_t id : order) {
            const auto found = group_of.find(id);
            if (found == group_of.end()) continue;                         // (no drawn cell: the marker would be pruned)
            const size_t g = found->second;
            out.markers.push_back(NamedMarker(std::string(kDisplayNs) + "_" + std::to_string(id)));
            display::Append(out.markers.back(), c, s, s.group_offsets[g], s.group_offsets[g + 1], true,
                            [&](const uint32_t key, uint32_t) { return color_of(key); });
        }
        return out;
    }
    // colour of an object under a caller's colour map: the map's entry, else the palette's
    static std_msgs::ColorRGBA MappedColor(const std::map<uint32_t, std_msgs::ColorRGBA>& color_map, const uint32_t id) {
        const auto found = color_map.find(id);
        return found != color_map.end() ? found->second : GenerateComponentColor(id);
    }
    // the selection of the colour-map forms: every object whose colour is visible (the GPU draws all ids, 0 only when the map makes
    // it visible; objects that the map hides are dropped here)
    display::Selection SelectMapped(const std::map<uint32_t, std_msgs::ColorRGBA>& color_map, const bool grouped) const {
        return DropHidden(SelectObjects(nullptr, MappedColor(color_map, 0u).a > 0.0f, grouped), color_map, grouped);
    }
    static display::Selection DropHidden(display::Selection s, const std::map<uint32_t, std_msgs::ColorRGBA>& color_map, const bool grouped) {
        std::vector<uint32_t> hidden;
        for (const auto& kv : color_map) if (!(kv.second.a > 0.0f) && kv.first != 0u) hidden.push_back(kv.first);
        if (hidden.empty() || s.indices.empty()) return s;
        display::Selection kept;
        kept.group_offsets.assign(1, 0u);
        auto is_hidden = [&](const uint32_t id) { return std::binary_search(hidden.begin(), hidden.end(), id); };
        if (!grouped) {
            for (size_t i = 0; i < s.indices.size(); ++i)
                if (!is_hidden(s.keys[i])) { kept.indices.push_back(s.indices[i]); kept.keys.push_back(s.keys[i]); }
            return kept;
        }
        for (size_t g = 0; g < s.group_keys.size(); ++g) {
            if (is_hidden(s.group_keys[g])) continue;
            kept.indices.insert(kept.indices.end(), s.indices.begin() + s.group_offsets[g], s.indices.begin() + s.group_offsets[g + 1]);
            kept.keys.insert(kept.keys.end(), s.keys.begin() + s.group_offsets[g], s.keys.begin() + s.group_offsets[g + 1]);
            kept.group_keys.push_back(s.group_keys[g]);
            kept.group_offsets.push_back((uint32_t)kept.indices.size());
        }
        return kept;
    }

public:
    visualization_msgs::Marker ExportForDisplay(const float alpha = 1.0f, const std::vector<uint32_t>& objects_to_draw = std::vector<uint32_t>()) const {
        visualization_msgs::Marker m = NamedMarker(kDisplayNs);
        if (!(alpha > 0.0f)) return m;                                     // (every colour would be invisible)
        const display::Selection s = SelectObjects(objects_to_draw.empty() ? nullptr : &objects_to_draw, false, false);
        display::Append(m, DisplayCells(), s, 0, s.indices.size(), true, [&](const uint32_t key, uint32_t) { return GenerateComponentColor(key, alpha); });
        return m;
    }
    visualization_msgs::MarkerArray ExportForDisplayUniqueNs(const float alpha = 1.0f,
                                                             const std::vector<uint32_t>& objects_to_draw = std::vector<uint32_t>()) const {
        if (!(alpha > 0.0f)) return visualization_msgs::MarkerArray();
        const display::Selection s = SelectObjects(objects_to_draw.empty() ? nullptr : &objects_to_draw, false, true);
        return UniqueNsMarkers(s, objects_to_draw, objects_to_draw.empty(), [&](const uint32_t key) { return GenerateComponentColor(key, alpha); });
    }
    visualization_msgs::Marker ExportForDisplay(const std::map<uint32_t, std_msgs::ColorRGBA>& color_map) const {
        visualization_msgs::Marker m = NamedMarker(kDisplayNs);
        const display::Selection s = SelectMapped(color_map, false);
        display::Append(m, DisplayCells(), s, 0, s.indices.size(), true, [&](const uint32_t key, uint32_t) { return MappedColor(color_map, key); });
        return m;
    }
    // markers of the map's objects first, in ascending id, then the others in the order of their first cell
    visualization_msgs::MarkerArray ExportForDisplayUniqueNs(const std::map<uint32_t, std_msgs::ColorRGBA>& color_map) const {
        std::vector<uint32_t> first;
        for (const auto& kv : color_map) first.push_back(kv.first);
        return UniqueNsMarkers(SelectMapped(color_map, true), first, true, [&](const uint32_t key) { return MappedColor(color_map, key); });
    }
    // ---- contours (reference :917-1180) --------------------------------------------------------------------------------------------
    // The reference builds MakeObjectSDFs(ids, unknown_is_filled = true, add_virtual_border = false) and draws a cell iff its own
    // object's distance lies in (-1.9 resolution, 0): the cells within squared distance `reach` of a cell that is not theirs
    // (sdfgpu_display_contour_reach; 3 at every ordinary resolution), which the GPU finds by a 26-neighbour stencil without any SDF.
    // Objects: the listed ones, or every id > 0 (MakeAllObjectSDFs drops id 0; a listed id 0 has the palette's alpha 0).  Throws what
    // MakeObjectSDFs throws on a non-uniform grid.
private:
    int ContourReach() const {
        const Eigen::Vector3d cell_sizes = GetCellSizes();
        if ((cell_sizes.x() != cell_sizes.y()) || (cell_sizes.x() != cell_sizes.z()))
            throw std::invalid_argument("Grid must have uniform resolution");
        int reach = 0;
        if (sdfgpu_display_contour_reach(GetResolution(), &reach) != SDFGPU_OK) throw std::invalid_argument("sdfgpu_display_contour_reach refused");
        return reach;
    }
    display::Selection SelectContour(const std::vector<uint32_t>* draw, const bool grouped) const {
        return display::SelectContour(DisplayCells(), offsetof(TAGGED_OBJECT_COLLISION_CELL, object_id), ContourReach(), draw, grouped);
    }
    // one marker per drawn object in ascending id (the order of the reference's std::map of SDFs); objects without a drawn cell have none
    template <typename ColorOf>
    visualization_msgs::MarkerArray ContourMarkers(const display::Selection& s, ColorOf color_of) const {
        visualization_msgs::MarkerArray out;
        const display::Cells c = DisplayCells();
        for (size_t g = 0; g < s.group_keys.size(); ++g) {
            if (s.group_offsets[g] == s.group_offsets[g + 1]) continue;
            out.markers.push_back(NamedMarker(std::string(kDisplayNs) + "_" + std::to_string(s.group_keys[g])));
            display::Append(out.markers.back(), c, s, s.group_offsets[g], s.group_offsets[g + 1], true,
                            [&](const uint32_t key, uint32_t) { return color_of(key); });
        }
        return out;
    }

public:
    visualization_msgs::Marker ExportContourOnlyForDisplay(const float alpha = 1.0f,
                                                           const std::vector<uint32_t>& objects_to_draw = std::vector<uint32_t>()) const {
        visualization_msgs::Marker m = NamedMarker(kDisplayNs);
        const int reach = ContourReach();                                  // (throws first, as the reference's SDF build does)
        if (!(alpha > 0.0f) || reach == 0) return m;                       // (every colour would be invisible)
        const display::Selection s = SelectContour(objects_to_draw.empty() ? nullptr : &objects_to_draw, false);
        display::Append(m, DisplayCells(), s, 0, s.indices.size(), true, [&](const uint32_t key, uint32_t) { return GenerateComponentColor(key, alpha); });
        return m;
    }
    visualization_msgs::MarkerArray ExportContourOnlyForDisplayUniqueNs(const float alpha = 1.0f,
                                                                        const std::vector<uint32_t>& objects_to_draw = std::vector<uint32_t>()) const {
        const int reach = ContourReach();
        if (!(alpha > 0.0f) || reach == 0) return visualization_msgs::MarkerArray();
        const display::Selection s = SelectContour(objects_to_draw.empty() ? nullptr : &objects_to_draw, true);
        return ContourMarkers(s, [&](const uint32_t key) { return GenerateComponentColor(key, alpha); });
    }
    // every id > 0 in the map's colour, or the palette's where the map has none; ids the map hides are dropped; id 0 is never drawn,
    // even when the map makes it visible (unlike ExportForDisplay(color_map))
    visualization_msgs::Marker ExportContourOnlyForDisplay(const std::map<uint32_t, std_msgs::ColorRGBA>& color_map) const {
        visualization_msgs::Marker m = NamedMarker(kDisplayNs);
        const display::Selection s = DropHidden(SelectContour(nullptr, false), color_map, false);
        display::Append(m, DisplayCells(), s, 0, s.indices.size(), true, [&](const uint32_t key, uint32_t) { return MappedColor(color_map, key); });
        return m;
    }
    visualization_msgs::MarkerArray ExportContourOnlyForDisplayUniqueNs(const std::map<uint32_t, std_msgs::ColorRGBA>& color_map) const {
        return ContourMarkers(DropHidden(SelectContour(nullptr, true), color_map, true), [&](const uint32_t key) { return MappedColor(color_map, key); });
    }

    visualization_msgs::Marker ExportForDisplayOccupancyOnly(const std_msgs::ColorRGBA& collision_color, const std_msgs::ColorRGBA& free_color,
                                                             const std_msgs::ColorRGBA& unknown_color) const {
        return display::ExportOccupancy(NamedMarker("tagged_object_collision_map_occupancy_display"), DisplayCells(), collision_color, free_color,
                                        unknown_color, false);
    }
    visualization_msgs::Marker ExportConnectedComponentsForDisplay(const bool color_unknown_components) const {
        return display::ExportComponents(NamedMarker("tagged_object_connected_components_display"), DisplayCells(), data_, color_unknown_components);
    }
    // The cells of one convex segment of one object: the GPU selects the segment, the object id is tested on the records here.
    // Below 22 segments the palette colours the segment; from 22 up the reference interpolates hot to cold, which is not vendored:
    // the palette stands in (UNVERIFIED, include/sdf_tools/display.hpp).
    visualization_msgs::Marker ExportConvexSegmentForDisplay(const uint32_t object_id, const uint32_t convex_segment) const {
        visualization_msgs::Marker m = NamedMarker("tagged_object_" + std::to_string(object_id) + "_convex_segment_" + std::to_string(convex_segment) + "_display");
        const std::vector<uint32_t> segment(1, convex_segment);
        display::Selection s = display::SelectCells(DisplayCells(), SDFGPU_DISPLAY_KEY_FIELD, offsetof(TAGGED_OBJECT_COLLISION_CELL, convex_segment), 7,
                                                    false, &segment, true, false);
        size_t kept = 0;
        for (size_t i = 0; i < s.indices.size(); ++i)
            if (data_[s.indices[i]].object_id == object_id) { s.indices[kept] = s.indices[i]; s.keys[kept] = s.keys[i]; ++kept; }
        s.indices.resize(kept);
        s.keys.resize(kept);
        display::Append(m, DisplayCells(), s, 0, kept, true, [&](const uint32_t key, uint32_t) { return GenerateComponentColor(key); });
        return m;
    }
    // host only: walks the caller's map (its order), keeping the entries marked 1
    visualization_msgs::Marker ExportSurfaceForDisplay(const std::unordered_map<GRID_INDEX, uint8_t>& surface,
                                                       const std_msgs::ColorRGBA& surface_color) const {
        visualization_msgs::Marker m = NamedMarker("tagged_object_collision_map_surface");
        for (const auto& entry : surface) {
            if (entry.second != 1) continue;
            const Eigen::Vector4d l = GridIndexToLocationGridFrame(entry.first);
            geometry_msgs::Point p;
            p.x = l(0); p.y = l(1); p.z = l(2);
            m.points.push_back(p);
            m.colors.push_back(surface_color);
        }
        return m;
    }

    bool SetValue(const int64_t x, const int64_t y, const int64_t z, const TAGGED_OBJECT_COLLISION_CELL& value) override {
        if (!IndexInBounds(x, y, z)) return false;
        components_valid_ = false;
        convex_segments_valid_ = false;
        AccessIndex(GetDataIndex(x, y, z)) = value;
        return true;
    }
    bool SetValue(const GRID_INDEX& i, const TAGGED_OBJECT_COLLISION_CELL& v) override { return SetValue(i.x, i.y, i.z, v); }

    // ---- Resample (reference tagged_object_collision_map.cpp:399-422): as CollisionMapGrid::Resample -- whole 16-byte records move
    // (occupancy, component, object id, convex segment); the result's components and convex segments are invalid; result cells
    // that hold no source centre keep the OOB value.
    TaggedObjectCollisionMapGrid Resample(const double new_resolution) const { return ResampleGridFromCells(*this, new_resolution); }

    // ---- connected components (reference tagged_object_collision_map.cpp:340-380): occupancy > 0.5 against the rest, whatever
    // the object id; 6-connectivity; numbered 1..K in x -> y -> z scan order, written into every cell's `component`.
    uint32_t UpdateConnectedComponents() {
        if (components_valid_) return number_of_components_;
        uint32_t count = 0;
        if (!data_.empty()) {
            const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
            const std::lock_guard<std::mutex> lock(ctx->mutex);
            sdf_generation::ThrowOnStatus(
                ctx->handle, sdfgpu_components_cells(ctx->handle, data_.data(), sizeof(TAGGED_OBJECT_COLLISION_CELL),
                                                     offsetof(TAGGED_OBJECT_COLLISION_CELL, occupancy),
                                                     offsetof(TAGGED_OBJECT_COLLISION_CELL, component), GetNumXCells(),
                                                     GetNumYCells(), GetNumZCells(), &count));
        }
        number_of_components_ = count;
        components_valid_ = true;
        return number_of_components_;
    }

    std::pair<uint32_t, bool> GetNumConnectedComponents() const { return std::make_pair(number_of_components_, components_valid_); }

    // ---- component topology (reference tagged_object_collision_map.cpp:424-490) ---------------------------------------------
    // {component: (holes, voids)} of the components whose voxels are in component_types_to_use: FILLED (occupancy > 0.5), EMPTY
    // (< 0.5), UNKNOWN (the rest, NaN included), computed on the GPU (include/sdfgpu.h "Component topology").  Free space is one
    // class for the components, so a free component holding both empty and unknown voxels under a mask that takes one of them
    // and not the other is refused (std::invalid_argument).  Labels as in CollisionMapGrid::ComputeComponentTopology.
    std::map<uint32_t, std::pair<int32_t, int32_t>> ComputeComponentTopology(const COMPONENT_TYPES component_types_to_use,
                                                                             const bool recompute_connected_components,
                                                                             const bool verbose) {
        if (recompute_connected_components) UpdateConnectedComponents();
        uint32_t max_label = number_of_components_;
        if (!components_valid_) {
            max_label = 0;
            for (const TAGGED_OBJECT_COLLISION_CELL& cell : data_) max_label = cell.component > max_label ? cell.component : max_label;
        }
        return ComputeComponentTopologyFromCells(data_.data(), sizeof(TAGGED_OBJECT_COLLISION_CELL),
                                                 offsetof(TAGGED_OBJECT_COLLISION_CELL, occupancy),
                                                 offsetof(TAGGED_OBJECT_COLLISION_CELL, component), GetNumXCells(), GetNumYCells(),
                                                 GetNumZCells(), (int)component_types_to_use, max_label, verbose);
    }

    // ---- component surfaces (reference tagged_object_collision_map.cpp:492-550, tagged_object_collision_map.hpp:703-723) ---------------------------------------------------------------
    // {component: {index: 1}} of the surface voxels -- a voxel with a face neighbour of another component, the outside of the
    // grid being component -1 -- whose occupancy class is in component_types_to_extract, found on the GPU from the STORED
    // labels (include/sdfgpu.h "Component surfaces": every class is tested at (x, y, z), and the z = nz - 1 face is a grid face
    // like the other five).  Components are not recomputed, as in the reference.
    std::map<uint32_t, std::unordered_map<GRID_INDEX, uint8_t>> ExtractComponentSurfaces(const COMPONENT_TYPES component_types_to_extract) const {
        return ComponentSurfacesToMap(ExtractComponentSurfaceIndices(component_types_to_extract), GetNumYCells(), GetNumZCells());
    }
    std::map<uint32_t, std::unordered_map<GRID_INDEX, uint8_t>> ExtractFilledComponentSurfaces() const { return ExtractComponentSurfaces(FILLED_COMPONENTS); }
    std::map<uint32_t, std::unordered_map<GRID_INDEX, uint8_t>> ExtractUnknownComponentSurfaces() const { return ExtractComponentSurfaces(UNKNOWN_COMPONENTS); }
    std::map<uint32_t, std::unordered_map<GRID_INDEX, uint8_t>> ExtractEmptyComponentSurfaces() const { return ExtractComponentSurfaces(EMPTY_COMPONENTS); }

    // The fast form: offsets per component and ascending uint32 linear indices, no hash maps (component_surfaces.hpp).
    ComponentSurfaceIndices ExtractComponentSurfaceIndices(const COMPONENT_TYPES component_types_to_extract) const {
        uint32_t max_label = number_of_components_;
        if (!components_valid_) {
            max_label = 0;
            for (const TAGGED_OBJECT_COLLISION_CELL& cell : data_) max_label = cell.component > max_label ? cell.component : max_label;
        }
        return ExtractComponentSurfaceIndicesFromCells(data_.data(), sizeof(TAGGED_OBJECT_COLLISION_CELL), offsetof(TAGGED_OBJECT_COLLISION_CELL, occupancy),
                                                       offsetof(TAGGED_OBJECT_COLLISION_CELL, component), GetNumXCells(), GetNumYCells(), GetNumZCells(),
                                                       (int)component_types_to_extract, max_label);
    }

    // ---- candidate corners (reference tagged_object_collision_map.hpp:558-669): (two or more in-grid face neighbours of another component, index in the grid)
    std::pair<bool, bool> CheckIfCandidateCorner3d(const Eigen::Vector3d& location) const {
        const GRID_INDEX index = LocationToGridIndex3d(location);
        return IndexInBounds(index) ? CheckIfCandidateCorner(index) : std::pair<bool, bool>(false, false);
    }
    std::pair<bool, bool> CheckIfCandidateCorner4d(const Eigen::Vector4d& location) const {
        const GRID_INDEX index = LocationToGridIndex4d(location);
        return IndexInBounds(index) ? CheckIfCandidateCorner(index) : std::pair<bool, bool>(false, false);
    }
    std::pair<bool, bool> CheckIfCandidateCorner(const double x, const double y, const double z) const {
        return CheckIfCandidateCorner4d(Eigen::Vector4d(x, y, z, 1.0));
    }
    std::pair<bool, bool> CheckIfCandidateCorner(const GRID_INDEX& index) const { return CheckIfCandidateCorner(index.x, index.y, index.z); }
    std::pair<bool, bool> CheckIfCandidateCorner(const int64_t x_index, const int64_t y_index, const int64_t z_index) const {
        return CheckIfCandidateCornerOnGrid(*this, x_index, y_index, z_index);
    }

    // ---- convex segments (reference tagged_object_collision_map.cpp:552-654) ---------------------------------------------------
    // The SDF (virtual border: every filled cell; otherwise free space outside, named objects inside) -> its local extrema map ->
    // segments: face neighbours that take part (occupancy < 0.5 or a named object, and an extremum inside the grid), carry the
    // same object id and whose extrema lie closer than connected_threshold are joined; numbered 1..K in x -> y -> z scan order,
    // 0 for every other cell, written into every cell's `convex_segment` (include/sdfgpu.h "Local extrema and convex segments").
    // One GPU call: the cells travel once, the SDF and the extrema never leave the device.  Unlike the reference, which writes
    // the labels through SetValue, the connected components stay valid: occupancy and object ids are not touched.
    uint32_t UpdateConvexSegments(const double connected_threshold, const bool add_virtual_border) {
        const Eigen::Vector3d cell_sizes = GetCellSizes();
        if ((cell_sizes.x() != cell_sizes.y()) || (cell_sizes.x() != cell_sizes.z()))
            throw std::invalid_argument("Grid must have uniform resolution");
        uint32_t count = 0;
        if (!data_.empty()) {
            const Eigen::Quaterniond q(GetOriginTransform().rotation());
            const Eigen::Quaterniond qi = q.inverse();
            const double q_and_qinv[8] = {q.w(), q.x(), q.y(), q.z(), qi.w(), qi.x(), qi.y(), qi.z()};
            const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
            const std::lock_guard<std::mutex> lock(ctx->mutex);
            sdf_generation::ThrowOnStatus(
                ctx->handle, sdfgpu_convex_segments_cells(ctx->handle, data_.data(), sizeof(TAGGED_OBJECT_COLLISION_CELL),
                                                          offsetof(TAGGED_OBJECT_COLLISION_CELL, occupancy),
                                                          offsetof(TAGGED_OBJECT_COLLISION_CELL, object_id),
                                                          offsetof(TAGGED_OBJECT_COLLISION_CELL, convex_segment), GetNumXCells(),
                                                          GetNumYCells(), GetNumZCells(), cell_sizes.x(), q_and_qinv, connected_threshold,
                                                          add_virtual_border ? 1 : 0, &count));
        }
        number_of_convex_segments_ = count;
        convex_segments_valid_ = true;
        return number_of_convex_segments_;
    }

    std::pair<uint32_t, bool> GetNumConvexSegments() const { return std::make_pair(number_of_convex_segments_, convex_segments_valid_); }
    bool AreConvexSegmentsValid() const { return convex_segments_valid_; }

    // ---- wire formats: tagged_object_collision_map.cpp:23-75 (fields), :242-307 (files), :309-339 (messages) ------------
    using CellSerializer = std::function<uint64_t(const TAGGED_OBJECT_COLLISION_CELL&, std::vector<uint8_t>&)>;
    using CellDeserializer = std::function<std::pair<TAGGED_OBJECT_COLLISION_CELL, uint64_t>(const std::vector<uint8_t>&, const uint64_t)>;

    uint64_t SerializeSelf(std::vector<uint8_t>& buffer,
                           const CellSerializer& value_serializer = arc_utilities::SerializeFixedSizePOD<TAGGED_OBJECT_COLLISION_CELL>) const override {
        (void)value_serializer;                                   // (ignored by the reference too: cells are fixed-size PODs, :29)
        const uint64_t start = buffer.size();
        BaseSerializeSelf(buffer, arc_utilities::SerializeFixedSizePOD<TAGGED_OBJECT_COLLISION_CELL>);   // initialized .. OOB value (:31-63)
        arc_utilities::SerializeFixedSizePOD<uint32_t>(number_of_components_, buffer);                   // (:65)
        arc_utilities::SerializeFixedSizePOD<uint32_t>(number_of_convex_segments_, buffer);              // (:66)
        arc_utilities::SerializeString(frame_, buffer);                                                  // (:67)
        arc_utilities::SerializeFixedSizePOD<uint8_t>((uint8_t)components_valid_, buffer);               // (:68)
        arc_utilities::SerializeFixedSizePOD<uint8_t>((uint8_t)convex_segments_valid_, buffer);          // (:70)
        return buffer.size() - start;
    }
    uint64_t DeserializeSelf(const std::vector<uint8_t>& buffer, const uint64_t current,
                             const CellDeserializer& value_deserializer = arc_utilities::DeserializeFixedSizePOD<TAGGED_OBJECT_COLLISION_CELL>) override {
        (void)value_deserializer;
        uint64_t pos = current;
        pos += BaseDeserializeSelf(buffer, pos, arc_utilities::DeserializeFixedSizePOD<TAGGED_OBJECT_COLLISION_CELL>);
        const auto nc = arc_utilities::DeserializeFixedSizePOD<uint32_t>(buffer, pos); pos += nc.second;
        const auto ns = arc_utilities::DeserializeFixedSizePOD<uint32_t>(buffer, pos); pos += ns.second;
        const auto fr = arc_utilities::DeserializeString(buffer, pos); pos += fr.second;
        const auto cv = arc_utilities::DeserializeFixedSizePOD<uint8_t>(buffer, pos); pos += cv.second;
        const auto sv = arc_utilities::DeserializeFixedSizePOD<uint8_t>(buffer, pos); pos += sv.second;
        number_of_components_ = nc.first;
        number_of_convex_segments_ = ns.first;
        frame_ = fr.first;
        components_valid_ = (bool)cv.first;
        convex_segments_valid_ = (bool)sv.first;
        return pos - current;
    }

    static void SaveToFile(const TaggedObjectCollisionMapGrid& map, const std::string& filepath, const bool compress) {
        std::vector<uint8_t> buffer;
        map.SerializeSelf(buffer);
        std::ofstream out(filepath, std::ios::out | std::ios::binary);
        const std::vector<uint8_t> body = compress ? ZlibHelpers::CompressBytes(buffer) : buffer;
        out.write(compress ? "TCMZ" : "TCMR", 4);                 // 4-byte magic (:251-263)
        out.write(reinterpret_cast<const char*>(body.data()), (std::streamsize)body.size());
    }
    static TaggedObjectCollisionMapGrid LoadFromFile(const std::string& filepath) {
        std::ifstream in(filepath, std::ios::in | std::ios::binary);
        if (!in.good()) throw std::invalid_argument("File does not exist");
        std::vector<uint8_t> all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (all.size() < 4) throw std::invalid_argument("File is too small");
        const std::string magic(all.begin(), all.begin() + 4);
        const std::vector<uint8_t> body(all.begin() + 4, all.end());
        TaggedObjectCollisionMapGrid map;
        if (magic == "TCMZ") map.DeserializeSelf(ZlibHelpers::DecompressBytes(body), 0);
        else if (magic == "TCMR") map.DeserializeSelf(body, 0);
        else throw std::invalid_argument("File has invalid header [" + magic + "]");
        return map;
    }
    static TaggedObjectCollisionMap GetMessageRepresentation(const TaggedObjectCollisionMapGrid& map) {
        TaggedObjectCollisionMap msg;                             // always zlib-compressed (:312-321); no ROS clock here: stamp stays 0
        msg.header.frame_id = map.GetFrame();
        std::vector<uint8_t> buffer;
        map.SerializeSelf(buffer);
        msg.serialized_map = ZlibHelpers::CompressBytes(buffer);
        msg.is_compressed = true;
        return msg;
    }
    static TaggedObjectCollisionMapGrid LoadFromMessageRepresentation(const TaggedObjectCollisionMap& message) {
        TaggedObjectCollisionMapGrid map;
        if (message.is_compressed) map.DeserializeSelf(ZlibHelpers::DecompressBytes(message.serialized_map), 0);
        else map.DeserializeSelf(message.serialized_map, 0);
        return map;
    }

    // Filled = occupied cell whose object id is in objects_to_use (any object if the list is empty), :813-856.
    std::pair<SignedDistanceField, std::pair<double, double>> ExtractSignedDistanceField(
        const float oob_value, const std::vector<uint32_t>& objects_to_use, const bool unknown_is_filled,
        const bool add_virtual_border) const {
        return BuildWithFilter(oob_value, 2, objects_to_use, unknown_is_filled, add_virtual_border);
    }

    // Free-space SDF outside, named-object SDF inside, 0 in filled cells that belong to no named object, :730-811.
    std::pair<SignedDistanceField, std::pair<double, double>> ExtractFreeAndNamedObjectsSignedDistanceField(
        const float oob_value, const bool unknown_is_filled) const {
        const auto free_sdf_result = BuildWithFilter(oob_value, 0, {}, unknown_is_filled, false);
        // (same records as the call above: they are still on the device)
        const auto named_objects_sdf_result = BuildWithFilter(oob_value, 1, {}, unknown_is_filled, false, true);
        SignedDistanceField combined_sdf = free_sdf_result.first;
        const std::vector<float>& fr = free_sdf_result.first.GetImmutableRawData();
        const std::vector<float>& nm = named_objects_sdf_result.first.GetImmutableRawData();
        float* out = combined_sdf.MutableDataForBuild();
        for (size_t i = 0; i < fr.size(); i++) {
            if (fr[i] >= 0.0) out[i] = fr[i];
            else if (nm[i] <= -0.0) out[i] = nm[i];
            else out[i] = 0.0f;
        }
        return std::make_pair(combined_sdf, std::make_pair(free_sdf_result.second.first, named_objects_sdf_result.second.second));
    }

    // One SDF per object id, built with oob = +inf like the reference (:875-891).  ONE call for all ids: the cell records travel
    // once and the batch kernels classify them per id (sdfgpu_build_tagged_objects), no host round trip between objects.
    std::map<uint32_t, SignedDistanceField> MakeObjectSDFs(const std::vector<uint32_t>& object_ids, const bool unknown_is_filled,
                                                           const bool add_virtual_border) const {
        std::map<uint32_t, SignedDistanceField> per_object_sdfs;
        if (object_ids.empty()) return per_object_sdfs;
        const Eigen::Vector3d cell_sizes = GetCellSizes();
        if ((cell_sizes.x() != cell_sizes.y()) || (cell_sizes.x() != cell_sizes.z()))
            throw std::invalid_argument("Grid must have uniform resolution");
        const size_t n = data_.size();
        std::vector<float> fields(object_ids.size() * n);
        {
            const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
            const std::lock_guard<std::mutex> lock(ctx->mutex);
            sdfgpu_handle h = ctx->handle;
            sdf_generation::ThrowOnStatus(
                h, sdfgpu_build_tagged_objects(h, data_.data(), sizeof(TAGGED_OBJECT_COLLISION_CELL),
                                               offsetof(TAGGED_OBJECT_COLLISION_CELL, occupancy),
                                               offsetof(TAGGED_OBJECT_COLLISION_CELL, object_id), object_ids.data(),
                                               (int64_t)object_ids.size(), unknown_is_filled ? 1 : 0, GetNumXCells(), GetNumYCells(),
                                               GetNumZCells(), cell_sizes.x(), add_virtual_border ? 1 : 0, fields.data(), nullptr, nullptr));
        }
        for (size_t b = 0; b < object_ids.size(); ++b) {
            SignedDistanceField new_sdf(SignedDistanceField::ForBuild{}, GetOriginTransform(), frame_, cell_sizes.x(), GetNumXCells(),
                                        GetNumYCells(), GetNumZCells(), std::numeric_limits<float>::infinity());
            std::memcpy(new_sdf.MutableDataForBuild(), fields.data() + b * n, n * sizeof(float));
            per_object_sdfs[object_ids[b]] = std::move(new_sdf);
        }
        return per_object_sdfs;
    }

    // ... for every object id > 0 present in the grid (:893-915).
    std::map<uint32_t, SignedDistanceField> MakeAllObjectSDFs(const bool unknown_is_filled, const bool add_virtual_border) const {
        std::map<uint32_t, uint32_t> object_id_map;
        for (const TAGGED_OBJECT_COLLISION_CELL& cell : data_)
            if (cell.object_id > 0) object_id_map[cell.object_id] = 1u;
        std::vector<uint32_t> ids;
        for (const auto& kv : object_id_map) ids.push_back(kv.first);
        return MakeObjectSDFs(ids, unknown_is_filled, add_virtual_border);
    }
};

}  // namespace sdf_tools
