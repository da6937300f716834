// CollisionMapGrid -- dense occupancy grid, API-compatible with the subset of
// sdf_tools::CollisionMapGrid (reference include/sdf_tools/collision_map.hpp) on the SDF path:
// COLLISION_CELL (:20-32), the constructors (:215-270), SetValue (:405-420) and
// ExtractSignedDistanceField (:680-712), and the connected components (UpdateConnectedComponents :564-618,
// ExtractConnectedComponents :757-778, GetNumConnectedComponents hpp :503) computed on the GPU by sdfgpu_components_cells,
// and their topology (ComputeComponentTopology :620-671, holes and voids per component) by sdfgpu_component_topology_cells.
// and the surface voxels of each component (ExtractComponentSurfaces :697-754 and its wrappers) by
// sdfgpu_component_surfaces_cells; CheckIfCandidateCorner (hpp :508-619) is a host query on the stored labels.
// Convex segments are out of scope.  The display export (ExportForDisplay and its kin, :317-562)
// selects on the GPU (include/sdfgpu.h "Display export", include/sdf_tools/display.hpp).  Wire formats (N3): SerializeSelf / DeserializeSelf, SaveToFile /
// LoadFromFile ("CMGZ" / "CMGR") and the CollisionMap message pair in the field order of
// src/sdf_tools/collision_map.cpp:21-62, :205-283, :285-315.  The byte layout of the primitives
// (arc_utilities::SerializeFixedSizePOD / SerializeEigen / SerializeVector / SerializeString) is the in-tree
// include/arc_utilities/serialization.hpp: arc_utilities is not vendored in the reference checkout, so byte-level
// interoperability with files written by the reference is UNVERIFIED.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <functional>
#include <iterator>
#include <stdexcept>
#include <string>
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

struct COLLISION_CELL {
    float occupancy;
    uint32_t component;
    COLLISION_CELL() : occupancy(0.0), component(0) {}
    explicit COLLISION_CELL(const float in_occupancy) : occupancy(in_occupancy), component(0) {}
    COLLISION_CELL(const float in_occupancy, const uint32_t in_component) : occupancy(in_occupancy), component(in_component) {}
};
static_assert(sizeof(COLLISION_CELL) == 8, "COLLISION_CELL must stay an 8-byte record (device classify kernel)");

// Plain mirror of msg/CollisionMap.msg for builds without ROS (field names kept).
struct CollisionMap {
    struct Header { uint32_t seq = 0; double stamp = 0.0; std::string frame_id; } header;
    std::vector<uint8_t> serialized_map;
    bool is_compressed = false;
};

class CollisionMapGrid : public VoxelGrid::VoxelGrid<COLLISION_CELL> {
protected:
    uint32_t number_of_components_;
    std::string frame_;
    bool components_valid_;

public:
    enum COMPONENT_TYPES : uint8_t { FILLED_COMPONENTS = 0x01, EMPTY_COMPONENTS = 0x02, UNKNOWN_COMPONENTS = 0x04 };

    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    using Base = ::VoxelGrid::VoxelGrid<COLLISION_CELL>;

    CollisionMapGrid(const Eigen::Isometry3d& origin_transform, const std::string& frame, const double resolution,
                     const int64_t x_cells, const int64_t y_cells, const int64_t z_cells, const COLLISION_CELL& oob_default_value)
        : Base(origin_transform, resolution, x_cells, y_cells, z_cells, oob_default_value), number_of_components_(0u), frame_(frame), components_valid_(false) {}
    CollisionMapGrid(const std::string& frame, const double resolution, const int64_t x_cells, const int64_t y_cells,
                     const int64_t z_cells, const COLLISION_CELL& oob_default_value)
        : Base(resolution, x_cells, y_cells, z_cells, oob_default_value), number_of_components_(0u), frame_(frame), components_valid_(false) {}
    CollisionMapGrid(const Eigen::Isometry3d& origin_transform, const std::string& frame, const double resolution,
                     const int64_t x_cells, const int64_t y_cells, const int64_t z_cells, const COLLISION_CELL& default_value,
                     const COLLISION_CELL& OOB_value)
        : Base(origin_transform, resolution, x_cells, y_cells, z_cells, default_value, OOB_value), number_of_components_(0u), frame_(frame), components_valid_(false) {}
    CollisionMapGrid(const Eigen::Isometry3d& origin_transform, const std::string& frame, const double resolution,
                     const double x_size, const double y_size, const double z_size, const COLLISION_CELL& oob_default_value)
        : Base(origin_transform, resolution, x_size, y_size, z_size, oob_default_value), number_of_components_(0u), frame_(frame), components_valid_(false) {}
    CollisionMapGrid() : Base(), number_of_components_(0u), frame_(""), components_valid_(false) {}

    Base* Clone() const override { return new CollisionMapGrid(*this); }

    double GetResolution() const { return GetCellSizes().x(); }
    std::string GetFrame() const { return frame_; }
    void SetFrame(const std::string& f) { frame_ = f; }
    bool AreComponentsValid() const { return components_valid_; }
    // For callers that write cells through GetMutableRawData() (SetValue does this itself): the stored components no longer
    // describe the grid, so the next UpdateConnectedComponents() recomputes them.
    void InvalidateConnectedComponents() { components_valid_ = false; }

    bool SetValue(const int64_t x, const int64_t y, const int64_t z, const COLLISION_CELL& value) override {
        if (!IndexInBounds(x, y, z)) return false;
        components_valid_ = false;
        AccessIndex(GetDataIndex(x, y, z)) = value;
        return true;
    }
    bool SetValue(const GRID_INDEX& i, const COLLISION_CELL& v) override { return SetValue(i.x, i.y, i.z, v); }
    bool SetValue4d(const Eigen::Vector4d& l, const COLLISION_CELL& v) override { return SetValue(LocationToGridIndex4d(l), v); }
    bool SetValue3d(const Eigen::Vector3d& l, const COLLISION_CELL& v) override { return SetValue(LocationToGridIndex3d(l), v); }
    bool SetValue(const double x, const double y, const double z, const COLLISION_CELL& v) override {
        return SetValue(LocationToGridIndex(x, y, z), v);
    }

    // occupancy > 0.5 is filled; == 0.5 is "unknown" and filled only on request (reference :689-704).
    // Every cell is in bounds by construction, so the reference's "index out of grid bounds" throw
    // (:707) cannot trigger; the raw cell array is classified on the device.
    std::pair<SignedDistanceField, std::pair<double, double>> ExtractSignedDistanceField(
        const float oob_value, const bool unknown_is_filled, const bool add_virtual_border) const {
        return sdf_generation::ExtractSignedDistanceFieldFromCells(
            GetOriginTransform(), GetCellSizes(), GetNumXCells(), GetNumYCells(), GetNumZCells(), data_.data(),
            sizeof(COLLISION_CELL), offsetof(COLLISION_CELL, occupancy), unknown_is_filled, oob_value, GetFrame(), add_virtual_border);
    }

    // The same build with the field left in HBM (round 4): batched EstimateDistance / GetGradient queries run on the
    // device, Host() downloads the reference's container lazily (include/sdf_tools/device_sdf.hpp).
    std::pair<DeviceSignedDistanceField, std::pair<double, double>> ExtractSignedDistanceFieldDevice(
        const float oob_value, const bool unknown_is_filled, const bool add_virtual_border) const {
        return sdf_generation::ExtractSignedDistanceFieldDeviceFromCells(
            GetOriginTransform(), GetCellSizes(), GetNumXCells(), GetNumYCells(), GetNumZCells(), data_.data(),
            sizeof(COLLISION_CELL), offsetof(COLLISION_CELL, occupancy), unknown_is_filled, oob_value, GetFrame(), add_virtual_border);
    }

    // ---- Resample (reference collision_map.cpp:673-695) -------------------------------------------------------------------------
    // A grid over the same volume at new_resolution: every cell, in x -> y -> z order, overwrites the result cell that holds its
    // centre (GPU: include/sdfgpu.h "Resample", bit for bit the host arithmetic).  Coarsening keeps the last such cell of the scan;
    // refining leaves the result cells that hold no source centre at the OOB value -- the reference's holes, kept.  The result's
    // components are invalid.  Throws std::invalid_argument when new_resolution is not positive and finite.
    CollisionMapGrid Resample(const double new_resolution) const { return ResampleGridFromCells(*this, new_resolution); }

    // ---- connected components (reference collision_map.cpp:564-618, :757-778) ---------------------------------------------
    // Two classes, occupancy > 0.5 and the rest (unknown and NaN join free space); 6-connectivity; components numbered 1..K in
    // the order of the x -> y -> z scan.  Labels are written into every cell's `component`; an early-out when the stored ones are
    // valid (also after deserialising a grid that carries them), as in the reference.
    uint32_t UpdateConnectedComponents() {
        if (components_valid_) return number_of_components_;
        uint32_t count = 0;
        if (!data_.empty()) {
            const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
            const std::lock_guard<std::mutex> lock(ctx->mutex);
            sdf_generation::ThrowOnStatus(
                ctx->handle, sdfgpu_components_cells(ctx->handle, data_.data(), sizeof(COLLISION_CELL), offsetof(COLLISION_CELL, occupancy),
                                                     offsetof(COLLISION_CELL, component), GetNumXCells(), GetNumYCells(),
                                                     GetNumZCells(), &count));
        }
        number_of_components_ = count;
        components_valid_ = true;
        return number_of_components_;
    }

    std::pair<uint32_t, bool> GetNumConnectedComponents() const { return std::make_pair(number_of_components_, components_valid_); }

    // ---- component topology (reference collision_map.cpp:620-671) ------------------------------------------------------------
    // {component: (holes, voids)} of the filled components (ignore_empty_components) or of every component, computed on the GPU
    // (include/sdfgpu.h "Component topology": the contract and its two deviations from the reference as written).  Labels are
    // recomputed first when asked (an early-out when the stored ones are valid); stored labels that are not valid are used as
    // they are, up to the largest of them.  Refusals throw std::invalid_argument, HIP failures std::runtime_error.
    std::map<uint32_t, std::pair<int32_t, int32_t>> ComputeComponentTopology(const bool ignore_empty_components,
                                                                             const bool recompute_connected_components,
                                                                             const bool verbose) {
        if (recompute_connected_components) UpdateConnectedComponents();
        uint32_t max_label = number_of_components_;
        if (!components_valid_) {
            max_label = 0;
            for (const COLLISION_CELL& cell : data_) max_label = cell.component > max_label ? cell.component : max_label;
        }
        return ComputeComponentTopologyFromCells(data_.data(), sizeof(COLLISION_CELL), offsetof(COLLISION_CELL, occupancy),
                                                 offsetof(COLLISION_CELL, component), GetNumXCells(), GetNumYCells(), GetNumZCells(),
                                                 ignore_empty_components ? FILLED_COMPONENTS : (FILLED_COMPONENTS | EMPTY_COMPONENTS | UNKNOWN_COMPONENTS),
                                                 max_label, verbose);
    }

    // ---- component surfaces (reference collision_map.cpp:697-754, collision_map.hpp:651-671) ---------------------------------------------------------------
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
            for (const COLLISION_CELL& cell : data_) max_label = cell.component > max_label ? cell.component : max_label;
        }
        return ExtractComponentSurfaceIndicesFromCells(data_.data(), sizeof(COLLISION_CELL), offsetof(COLLISION_CELL, occupancy),
                                                       offsetof(COLLISION_CELL, component), GetNumXCells(), GetNumYCells(), GetNumZCells(),
                                                       (int)component_types_to_extract, max_label);
    }

    // ---- display export (reference collision_map.cpp:317-562; include/sdf_tools/display.hpp) -----------------------------------------
    // Which cells are drawn, and in which order, comes from the GPU (include/sdfgpu.h "Display export"); a class whose colour has
    // alpha <= 0 is not drawn.  Points are GridIndexToLocationGridFrame of the cell, in the marker's pose = the origin transform.
    static std_msgs::ColorRGBA GenerateComponentColor(const uint32_t component, const float alpha = 1.0f) { return GenerateUniqueColor(component, alpha); }
    display::Cells DisplayCells() const {
        display::Cells c;
        c.data = data_.data(); c.stride = sizeof(COLLISION_CELL); c.occupancy_offset = offsetof(COLLISION_CELL, occupancy);
        c.nx = GetNumXCells(); c.ny = GetNumYCells(); c.nz = GetNumZCells(); c.cell_sizes = GetCellSizes();
        return c;
    }
    visualization_msgs::Marker DisplayMarker(const std::string& ns) const { return display::MakeMarker(frame_, ns, GetOriginTransform(), GetResolution()); }
    visualization_msgs::Marker ExportForDisplay(const std_msgs::ColorRGBA& collision_color, const std_msgs::ColorRGBA& free_color,
                                                const std_msgs::ColorRGBA& unknown_color) const {
        return display::ExportOccupancy(DisplayMarker("collision_map_display"), DisplayCells(), collision_color, free_color, unknown_color, false);
    }
    visualization_msgs::Marker ExportSurfacesForDisplay(const std_msgs::ColorRGBA& collision_color, const std_msgs::ColorRGBA& free_color,
                                                        const std_msgs::ColorRGBA& unknown_color) const {
        return display::ExportOccupancy(DisplayMarker("collision_map_display"), DisplayCells(), collision_color, free_color, unknown_color, true);
    }
    // collision, free and unknown cells as three markers, from one grouped selection
    visualization_msgs::MarkerArray ExportForSeparateDisplay(const std_msgs::ColorRGBA& collision_color, const std_msgs::ColorRGBA& free_color,
                                                             const std_msgs::ColorRGBA& unknown_color) const {
        static const char* const ns[3] = {"collision_only", "free_only", "unknown_only"};
        return display::ExportOccupancySeparate(DisplayMarker("collision_map_display"), DisplayCells(), collision_color, free_color, unknown_color, false, ns);
    }
    visualization_msgs::MarkerArray ExportSurfacesForSeparateDisplay(const std_msgs::ColorRGBA& collision_color,
                                                                     const std_msgs::ColorRGBA& free_color,
                                                                     const std_msgs::ColorRGBA& unknown_color) const {
        static const char* const ns[3] = {"collision_surfaces_only", "free_surfaces_only", "unknown_surfaces_only"};
        return display::ExportOccupancySeparate(DisplayMarker("collision_map_display"), DisplayCells(), collision_color, free_color, unknown_color, true, ns);
    }
    visualization_msgs::Marker ExportConnectedComponentsForDisplay(const bool color_unknown_components) const {
        return display::ExportComponents(DisplayMarker("connected_components_display"), DisplayCells(), data_, color_unknown_components);
    }

    // ---- candidate corners (reference collision_map.hpp:508-619): (two or more in-grid face neighbours of another component, index in the grid)
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

    // Indices of each component, in scan order inside each (one counting pass, then one placement pass over the labels).
    std::vector<std::vector<GRID_INDEX>> ExtractConnectedComponents() {
        if (!components_valid_) UpdateConnectedComponents();
        std::vector<size_t> sizes(number_of_components_, 0);
        for (const COLLISION_CELL& cell : data_) sizes.at(cell.component - 1) += 1;
        std::vector<std::vector<GRID_INDEX>> components(number_of_components_);
        for (size_t c = 0; c < components.size(); ++c) components[c].reserve(sizes[c]);
        const int64_t nx = GetNumXCells(), ny = GetNumYCells(), nz = GetNumZCells();
        size_t i = 0;
        for (int64_t x = 0; x < nx; ++x)
            for (int64_t y = 0; y < ny; ++y)
                for (int64_t z = 0; z < nz; ++z, ++i) components[data_[i].component - 1].emplace_back(x, y, z);
        return components;
    }

    // ---- wire formats: collision_map.cpp:21-62 (fields), :205-283 (files), :285-315 (messages) ------------------------
    using CellSerializer = std::function<uint64_t(const COLLISION_CELL&, std::vector<uint8_t>&)>;
    using CellDeserializer = std::function<std::pair<COLLISION_CELL, uint64_t>(const std::vector<uint8_t>&, const uint64_t)>;

    uint64_t SerializeSelf(std::vector<uint8_t>& buffer,
                           const CellSerializer& value_serializer = arc_utilities::SerializeFixedSizePOD<COLLISION_CELL>) const override {
        (void)value_serializer;                                   // (the reference ignores it too: cells are fixed-size PODs)
        const uint64_t start = buffer.size();
        BaseSerializeSelf(buffer, arc_utilities::SerializeFixedSizePOD<COLLISION_CELL>);   // initialized .. OOB value (:28-57)
        arc_utilities::SerializeFixedSizePOD<uint32_t>(number_of_components_, buffer);     // (:59)
        arc_utilities::SerializeString(frame_, buffer);                                    // (:60)
        arc_utilities::SerializeFixedSizePOD<uint8_t>((uint8_t)components_valid_, buffer); // (:61)
        return buffer.size() - start;
    }
    uint64_t DeserializeSelf(const std::vector<uint8_t>& buffer, const uint64_t current,
                             const CellDeserializer& value_deserializer = arc_utilities::DeserializeFixedSizePOD<COLLISION_CELL>) override {
        (void)value_deserializer;
        uint64_t pos = current;
        pos += BaseDeserializeSelf(buffer, pos, arc_utilities::DeserializeFixedSizePOD<COLLISION_CELL>);
        const auto nc = arc_utilities::DeserializeFixedSizePOD<uint32_t>(buffer, pos); pos += nc.second;
        const auto fr = arc_utilities::DeserializeString(buffer, pos); pos += fr.second;
        const auto cv = arc_utilities::DeserializeFixedSizePOD<uint8_t>(buffer, pos); pos += cv.second;
        number_of_components_ = nc.first;
        frame_ = fr.first;
        components_valid_ = (bool)cv.first;
        return pos - current;
    }

    static void SaveToFile(const CollisionMapGrid& map, const std::string& filepath, const bool compress) {
        std::vector<uint8_t> buffer;
        map.SerializeSelf(buffer);
        std::ofstream out(filepath, std::ios::out | std::ios::binary);
        const std::vector<uint8_t> body = compress ? ZlibHelpers::CompressBytes(buffer) : buffer;
        out.write(compress ? "CMGZ" : "CMGR", 4);                 // 4-byte magic (:214-229)
        out.write(reinterpret_cast<const char*>(body.data()), (std::streamsize)body.size());
    }
    static CollisionMapGrid LoadFromFile(const std::string& filepath) {
        std::ifstream in(filepath, std::ios::in | std::ios::binary);
        if (!in.good()) throw std::invalid_argument("File does not exist");
        std::vector<uint8_t> all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (all.size() < 4) throw std::invalid_argument("File is too small");
        const std::string magic(all.begin(), all.begin() + 4);
        const std::vector<uint8_t> body(all.begin() + 4, all.end());
        CollisionMapGrid map;
        if (magic == "CMGZ") map.DeserializeSelf(ZlibHelpers::DecompressBytes(body), 0);
        else if (magic == "CMGR") map.DeserializeSelf(body, 0);
        else throw std::invalid_argument("File has invalid header [" + magic + "]");
        return map;
    }
    static CollisionMap GetMessageRepresentation(const CollisionMapGrid& map) {
        CollisionMap msg;                                         // always zlib-compressed (:285-296); no ROS clock here: stamp stays 0
        msg.header.frame_id = map.GetFrame();
        std::vector<uint8_t> buffer;
        map.SerializeSelf(buffer);
        msg.serialized_map = ZlibHelpers::CompressBytes(buffer);
        msg.is_compressed = true;
        return msg;
    }
    static CollisionMapGrid LoadFromMessageRepresentation(const CollisionMap& message) {
        CollisionMapGrid map;
        if (message.is_compressed) map.DeserializeSelf(ZlibHelpers::DecompressBytes(message.serialized_map), 0);
        else map.DeserializeSelf(message.serialized_map, 0);
        return map;
    }

    // Same result through the generic predicate seam (kept for callers that pass their own predicate).
    std::pair<SignedDistanceField, std::pair<double, double>> ExtractSignedDistanceFieldViaPredicate(
        const float oob_value, const bool unknown_is_filled, const bool add_virtual_border) const {
        const std::function<bool(const GRID_INDEX&)> is_filled_fn = [&](const GRID_INDEX& index) {
            const auto query = GetImmutable(index);
            if (!query.second) throw std::runtime_error("index out of grid bounds");
            return (query.first.occupancy > 0.5) || (unknown_is_filled && (query.first.occupancy == 0.5));
        };
        return sdf_generation::ExtractSignedDistanceField(*this, is_filled_fn, oob_value, GetFrame(), add_virtual_border);
    }
};

// A batch of maps of ONE shape in one launch sequence (sdfgpu_build_batch): what a caller with many small environments uses in
// place of a loop over CollisionMapGrid::ExtractSignedDistanceField.  Each result carries its own map's origin, frame and
// resolution and equals that map's single call.  std::invalid_argument when the shapes differ or a map has non-uniform cells.
inline std::vector<std::pair<SignedDistanceField, std::pair<double, double>>> ExtractSignedDistanceFieldBatch(
    const std::vector<const CollisionMapGrid*>& maps, const float oob_value, const bool unknown_is_filled, const bool add_virtual_border) {
    std::vector<std::pair<SignedDistanceField, std::pair<double, double>>> results;
    if (maps.empty()) return results;
    const int64_t nx = maps[0]->GetNumXCells(), ny = maps[0]->GetNumYCells(), nz = maps[0]->GetNumZCells();
    const size_t n = (size_t)(nx * ny * nz), batch = maps.size();
    std::vector<double> resolutions(batch);
    std::vector<uint8_t> filled(batch * n);
    for (size_t b = 0; b < batch; ++b) {
        const CollisionMapGrid& map = *maps[b];
        if (map.GetNumXCells() != nx || map.GetNumYCells() != ny || map.GetNumZCells() != nz)
            throw std::invalid_argument("All grids of a batch must have the same shape");
        const Eigen::Vector3d cell_sizes = map.GetCellSizes();
        if ((cell_sizes.x() != cell_sizes.y()) || (cell_sizes.x() != cell_sizes.z()))
            throw std::invalid_argument("Grid must have uniform resolution");
        resolutions[b] = cell_sizes.x();
        const std::vector<COLLISION_CELL>& cells = map.GetImmutableRawData();       // the predicate of :689-704
        for (size_t i = 0; i < n; ++i)
            filled[b * n + i] = ((cells[i].occupancy > 0.5f) || (unknown_is_filled && (cells[i].occupancy == 0.5f))) ? 1 : 0;
    }
    if (n == 0) throw std::invalid_argument("Grid must not be empty");
    std::vector<float> fields(batch * n);
    std::vector<double> mx(batch), mn(batch);
    {
        const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
        const std::lock_guard<std::mutex> lock(ctx->mutex);
        sdf_generation::ThrowOnStatus(ctx->handle, sdfgpu_build_batch(ctx->handle, filled.data(), (int64_t)batch, nx, ny, nz, resolutions[0],
                                                                      resolutions.data(), add_virtual_border ? 1 : 0, fields.data(),
                                                                      mx.data(), mn.data()));
    }
    results.reserve(batch);
    for (size_t b = 0; b < batch; ++b) {
        SignedDistanceField new_sdf(SignedDistanceField::ForBuild{}, maps[b]->GetOriginTransform(), maps[b]->GetFrame(), resolutions[b], nx,
                                    ny, nz, oob_value);
        std::memcpy(new_sdf.MutableDataForBuild(), fields.data() + b * n, n * sizeof(float));
        results.emplace_back(std::move(new_sdf), std::make_pair(mx[b], mn[b]));
    }
    return results;
}

}  // namespace sdf_tools
