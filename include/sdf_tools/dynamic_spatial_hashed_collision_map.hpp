// DynamicSpatialHashedCollisionMapGrid -- the reference's class of the same name (include/sdf_tools/dynamic_spatial_hashed_collision_map.hpp,
// src/sdf_tools/dynamic_spatial_hashed_collision_map.cpp) over the device-resident map of include/sdfgpu.h "Dynamic spatial hashed map":
// the reference's constructors and methods with their signatures, and batch forms beside them (SetCells, SetChunks, GetBatch,
// InsertPointCloud, the window extractions), which are what the map is for -- one SetCell per call costs a kernel launch sequence.
//
// The reference keeps its cells in arc_utilities' DynamicSpatialHashedVoxelGrid, which this project has never seen: the contract
// (location -> cell by floor, chunk states, what Get and the setters return) is this project's own, DESIGN.md section 29, UNVERIFIED
// against that class.  So are the values of VoxelGrid::FOUND_STATUS / SET_STATUS below, and the place of a chunk's marker: the
// reference asks the chunk for the location of its index (0, 0, 0); here the marker sits at the chunk's centre, where a cube of the
// chunk's size covers the chunk.
//
// Uninitialised maps: the reference's default constructor leaves the underlying grid empty.  Here Get on such a map returns
// (COLLISION_CELL(), NOT_FOUND), the setters return NOT_SET, the batch forms and extractions throw std::runtime_error and
// ExportForDisplay returns no marker.  (The reference's two other constructors never set initialized_; here they do.)
#pragma once
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sdf_tools/collision_map.hpp"
#include "sdf_tools/device_sdf.hpp"
#include "sdf_tools/display.hpp"
#include "sdf_tools/gpu_context.hpp"
#include "sdfgpu.h"

namespace VoxelGrid {
enum FOUND_STATUS { NOT_FOUND = SDFGPU_DSH_NOT_FOUND, FOUND_IN_CHUNK = SDFGPU_DSH_FOUND_IN_CHUNK, FOUND_IN_CELL = SDFGPU_DSH_FOUND_IN_CELL };
enum SET_STATUS { NOT_SET = SDFGPU_DSH_NOT_SET, SET_CHUNK = SDFGPU_DSH_SET_CHUNK, SET_CELL = SDFGPU_DSH_SET_CELL };
}  // namespace VoxelGrid

namespace sdf_tools {

class DynamicSpatialHashedCollisionMapGrid {
protected:
    // the device map and the context it lives on (shared by copies of the grid: a copy is another name for the same map)
    struct DeviceMap {
        std::shared_ptr<sdf_generation::SharedGpuContext> ctx;
        sdfgpu_dsh_map map = nullptr;
        ~DeviceMap() {
            if (!map) return;
            const std::lock_guard<std::mutex> lock(ctx->mutex);
            sdfgpu_dsh_destroy(map);
        }
    };
    std::shared_ptr<DeviceMap> collision_field_;
    Eigen::Isometry3d origin_transform_;
    double resolution_ = 0.0;
    int64_t chunk_sizes_[3] = {0, 0, 0};
    COLLISION_CELL default_value_;
    uint32_t number_of_components_;
    std::string frame_;
    bool initialized_;
    bool components_valid_;

    void Create(const uint64_t byte_limit) {
        std::shared_ptr<DeviceMap> fresh = std::make_shared<DeviceMap>();
        fresh->ctx = sdf_generation::GpuContext::Shared();
        const Eigen::Isometry3d inverse = origin_transform_.inverse();
        double inv16[16];
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) inv16[4 * r + c] = inverse.matrix()(r, c);
        const std::lock_guard<std::mutex> lock(fresh->ctx->mutex);
        sdf_generation::ThrowOnStatus(fresh->ctx->handle, sdfgpu_dsh_create(fresh->ctx->handle, inv16, resolution_, chunk_sizes_[0], chunk_sizes_[1],
                                                                            chunk_sizes_[2], &default_value_, 0, byte_limit, &fresh->map));
        collision_field_ = std::move(fresh);
        initialized_ = true;
    }
    void RequireInitialized() const {
        if (!initialized_) throw std::runtime_error("DynamicSpatialHashedCollisionMapGrid is not initialized");
    }
    template <typename Call>
    void Locked(Call call) const {
        const std::lock_guard<std::mutex> lock(collision_field_->ctx->mutex);
        sdf_generation::ThrowOnStatus(collision_field_->ctx->handle, call(collision_field_->map));
    }

public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW

    DynamicSpatialHashedCollisionMapGrid(std::string frame, double resolution, int64_t chunk_x_size, int64_t chunk_y_size, int64_t chunk_z_size,
                                         COLLISION_CELL OOB_value)
        : DynamicSpatialHashedCollisionMapGrid(Eigen::Isometry3d::Identity(), std::move(frame), resolution, chunk_x_size, chunk_y_size, chunk_z_size, OOB_value) {}

    DynamicSpatialHashedCollisionMapGrid(Eigen::Isometry3d origin_transform, std::string frame, double resolution, int64_t chunk_x_size,
                                         int64_t chunk_y_size, int64_t chunk_z_size, COLLISION_CELL OOB_value, uint64_t byte_limit = 0)
        : origin_transform_(origin_transform), resolution_(resolution), default_value_(OOB_value), number_of_components_(0), frame_(std::move(frame)),
          initialized_(false), components_valid_(false) {
        chunk_sizes_[0] = chunk_x_size; chunk_sizes_[1] = chunk_y_size; chunk_sizes_[2] = chunk_z_size;
        Create(byte_limit);
    }

    DynamicSpatialHashedCollisionMapGrid() : number_of_components_(0), initialized_(false), components_valid_(false) {}

    bool IsInitialized() const { return initialized_; }
    // Whether the component words of the map's records are those of the last UpdateConnectedComponents (an addition: no method of
    // the reference computes them).  The MAP keeps that, not this object: two copies of a grid are two names for one map and agree.
    // False before any update, after any call that set or removed something, and on an uninitialised map.  (number_of_components_
    // and components_valid_ keep the reference's layout; the setters still clear the flag, but the map's answer is the truth.)
    bool AreComponentsValid() const { return ComponentsInfo().valid; }
    std::string GetFrame() const { return frame_; }
    double GetResolution() const { return resolution_; }
    std::vector<double> GetCellSizes() const { return {resolution_, resolution_, resolution_}; }
    std::vector<double> GetChunkSizes() const {
        return {resolution_ * (double)chunk_sizes_[0], resolution_ * (double)chunk_sizes_[1], resolution_ * (double)chunk_sizes_[2]};
    }
    std::vector<int64_t> GetChunkNumCells() const { return {chunk_sizes_[0], chunk_sizes_[1], chunk_sizes_[2]}; }
    COLLISION_CELL GetDefaultValue() const { return default_value_; }
    Eigen::Isometry3d GetOriginTransform() const { return origin_transform_; }
    // the C ABI's map, for callers of the *_device entry points (hold Context()->mutex around such calls)
    sdfgpu_dsh_map DeviceMapHandle() const { return collision_field_ ? collision_field_->map : nullptr; }
    std::shared_ptr<sdf_generation::SharedGpuContext> Context() const { return collision_field_ ? collision_field_->ctx : nullptr; }

    // ---- the reference's accessors ----------------------------------------------------------------------------------------------------
    std::pair<COLLISION_CELL, VoxelGrid::FOUND_STATUS> Get(const double x, const double y, const double z) const {
        if (!initialized_) return std::make_pair(COLLISION_CELL(), VoxelGrid::NOT_FOUND);
        const double location[3] = {x, y, z};
        COLLISION_CELL cell;
        uint8_t status = 0;
        Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_get(m, location, 1, &cell, &status); });
        return std::make_pair(cell, (VoxelGrid::FOUND_STATUS)status);
    }
    std::pair<COLLISION_CELL, VoxelGrid::FOUND_STATUS> Get(const Eigen::Vector3d& location) const { return Get(location.x(), location.y(), location.z()); }

    VoxelGrid::SET_STATUS SetCell(const double x, const double y, const double z, COLLISION_CELL value) {
        if (!initialized_) return VoxelGrid::NOT_SET;
        const double location[3] = {x, y, z};
        uint8_t status = 0;
        Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_set_cells(m, location, 1, nullptr, &value, &status); });
        if (status != VoxelGrid::NOT_SET) components_valid_ = false;
        return (VoxelGrid::SET_STATUS)status;
    }
    VoxelGrid::SET_STATUS SetCell(const Eigen::Vector3d& location, COLLISION_CELL value) { return SetCell(location.x(), location.y(), location.z(), value); }

    VoxelGrid::SET_STATUS SetChunk(const double x, const double y, const double z, COLLISION_CELL value) {
        if (!initialized_) return VoxelGrid::NOT_SET;
        const double location[3] = {x, y, z};
        uint8_t status = 0;
        Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_set_chunks(m, location, 1, nullptr, &value, &status); });
        if (status != VoxelGrid::NOT_SET) components_valid_ = false;
        return (VoxelGrid::SET_STATUS)status;
    }
    VoxelGrid::SET_STATUS SetChunk(const Eigen::Vector3d& location, COLLISION_CELL value) { return SetChunk(location.x(), location.y(), location.z(), value); }

    // ---- batches (additions): as if applied one after the other in list order ------------------------------------------------------------
    // locations_xyz: n x 3 doubles; values: one record for the whole batch, or one per location.  Returns the statuses.
    std::vector<VoxelGrid::SET_STATUS> SetCells(const std::vector<double>& locations_xyz, const std::vector<COLLISION_CELL>& values) {
        return SetBatch(false, locations_xyz, values);
    }
    std::vector<VoxelGrid::SET_STATUS> SetChunks(const std::vector<double>& locations_xyz, const std::vector<COLLISION_CELL>& values) {
        return SetBatch(true, locations_xyz, values);
    }
    std::pair<std::vector<COLLISION_CELL>, std::vector<VoxelGrid::FOUND_STATUS>> GetBatch(const std::vector<double>& locations_xyz) const {
        RequireInitialized();
        if (locations_xyz.size() % 3) throw std::invalid_argument("GetBatch: locations are x, y, z triples");
        const size_t n = locations_xyz.size() / 3;
        std::vector<COLLISION_CELL> cells(n);
        std::vector<uint8_t> raw(n);
        if (n) Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_get(m, locations_xyz.data(), (int64_t)n, cells.data(), raw.data()); });
        std::vector<VoxelGrid::FOUND_STATUS> statuses(n);
        for (size_t i = 0; i < n; ++i) statuses[i] = (VoxelGrid::FOUND_STATUS)raw[i];
        return std::make_pair(std::move(cells), std::move(statuses));
    }
    // A point cloud (n x 3 floats, as a depth camera delivers it) as cell sets of one value; returns how many points were set.
    size_t InsertPointCloud(const std::vector<float>& points_xyz, const COLLISION_CELL value) {
        RequireInitialized();
        if (points_xyz.size() % 3) throw std::invalid_argument("InsertPointCloud: points are x, y, z triples");
        const size_t n = points_xyz.size() / 3;
        if (!n) return 0;
        const std::lock_guard<std::mutex> lock(collision_field_->ctx->mutex);
        sdfgpu_handle h = collision_field_->ctx->handle;
        void* d_points = nullptr;
        void* d_statuses = nullptr;
        std::vector<uint8_t> statuses(n);
        int rc = sdfgpu_device_malloc(h, n * 12, &d_points);
        if (rc == SDFGPU_OK) rc = sdfgpu_device_malloc(h, n, &d_statuses);
        if (rc == SDFGPU_OK) rc = sdfgpu_copy_from_host(h, d_points, points_xyz.data(), n * 12, nullptr);
        if (rc == SDFGPU_OK) rc = sdfgpu_dsh_insert_points_device(collision_field_->map, static_cast<const float*>(d_points), (int64_t)n, &value,
                                                                  static_cast<uint8_t*>(d_statuses), nullptr);
        if (rc == SDFGPU_OK) rc = sdfgpu_copy_to_host(h, statuses.data(), d_statuses, n, nullptr);
        const std::string message = rc == SDFGPU_OK ? "" : sdfgpu_last_error(h);
        (void)sdfgpu_device_free(h, d_points);
        (void)sdfgpu_device_free(h, d_statuses);
        if (rc == SDFGPU_ERR_INVALID_ARGUMENT) throw std::invalid_argument("sdfgpu: " + message);
        if (rc != SDFGPU_OK) throw std::runtime_error("sdfgpu: " + message);
        size_t set = 0;
        for (const uint8_t s : statuses) set += s != VoxelGrid::NOT_SET;
        if (set) components_valid_ = false;
        return set;
    }

    // One frame of a range sensor (an addition; include/sdfgpu.h "Sensor rays"): the cells between
    // sensor_origin and each point become free_value, then the points' cells become filled_value; a point beyond max_range carves
    // up to that range and fills nothing, a point that is not finite is skipped.  max_range must span more than 0 and at most 65536
    // cells, and the sensor must be a valid location: otherwise std::invalid_argument, and nothing is written.  Returns the frame's
    // counts.  The contract is this project's own, UNVERIFIED against octomap's insertPointCloud.
    sdfgpu_dsh_ray_counts InsertPointCloudRays(const std::vector<float>& points_xyz, const Eigen::Vector3d& sensor_origin, const double max_range,
                                               const COLLISION_CELL free_value, const COLLISION_CELL filled_value) {
        RequireInitialized();
        if (points_xyz.size() % 3) throw std::invalid_argument("InsertPointCloudRays: points are x, y, z triples");
        const double sensor[3] = {sensor_origin.x(), sensor_origin.y(), sensor_origin.z()};
        sdfgpu_dsh_ray_counts counts = sdfgpu_dsh_ray_counts();
        Locked([&](sdfgpu_dsh_map m) {
            return sdfgpu_dsh_insert_rays(m, sensor, points_xyz.data(), (int64_t)(points_xyz.size() / 3), max_range, &free_value, &filled_value, nullptr, &counts);
        });
        if (counts.rays_hit + counts.rays_truncated) components_valid_ = false;
        return counts;
    }

    // The sensor model of FusePointCloudRays: how much one return (prob_hit) and one ray passing through (prob_miss) say about a
    // cell, and where the occupancy is clamped.  The defaults are octomap's.  All four lie in [0.001, 0.999], clamp_min <= clamp_max.
    struct SensorModel {
        float prob_hit, prob_miss, clamp_min, clamp_max;
        SensorModel() : prob_hit(0.7f), prob_miss(0.4f), clamp_min(0.12f), clamp_max(0.97f) {}
        SensorModel(float hit, float miss, float min, float max) : prob_hit(hit), prob_miss(miss), clamp_min(min), clamp_max(max) {}
    };

    // One frame of a range sensor fused into the occupancies (an addition; include/sdfgpu.h "Sensor rays: fusion", DESIGN.md section
    // 31): the rays are those of InsertPointCloudRays, but every cell they pass is updated once with prob_miss and every cell a
    // point falls into once with prob_hit (Bayes' rule on the clamped occupancy; the component word of a cell is kept), so evidence
    // accumulates over frames where InsertPointCloudRays overwrites.  std::invalid_argument, and nothing written, for a model outside
    // its domain and for what InsertPointCloudRays refuses.  Returns the frame's counts.  The contract is this project's own,
    // UNVERIFIED against octomap's insertPointCloud.
    sdfgpu_dsh_ray_counts FusePointCloudRays(const std::vector<float>& points_xyz, const Eigen::Vector3d& sensor_origin, const double max_range,
                                             const SensorModel model = SensorModel()) {
        RequireInitialized();
        if (points_xyz.size() % 3) throw std::invalid_argument("FusePointCloudRays: points are x, y, z triples");
        const double sensor[3] = {sensor_origin.x(), sensor_origin.y(), sensor_origin.z()};
        const sdfgpu_dsh_sensor_model raw = {model.prob_hit, model.prob_miss, model.clamp_min, model.clamp_max};
        sdfgpu_dsh_ray_counts counts = sdfgpu_dsh_ray_counts();
        Locked([&](sdfgpu_dsh_map m) {
            return sdfgpu_dsh_fuse_rays(m, sensor, points_xyz.data(), (int64_t)(points_xyz.size() / 3), max_range, &raw, nullptr, &counts);
        });
        if (counts.rays_hit + counts.rays_truncated) components_valid_ = false;
        return counts;
    }

    // ---- removal (additions; include/sdfgpu.h "Removal") ------------------------------------------------------------
    // A removed chunk is absent again: Get says NOT_FOUND, a window reads the default.  On an uninitialised map RemoveChunk returns
    // false and Clear 0; the others throw std::runtime_error, as the batch forms do.
    bool RemoveChunk(const double x, const double y, const double z) {
        if (!initialized_) return false;
        const double location[3] = {x, y, z};
        int64_t removed = 0;
        Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_remove_chunks(m, location, 1, nullptr, &removed); });
        if (removed) components_valid_ = false;
        return removed != 0;
    }
    bool RemoveChunk(const Eigen::Vector3d& location) { return RemoveChunk(location.x(), location.y(), location.z()); }
    // locations_xyz: n x 3 doubles, removed in list order; true for the first location that names a live chunk
    std::vector<bool> RemoveChunks(const std::vector<double>& locations_xyz) {
        RequireInitialized();
        if (locations_xyz.size() % 3) throw std::invalid_argument("RemoveChunks: locations are x, y, z triples");
        const size_t n = locations_xyz.size() / 3;
        std::vector<uint8_t> raw(n);
        int64_t removed = 0;
        if (n) Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_remove_chunks(m, locations_xyz.data(), (int64_t)n, raw.data(), &removed); });
        if (removed) components_valid_ = false;
        std::vector<bool> statuses(n);
        for (size_t i = 0; i < n; ++i) statuses[i] = raw[i] == SDFGPU_DSH_CHUNK_REMOVED;
        return statuses;
    }
    // Keep the chunks that hold at least one of the nx x ny x nz cells from global cell lower_index on, remove every other one
    // (RemoveBox: the other way round).  Returns how many chunks were removed.
    int64_t RetainBox(const VoxelGrid::GRID_INDEX& lower_index, const int64_t nx, const int64_t ny, const int64_t nz) {
        return BoxRemoval(lower_index, nx, ny, nz, 0);
    }
    int64_t RemoveBox(const VoxelGrid::GRID_INDEX& lower_index, const int64_t nx, const int64_t ny, const int64_t nz) {
        return BoxRemoval(lower_index, nx, ny, nz, 1);
    }
    int64_t Clear() { return initialized_ ? BoxRemoval(VoxelGrid::GRID_INDEX(0, 0, 0), 0, 0, 0, 0) : 0; }
    // Hand memory back: the pool keeps room for the live chunks and spare_chunks more, the table follows.
    void ShrinkToFit(const int64_t spare_chunks = 0) {
        RequireInitialized();
        Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_shrink(m, spare_chunks, nullptr); });
    }

    // ---- connected components (additions; include/sdfgpu.h "Dynamic spatial hashed map: connected components") -------
    // Labels the connected components of the WHOLE map in place: every cell of a cell-filled chunk and every chunk-filled chunk (one
    // node) gets its component's number in 1..K in the component word of its record, which Get, GetBatch, ExtractCollisionMapGrid
    // and Export then hand out.  Nodes are joined iff they are of the same class and 6-face neighbours in global cell coordinates,
    // across chunk borders too; cells of absent chunks connect nothing.  Classes: filled (occupancy > 0.5) and everything else, as
    // CollisionMapGrid::UpdateConnectedComponents; with unknown_apart filled, free (< 0.5) and the rest (0.5 and NaN), so that known-free
    // space is not joined with never-seen cells of live chunks.  Components are numbered by their first node in Export's order.
    // Returns K; the stored K, without any launch, when the map says it is still valid under the same rule; 0 on an uninitialised
    // map.  A map of 2^32 - 1 nodes or more is refused (std::runtime_error).  The contract is this project's own, UNVERIFIED.
    uint32_t UpdateConnectedComponents(const bool unknown_apart = false) {
        if (!initialized_) return 0;
        const uint32_t flags = unknown_apart ? (uint32_t)SDFGPU_DSH_COMPONENTS_UNKNOWN_APART : 0u;
        const Components now = ComponentsInfo();
        uint32_t count = now.count;
        if (!(now.valid && now.flags == flags)) Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_update_components(m, flags, &count, nullptr); });
        number_of_components_ = count;
        components_valid_ = true;
        return count;
    }
    // (K of the last update, whether it still holds): (0, false) before any update and on an uninitialised map
    std::pair<uint32_t, bool> GetNumConnectedComponents() const {
        const Components now = ComponentsInfo();
        return std::make_pair(now.count, now.valid);
    }

    // ---- ray casts (additions; include/sdfgpu.h "Ray casts") -----------------------------------------------------------
    // What a ray meets first: the walk of InsertPointCloudRays, read-only, stopped at the first cell whose record satisfies the
    // CollisionMapGrid predicate (occupancy > 0.5, or == 0.5 with unknown_is_filled).  skip_first leaves the start's cell untested,
    // skip_last the end's; both together ask whether the segment between two cells is clear.  max_range must span more than 0 and at
    // most 65536 cells, and CastRays' sensor must be a valid location: otherwise std::invalid_argument.  A ray with an invalid end
    // is SKIPPED.  The contract is this project's own, UNVERIFIED against octomap's castRay.
    enum CAST_STATUS { CAST_SKIPPED = SDFGPU_DSH_CAST_SKIPPED, CAST_CLEAR = SDFGPU_DSH_CAST_CLEAR, CAST_CLEAR_IN_RANGE = SDFGPU_DSH_CAST_CLEAR_IN_RANGE,
                       CAST_BLOCKED = SDFGPU_DSH_CAST_BLOCKED };
    struct RayCast {
        CAST_STATUS status;               // BLOCKED: the fields below describe the blocker; CLEAR / CLEAR_IN_RANGE: the last cell walked
        VoxelGrid::GRID_INDEX cell;       // global cell index (the coordinates of the window extractions' lower_index)
        COLLISION_CELL value;             // what Get returns there
        VoxelGrid::FOUND_STATUS found;
        double t;                         // the fraction of start -> end at which the ray enters the cell (0 for the start's cell)
        uint32_t step;                    // the cell's place in the walk
        double distance;                  // t * sqrt((dx dx + dy dy) + dz dz) of end - start in world units, in double on the host
    };
    std::vector<RayCast> CastRays(const std::vector<float>& points_xyz, const Eigen::Vector3d& sensor_origin, const double max_range,
                                  const bool unknown_is_filled, const bool skip_first = false, const bool skip_last = false) const {
        RequireInitialized();
        if (points_xyz.size() % 3) throw std::invalid_argument("CastRays: points are x, y, z triples");
        const size_t n = points_xyz.size() / 3;
        const double sensor[3] = {sensor_origin.x(), sensor_origin.y(), sensor_origin.z()};
        std::vector<uint8_t> statuses(n);
        std::vector<sdfgpu_dsh_cast_hit> hits(n);
        uint8_t no_status = 0;                                                 // (an output must be given, with no ray too)
        Locked([&](sdfgpu_dsh_map m) {
            return sdfgpu_dsh_cast_rays(m, sensor, points_xyz.data(), (int64_t)n, max_range, CastFlags(unknown_is_filled, skip_first, skip_last),
                                        n ? statuses.data() : &no_status, hits.data());
        });
        std::vector<RayCast> casts(n);
        for (size_t i = 0; i < n; ++i) {
            const double end[3] = {(double)points_xyz[3 * i], (double)points_xyz[3 * i + 1], (double)points_xyz[3 * i + 2]};
            casts[i] = MakeRayCast(statuses[i], hits[i], sensor, end);
        }
        return casts;
    }
    std::vector<RayCast> CastSegments(const std::vector<double>& starts_xyz, const std::vector<double>& ends_xyz, const double max_range,
                                      const bool unknown_is_filled, const bool skip_first = false, const bool skip_last = false) const {
        RequireInitialized();
        if (starts_xyz.size() % 3 || starts_xyz.size() != ends_xyz.size()) throw std::invalid_argument("CastSegments: starts and ends are as many x, y, z triples");
        const size_t n = starts_xyz.size() / 3;
        std::vector<uint8_t> statuses(n);
        std::vector<sdfgpu_dsh_cast_hit> hits(n);
        uint8_t no_status = 0;
        Locked([&](sdfgpu_dsh_map m) {
            return sdfgpu_dsh_cast_segments(m, starts_xyz.data(), ends_xyz.data(), (int64_t)n, max_range, CastFlags(unknown_is_filled, skip_first, skip_last),
                                            n ? statuses.data() : &no_status, hits.data());
        });
        std::vector<RayCast> casts(n);
        for (size_t i = 0; i < n; ++i) casts[i] = MakeRayCast(statuses[i], hits[i], starts_xyz.data() + 3 * i, ends_xyz.data() + 3 * i);
        return casts;
    }
    RayCast CastRay(const Eigen::Vector3d& origin, const Eigen::Vector3d& end, const double max_range, const bool unknown_is_filled,
                    const bool skip_first = false, const bool skip_last = false) const {
        return CastSegments({origin.x(), origin.y(), origin.z()}, {end.x(), end.y(), end.z()}, max_range, unknown_is_filled, skip_first, skip_last)[0];
    }

    // ---- dense windows (additions) ------------------------------------------------------------------------------------------------------
    // The nx x ny x nz cells from global cell lower_index on as a CollisionMapGrid: cell (x, y, z) is what Get returns there.  The
    // result's origin is the map's origin times the translation to that corner; its OOB value is the map's default.
    CollisionMapGrid ExtractCollisionMapGrid(const VoxelGrid::GRID_INDEX& lower_index, const int64_t nx, const int64_t ny, const int64_t nz) const {
        RequireInitialized();
        if (nx <= 0 || ny <= 0 || nz <= 0) throw std::invalid_argument("ExtractCollisionMapGrid: cell counts must be positive");
        CollisionMapGrid grid(WindowOrigin(lower_index), frame_, resolution_, nx, ny, nz, default_value_);
        const int64_t lower[3] = {lower_index.x, lower_index.y, lower_index.z};
        Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_extract_window(m, lower, nx, ny, nz, 0, grid.GetMutableRawData().data(), nullptr); });
        return grid;
    }
    // The SDF of a window, built from the window's bit field without a cell record leaving the device.
    std::pair<DeviceSignedDistanceField, std::pair<double, double>> ExtractSignedDistanceFieldDevice(
        const VoxelGrid::GRID_INDEX& lower_index, const int64_t nx, const int64_t ny, const int64_t nz, const float oob_value,
        const bool unknown_is_filled, const bool add_virtual_border) const {
        RequireInitialized();
        DeviceSignedDistanceField sdf(WindowOrigin(lower_index), frame_, resolution_, nx, ny, nz, oob_value);
        if (sdf.Context() != collision_field_->ctx) throw std::runtime_error("DynamicSpatialHashedCollisionMapGrid: the map lives on another thread's GPU context");
        const int64_t lower[3] = {lower_index.x, lower_index.y, lower_index.z};
        double max_distance = 0.0, min_distance = 0.0;
        int rc = SDFGPU_OK;
        std::string message;
        {   // (the lock is released before anything is thrown: the field's destructor takes it)
            const std::lock_guard<std::mutex> lock(collision_field_->ctx->mutex);
            sdfgpu_handle h = collision_field_->ctx->handle;
            void* d_bits = nullptr;
            rc = sdfgpu_device_malloc(h, (size_t)((nx * ny * nz + 31) / 32) * 4, &d_bits);
            if (rc == SDFGPU_OK) rc = sdfgpu_dsh_extract_window_device(collision_field_->map, lower, nx, ny, nz, unknown_is_filled ? 1 : 0, nullptr,
                                                                       static_cast<uint32_t*>(d_bits), nullptr);
            if (rc == SDFGPU_OK) rc = sdfgpu_build_bits_device(h, static_cast<const uint32_t*>(d_bits), nx, ny, nz, resolution_, add_virtual_border ? 1 : 0,
                                                               sdf.DevicePointer(), nullptr);
            if (rc == SDFGPU_OK) rc = sdfgpu_get_extrema(h, &max_distance, &min_distance);
            if (rc != SDFGPU_OK) message = sdfgpu_last_error(h);
            (void)sdfgpu_device_free(h, d_bits);
        }
        if (rc == SDFGPU_ERR_INVALID_ARGUMENT) throw std::invalid_argument("sdfgpu: " + message);
        if (rc != SDFGPU_OK) throw std::runtime_error("sdfgpu: " + message);
        sdf.SetExtrema(std::make_pair(max_distance, min_distance));
        return std::make_pair(std::move(sdf), std::make_pair(max_distance, min_distance));
    }
    std::pair<SignedDistanceField, std::pair<double, double>> ExtractSignedDistanceField(
        const VoxelGrid::GRID_INDEX& lower_index, const int64_t nx, const int64_t ny, const int64_t nz, const float oob_value,
        const bool unknown_is_filled, const bool add_virtual_border) const {
        std::pair<DeviceSignedDistanceField, std::pair<double, double>> device =
            ExtractSignedDistanceFieldDevice(lower_index, nx, ny, nz, oob_value, unknown_is_filled, add_virtual_border);
        return std::make_pair(device.first.Host(), device.second);
    }

    // ---- frontier cells (additions; include/sdfgpu.h "Frontier cells") ----------------------------------------------------
    // Where seen-free space ends in never-seen space: a frontier cell is a cell of a live chunk that is free (occupancy < 0.5) and
    // has an unknown neighbour (occupancy == 0.5) among its 6 face neighbours, or among all 26 with use_26.  Neighbours are read
    // wherever they lie (an absent chunk reads as the default); a window or a box only restricts which cells are candidates.
    // A refusal of the library (a window of more than 2^32 - 1 cells, cell counts below 1) is std::invalid_argument.
    //
    // The frontier cells of the whole map as global cell indices (the coordinates of the window extractions' lower_index), chunks in
    // ascending (c_x, c_y, c_z) order and cells x -> y -> z inside a chunk.
    std::vector<VoxelGrid::GRID_INDEX> ExtractFrontierCells(const bool use_26 = false) const { return FrontierCells(nullptr, nullptr, use_26); }
    // ... among the nx x ny x nz cells from global cell lower_index on
    std::vector<VoxelGrid::GRID_INDEX> ExtractFrontierCells(const VoxelGrid::GRID_INDEX& lower_index, const int64_t nx, const int64_t ny, const int64_t nz,
                                                            const bool use_26 = false) const {
        const int64_t lower[3] = {lower_index.x, lower_index.y, lower_index.z}, extent[3] = {nx, ny, nz};
        return FrontierCells(lower, extent, use_26);
    }
    // The frontier cells of a window as the bit field of sdfgpu_build_bits_device: bit (x ny + y) nz + z is set iff global cell
    // lower_index + (x, y, z) is a frontier cell; ceil(nx ny nz / 32) words.  (A caller that keeps going on the device calls
    // sdfgpu_dsh_frontier_window_device on DeviceMapHandle() itself, as ExtractFrontierClusters does.)
    std::vector<uint32_t> ExtractFrontierWindowBits(const VoxelGrid::GRID_INDEX& lower_index, const int64_t nx, const int64_t ny, const int64_t nz,
                                                    const bool use_26 = false) const {
        RequireInitialized();
        const int64_t lower[3] = {lower_index.x, lower_index.y, lower_index.z};
        if (!WindowCountsOk(nx, ny, nz)) throw std::invalid_argument("ExtractFrontierWindowBits: cell counts must be positive and span at most 2^32 - 1 cells");
        std::vector<uint32_t> bits((size_t)((nx * ny * nz + 31) / 32));
        Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_frontier_window(m, lower, nx, ny, nz, FrontierFlags(use_26), bits.data()); });
        return bits;
    }
    // One connected piece of a window's frontier.  Pieces are 6-connected components of the window's frontier cells, which is what
    // the project's components are (sdfgpu_components_bits_device), whichever rule found the cells: under the 6-rule a frontier
    // tends to fall apart along the diagonal steps of a surface, which is why use_26 defaults to true here.
    struct FrontierCluster {
        uint32_t label;                       // of sdfgpu_components_bits_device on the window's frontier bits
        int64_t cells;
        VoxelGrid::GRID_INDEX lower, upper;   // bounding box in global cells, inclusive
        Eigen::Vector3d centroid;             // the mean of the cells' centres in world coordinates, in double on the host:
                                              // g_a = ((double)lower_index_a + ((double)sum_a / (double)cells + 0.5)) * resolution, sum_a the sum of the
                                              // cells' window coordinates along a; centroid = origin_transform * (g_x, g_y, g_z)
    };
    // The clusters of at least min_cells cells among the frontier cells of a window, in label order: window bits -> components ->
    // statistics on the device; nothing but the statistics records leaves it.
    std::vector<FrontierCluster> ExtractFrontierClusters(const VoxelGrid::GRID_INDEX& lower_index, const int64_t nx, const int64_t ny, const int64_t nz,
                                                         const int64_t min_cells = 1, const bool use_26 = true) const {
        RequireInitialized();
        if (!WindowCountsOk(nx, ny, nz)) throw std::invalid_argument("ExtractFrontierClusters: cell counts must be positive and span at most 2^32 - 1 cells");
        const int64_t lower[3] = {lower_index.x, lower_index.y, lower_index.z};
        const size_t n = (size_t)(nx * ny * nz);
        std::vector<sdfgpu_component_stats> stats;
        int rc = SDFGPU_OK;
        std::string message;
        {
            const std::lock_guard<std::mutex> lock(collision_field_->ctx->mutex);
            sdfgpu_handle h = collision_field_->ctx->handle;
            void *d_bits = nullptr, *d_labels = nullptr, *d_stats = nullptr;
            uint32_t label_count = 0;
            int64_t total = 0;
            rc = sdfgpu_device_malloc(h, (n + 31) / 32 * 4, &d_bits);
            if (rc == SDFGPU_OK) rc = sdfgpu_device_malloc(h, n * 4, &d_labels);
            if (rc == SDFGPU_OK) rc = sdfgpu_dsh_frontier_window_device(collision_field_->map, lower, nx, ny, nz, FrontierFlags(use_26), static_cast<uint32_t*>(d_bits), nullptr);
            if (rc == SDFGPU_OK) rc = sdfgpu_components_bits_device(h, static_cast<const uint32_t*>(d_bits), nx, ny, nz, static_cast<uint32_t*>(d_labels), &label_count, nullptr);
            // (the number of records first: the labels of the window's other cells take none)
            if (rc == SDFGPU_OK) rc = sdfgpu_component_stats_device(h, static_cast<const uint32_t*>(d_bits), static_cast<const uint32_t*>(d_labels), nx, ny, nz,
                                                                    label_count, nullptr, 0, &total, nullptr);
            if (rc == SDFGPU_OK && total > 0) {
                stats.resize((size_t)total);
                rc = sdfgpu_device_malloc(h, stats.size() * sizeof(sdfgpu_component_stats), &d_stats);
                if (rc == SDFGPU_OK) rc = sdfgpu_component_stats_device(h, static_cast<const uint32_t*>(d_bits), static_cast<const uint32_t*>(d_labels), nx, ny, nz,
                                                                        label_count, static_cast<sdfgpu_component_stats*>(d_stats), total, &total, nullptr);
                if (rc == SDFGPU_OK) rc = sdfgpu_copy_to_host(h, stats.data(), d_stats, stats.size() * sizeof(sdfgpu_component_stats), nullptr);
            }
            if (rc != SDFGPU_OK) message = sdfgpu_last_error(h);
            (void)sdfgpu_device_free(h, d_bits);
            (void)sdfgpu_device_free(h, d_labels);
            (void)sdfgpu_device_free(h, d_stats);
        }
        if (rc == SDFGPU_ERR_INVALID_ARGUMENT) throw std::invalid_argument("sdfgpu: " + message);
        if (rc != SDFGPU_OK) throw std::runtime_error("sdfgpu: " + message);
        std::vector<FrontierCluster> clusters;
        for (const sdfgpu_component_stats& s : stats) {
            if (s.count < min_cells) continue;
            FrontierCluster cluster;
            cluster.label = s.label;
            cluster.cells = s.count;
            cluster.lower = VoxelGrid::GRID_INDEX(lower[0] + s.lo[0], lower[1] + s.lo[1], lower[2] + s.lo[2]);
            cluster.upper = VoxelGrid::GRID_INDEX(lower[0] + s.hi[0], lower[1] + s.hi[1], lower[2] + s.hi[2]);
            double g[3];
            for (int a = 0; a < 3; ++a) g[a] = ((double)lower[a] + ((double)s.sum[a] / (double)s.count + 0.5)) * resolution_;
            cluster.centroid = origin_transform_ * Eigen::Vector3d(g[0], g[1], g[2]);
            clusters.push_back(cluster);
        }
        return clusters;
    }

    // ---- display (reference dynamic_spatial_hashed_collision_map.cpp:85-199) ---------------------------------------------------------------
    // 0, 1 or 2 markers: the chunk-filled chunks as cubes of the chunk's size at their centres, then the cells of the cell-filled
    // chunks as cubes of the cell's size; a marker without a point is left out.  Chunks in ascending (c_x, c_y, c_z) order (the
    // reference's is its hash map's), cells x -> y -> z inside a chunk.
    std::vector<visualization_msgs::Marker> ExportForDisplay(const std_msgs::ColorRGBA& collision_color, const std_msgs::ColorRGBA& free_color,
                                                             const std_msgs::ColorRGBA& unknown_color) const {
        std::vector<visualization_msgs::Marker> display_markers;
        if (!initialized_) return display_markers;
        std::vector<sdfgpu_dsh_chunk> chunks;
        std::vector<COLLISION_CELL> cells;
        Export(chunks, cells);
        visualization_msgs::Marker chunks_display_rep =
            display::MakeMarker(frame_, "dynamic_spatial_hashed_collision_map_chunks_display", Eigen::Isometry3d::Identity(), 1.0);
        const std::vector<double> chunk_sizes = GetChunkSizes();
        chunks_display_rep.scale.x = chunk_sizes[0]; chunks_display_rep.scale.y = chunk_sizes[1]; chunks_display_rep.scale.z = chunk_sizes[2];
        visualization_msgs::Marker cells_display_rep =
            display::MakeMarker(frame_, "dynamic_spatial_hashed_collision_map_cells_display", Eigen::Isometry3d::Identity(), resolution_);
        const auto color_of = [&](const float occupancy) -> const std_msgs::ColorRGBA& {
            return occupancy > 0.5 ? collision_color : occupancy < 0.5 ? free_color : unknown_color;
        };
        const auto point_of = [&](const double gx, const double gy, const double gz) {
            const Eigen::Vector3d location = origin_transform_ * Eigen::Vector3d(gx, gy, gz);
            geometry_msgs::Point p;
            p.x = location.x(); p.y = location.y(); p.z = location.z();
            return p;
        };
        for (const sdfgpu_dsh_chunk& chunk : chunks) {
            const double base[3] = {(double)(chunk.c[0] * chunk_sizes_[0]), (double)(chunk.c[1] * chunk_sizes_[1]), (double)(chunk.c[2] * chunk_sizes_[2])};
            if (chunk.state == SDFGPU_DSH_FOUND_IN_CHUNK) {
                COLLISION_CELL cell;
                std::memcpy(static_cast<void*>(&cell), &chunk.record, sizeof cell);
                chunks_display_rep.points.push_back(point_of((base[0] + 0.5 * (double)chunk_sizes_[0]) * resolution_, (base[1] + 0.5 * (double)chunk_sizes_[1]) * resolution_,
                                                             (base[2] + 0.5 * (double)chunk_sizes_[2]) * resolution_));
                chunks_display_rep.colors.push_back(color_of(cell.occupancy));
                continue;
            }
            const COLLISION_CELL* cell = cells.data() + chunk.first_cell;
            for (int64_t x = 0; x < chunk_sizes_[0]; ++x)
                for (int64_t y = 0; y < chunk_sizes_[1]; ++y)
                    for (int64_t z = 0; z < chunk_sizes_[2]; ++z, ++cell) {
                        cells_display_rep.points.push_back(point_of((base[0] + (double)x + 0.5) * resolution_, (base[1] + (double)y + 0.5) * resolution_,
                                                                    (base[2] + (double)z + 0.5) * resolution_));
                        cells_display_rep.colors.push_back(color_of(cell->occupancy));
                    }
        }
        if (chunks_display_rep.points.size() > 0) display_markers.push_back(chunks_display_rep);
        if (cells_display_rep.points.size() > 0) display_markers.push_back(cells_display_rep);
        return display_markers;
    }

    // the live chunks in ascending (c_x, c_y, c_z) order and the cell-filled chunks' cells (sdfgpu_dsh_export)
    void Export(std::vector<sdfgpu_dsh_chunk>& chunks, std::vector<COLLISION_CELL>& cells) const {
        RequireInitialized();
        int64_t n_chunks = 0, n_cells = 0;
        Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_export(m, nullptr, 0, nullptr, 0, &n_chunks, &n_cells); });
        chunks.assign((size_t)n_chunks, sdfgpu_dsh_chunk());
        cells.assign((size_t)n_cells, COLLISION_CELL());
        if (n_chunks) Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_export(m, chunks.data(), n_chunks, cells.data(), n_cells, &n_chunks, &n_cells); });
    }
    sdfgpu_dsh_counts GetCounts() const {
        RequireInitialized();
        sdfgpu_dsh_counts counts;
        Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_info(m, &counts); });
        return counts;
    }

private:
    struct Components { uint32_t count, flags; bool valid; };
    // what the map says about its components (host-only: no GPU call)
    Components ComponentsInfo() const {
        Components now = {0u, 0u, false};
        if (!initialized_ || !collision_field_ || !collision_field_->map) return now;
        int valid = 0;
        const std::lock_guard<std::mutex> lock(collision_field_->ctx->mutex);
        if (sdfgpu_dsh_components_info(collision_field_->map, &now.count, &now.flags, &valid) != SDFGPU_OK) return Components{0u, 0u, false};
        now.valid = valid != 0;
        return now;
    }
    static uint32_t FrontierFlags(const bool use_26) { return use_26 ? (uint32_t)SDFGPU_DSH_FRONTIER_26 : 0u; }
    // positive cell counts whose product is at most 2^32 - 1 (what the window calls take)
    static bool WindowCountsOk(const int64_t nx, const int64_t ny, const int64_t nz) {
        const int64_t most = 4294967295ll;
        return nx > 0 && ny > 0 && nz > 0 && nx <= most && ny <= most / nx && nz <= most / (nx * ny);
    }
    std::vector<VoxelGrid::GRID_INDEX> FrontierCells(const int64_t* lower, const int64_t* extent, const bool use_26) const {
        RequireInitialized();
        int64_t total = 0;
        Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_frontier_cells(m, lower, extent, FrontierFlags(use_26), nullptr, 0, &total); });
        std::vector<int64_t> raw((size_t)total * 3);
        if (total) Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_frontier_cells(m, lower, extent, FrontierFlags(use_26), raw.data(), total, &total); });
        std::vector<VoxelGrid::GRID_INDEX> cells((size_t)total);
        for (size_t i = 0; i < cells.size(); ++i) cells[i] = VoxelGrid::GRID_INDEX(raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]);
        return cells;
    }
    static uint32_t CastFlags(const bool unknown_is_filled, const bool skip_first, const bool skip_last) {
        return (unknown_is_filled ? (uint32_t)SDFGPU_DSH_CAST_UNKNOWN_IS_FILLED : 0u) | (skip_first ? (uint32_t)SDFGPU_DSH_CAST_SKIP_FIRST : 0u) |
               (skip_last ? (uint32_t)SDFGPU_DSH_CAST_SKIP_LAST : 0u);
    }
    static RayCast MakeRayCast(const uint8_t status, const sdfgpu_dsh_cast_hit& hit, const double* start, const double* end) {
        RayCast cast;
        cast.status = (CAST_STATUS)status;
        cast.cell = VoxelGrid::GRID_INDEX(hit.cell[0], hit.cell[1], hit.cell[2]);
        std::memcpy(static_cast<void*>(&cast.value), &hit.record, sizeof cast.value);
        cast.found = (VoxelGrid::FOUND_STATUS)hit.found;
        cast.t = hit.t;
        cast.step = hit.step;
        const double dx = end[0] - start[0], dy = end[1] - start[1], dz = end[2] - start[2];
        cast.distance = status == SDFGPU_DSH_CAST_SKIPPED ? 0.0 : hit.t * std::sqrt((dx * dx + dy * dy) + dz * dz);
        return cast;
    }
    int64_t BoxRemoval(const VoxelGrid::GRID_INDEX& lower_index, const int64_t nx, const int64_t ny, const int64_t nz, const int invert) {
        RequireInitialized();
        const int64_t lower[3] = {lower_index.x, lower_index.y, lower_index.z}, extent[3] = {nx, ny, nz};
        int64_t removed = 0;
        Locked([&](sdfgpu_dsh_map m) { return sdfgpu_dsh_retain_box(m, lower, extent, invert, &removed, nullptr); });
        if (removed) components_valid_ = false;
        return removed;
    }
    Eigen::Isometry3d WindowOrigin(const VoxelGrid::GRID_INDEX& lower_index) const {
        Eigen::Isometry3d corner;
        corner.setTranslation((double)lower_index.x * resolution_, (double)lower_index.y * resolution_, (double)lower_index.z * resolution_);
        return origin_transform_ * corner;
    }
    std::vector<VoxelGrid::SET_STATUS> SetBatch(const bool chunk_sets, const std::vector<double>& locations_xyz, const std::vector<COLLISION_CELL>& values) {
        RequireInitialized();
        if (locations_xyz.size() % 3) throw std::invalid_argument("SetCells / SetChunks: locations are x, y, z triples");
        const size_t n = locations_xyz.size() / 3;
        const bool one = values.size() == 1;
        if (!one && values.size() != n) throw std::invalid_argument("SetCells / SetChunks: one value, or one per location");
        std::vector<uint8_t> raw(n);
        if (n) Locked([&](sdfgpu_dsh_map m) {
            return (chunk_sets ? sdfgpu_dsh_set_chunks : sdfgpu_dsh_set_cells)(m, locations_xyz.data(), (int64_t)n, one ? nullptr : values.data(),
                                                                               one ? values.data() : nullptr, raw.data());
        });
        std::vector<VoxelGrid::SET_STATUS> statuses(n);
        for (size_t i = 0; i < n; ++i) {
            statuses[i] = (VoxelGrid::SET_STATUS)raw[i];
            if (raw[i] != VoxelGrid::NOT_SET) components_valid_ = false;
        }
        return statuses;
    }
};

}  // namespace sdf_tools
