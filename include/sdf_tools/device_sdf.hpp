// DeviceSignedDistanceField -- a signed distance field that STAYS IN HBM (round 4, next-row N1 for C++ callers).
//
// The reference's C++ callers build a field and then ask it for distances and gradients at THEIR points, one host call per
// point: SignedDistanceField::EstimateDistance / EstimateDistance3d / 4d (include/sdf_tools/sdf.hpp:922-961) and
// GetGradient / 3d / 4d (:383-430).  Behind the drop-in seam that costs a 512^3 caller the 512 MiB download of
// sdfgpu_build (~10 ms of PCIe against 0.14 - 1.5 ms of kernels) before the first query.  This class is the other
// shape of the same API: ExtractSignedDistanceFieldDevice (sdf_generation.hpp / CollisionMapGrid) leaves the field on the
// MI355X, EstimateDistanceBatch / GetGradientBatch answer n points with ONE kernel (sdfgpu_query_points: one lane per
// point, the reference's double arithmetic), ProjectBatch walks n points out of collision in one kernel (sdfgpu_project_points),
// QueryGradientsBatch answers GetAutoDiffGradient / GetSmoothGradient / DistanceToBoundary for n points in one kernel
// (sdfgpu_query_gradients), and Host() downloads the field lazily, once, for callers that do want the
// reference's container (GetValue*, serialisation, per-point calls).
//
// Ownership (round 5): the device memory belongs to the libsdfgpu context of the thread that built the field,
// and the field SHARES ownership of that context (sdf_generation::SharedGpuContext): it may be returned from a worker
// thread, queried or destroyed on another thread, or outlive the thread that built it -- the context is destroyed with its
// last owner, and every call on it (builds on the owning thread included) is made under the context's mutex.
#pragma once
#include <cstdint>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sdf_tools/gpu_context.hpp"
#include "sdf_tools/sdf.hpp"
#include "sdfgpu.h"

namespace sdf_tools {

class DeviceSignedDistanceField {
public:
    DeviceSignedDistanceField() = default;
    // An empty field of the given geometry in HBM (contents undefined until a build writes them).
    DeviceSignedDistanceField(const Eigen::Isometry3d& origin_transform, const std::string& frame, const double resolution,
                              const int64_t x_cells, const int64_t y_cells, const int64_t z_cells, const float oob_value)
        : origin_(origin_transform), inverse_origin_(origin_transform.inverse()), frame_(frame), resolution_(resolution),
          nx_(x_cells), ny_(y_cells), nz_(z_cells), oob_(oob_value) {
        if (nx_ <= 0 || ny_ <= 0 || nz_ <= 0) throw std::invalid_argument("DeviceSignedDistanceField: cell counts must be positive");
        ctx_ = sdf_generation::GpuContext::Shared();
        handle_ = ctx_->handle;
        void* p = nullptr;
        const std::lock_guard<std::mutex> lock(ctx_->mutex);
        sdf_generation::ThrowOnStatus(handle_, sdfgpu_device_malloc(handle_, (size_t)(nx_ * ny_ * nz_) * sizeof(float), &p));
        d_sdf_ = static_cast<float*>(p);
    }
    ~DeviceSignedDistanceField() { Release(); }
    DeviceSignedDistanceField(const DeviceSignedDistanceField&) = delete;
    DeviceSignedDistanceField& operator=(const DeviceSignedDistanceField&) = delete;
    DeviceSignedDistanceField(DeviceSignedDistanceField&& o) noexcept { MoveFrom(o); }
    DeviceSignedDistanceField& operator=(DeviceSignedDistanceField&& o) noexcept {
        if (this != &o) { Release(); MoveFrom(o); }
        return *this;
    }

    // A host field -> HBM (one upload; for fields loaded from a file or a message).
    static DeviceSignedDistanceField Upload(const SignedDistanceField& sdf) {
        DeviceSignedDistanceField d(sdf.GetOriginTransform(), sdf.GetFrame(), sdf.GetResolution(), sdf.GetNumXCells(),
                                    sdf.GetNumYCells(), sdf.GetNumZCells(), sdf.GetOOBValue());
        const std::lock_guard<std::mutex> lock(d.ctx_->mutex);
        sdf_generation::ThrowOnStatus(d.handle_, sdfgpu_copy_from_host(d.handle_, d.d_sdf_, sdf.GetImmutableRawData().data(),
                                                                       (size_t)d.NumCells() * sizeof(float), nullptr));
        return d;
    }

    bool IsInitialized() const { return d_sdf_ != nullptr; }
    double GetResolution() const { return resolution_; }
    std::string GetFrame() const { return frame_; }
    int64_t GetNumXCells() const { return nx_; }
    int64_t GetNumYCells() const { return ny_; }
    int64_t GetNumZCells() const { return nz_; }
    int64_t NumCells() const { return nx_ * ny_ * nz_; }
    float GetOOBValue() const { return oob_; }
    const Eigen::Isometry3d& GetOriginTransform() const { return origin_; }
    // Device pointer of the [x][y][z] fp32 field (z fastest), for callers with their own kernels / the *_device ABI.
    float* DevicePointer() { host_.reset(); return d_sdf_; }
    const float* DevicePointer() const { return d_sdf_; }
    sdfgpu_handle Handle() const { return handle_; }
    // the context this field lives on (shared ownership); callers that use Handle() / DevicePointer() with the C ABI themselves
    // hold Context()->mutex around their calls
    const std::shared_ptr<sdf_generation::SharedGpuContext>& Context() const { return ctx_; }

    // (max, min) of the un-narrowed distances, as the reference returns them beside the field (sdf_generation.hpp:246-269).
    std::pair<double, double> GetExtrema() const { return extrema_; }
    void SetExtrema(const std::pair<double, double>& e) { extrema_ = e; }

    // n world-frame points (n x 3 doubles, x y z) -> what n calls of EstimateDistance3d (sdf.hpp:947-953) and
    // GetGradient3d (:395-403) return, from one kernel:
    //   out_distance[n]    the trilinear estimate, OOB value outside the grid
    //   out_gradient[3 n]  world-frame gradient of the cell holding the point, NaN where the reference returns an empty
    //                      vector (outside the grid; boundary shell unless enable_edge_gradients)
    //   out_flags[n]       bit 0 = inside the grid (EstimateDistance's .second), bit 1 = gradient available
    // Any output may be null.
    void QueryBatch(const double* points_xyz, const int64_t n, const bool enable_edge_gradients, double* out_distance,
                    double* out_gradient, uint8_t* out_flags) const {
        if (!d_sdf_) throw std::runtime_error("DeviceSignedDistanceField is not initialized");
        double w2g[12], rot[9];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 4; ++c) w2g[r * 4 + c] = inverse_origin_.matrix()(r, c);
            for (int c = 0; c < 3; ++c) rot[r * 3 + c] = origin_.matrix()(r, c);
        }
        const std::lock_guard<std::mutex> lock(ctx_->mutex);
        sdf_generation::ThrowOnStatus(handle_, sdfgpu_query_points(handle_, d_sdf_, nx_, ny_, nz_, resolution_, w2g, rot, oob_,
                                                                   points_xyz, n, enable_edge_gradients ? 1 : 0, out_distance,
                                                                   out_gradient, out_flags));
    }
    // Reference-shaped results: one std::pair<double, bool> per location, like EstimateDistance3d.
    std::vector<std::pair<double, bool>> EstimateDistanceBatch(const std::vector<Eigen::Vector3d>& locations) const {
        const std::vector<double> pts = Flatten(locations);
        std::vector<double> dist(locations.size());
        std::vector<uint8_t> flags(locations.size());
        QueryBatch(pts.data(), (int64_t)locations.size(), false, dist.data(), nullptr, flags.data());
        std::vector<std::pair<double, bool>> out(locations.size());
        for (size_t i = 0; i < out.size(); ++i) out[i] = std::make_pair(dist[i], (flags[i] & 1u) != 0);
        return out;
    }
    // ... and one std::vector<double> per location like GetGradient3d: 3 components, or empty.
    std::vector<std::vector<double>> GetGradientBatch(const std::vector<Eigen::Vector3d>& locations,
                                                      const bool enable_edge_gradients = false) const {
        const std::vector<double> pts = Flatten(locations);
        std::vector<double> grad(locations.size() * 3);
        std::vector<uint8_t> flags(locations.size());
        QueryBatch(pts.data(), (int64_t)locations.size(), enable_edge_gradients, nullptr, grad.data(), flags.data());
        std::vector<std::vector<double>> out(locations.size());
        for (size_t i = 0; i < out.size(); ++i)
            if (flags[i] & 2u) out[i] = std::vector<double>{grad[3 * i], grad[3 * i + 1], grad[3 * i + 2]};
        return out;
    }

    // n world-frame points (n x 3 doubles) -> what n calls of SignedDistanceField::ProjectCounted4d return (the counted form of
    // ProjectOutOfCollisionToMinimumDistance3d, or of ProjectIntoValidVolumeToMinimumDistance3d with into_valid_volume_only), from
    // one kernel (sdfgpu_project_points, include/sdfgpu.h "Projection"):
    //   out_points[3 n]  world-frame results (a failed walk keeps the last location it reached; a refused point its input)
    //   out_status[n]    SDFGPU_PROJECT_*
    //   out_steps[n]     steps taken
    // out_status and out_steps may be null.  max_steps = 0: the library default (sdfgpu_project_step_limit).
    void ProjectBatch(const double* points_xyz, const int64_t n, const double minimum_distance, const double stepsize_multiplier,
                      const bool into_valid_volume_only, const int max_steps, double* out_points, uint8_t* out_status,
                      int32_t* out_steps) const {
        if (!d_sdf_) throw std::runtime_error("DeviceSignedDistanceField is not initialized");
        double w2g[12], g2w[12];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) { w2g[r * 4 + c] = inverse_origin_.matrix()(r, c); g2w[r * 4 + c] = origin_.matrix()(r, c); }
        const std::lock_guard<std::mutex> lock(ctx_->mutex);
        sdf_generation::ThrowOnStatus(handle_, sdfgpu_project_points(handle_, d_sdf_, nx_, ny_, nz_, resolution_, w2g, g2w, minimum_distance,
                                                                     stepsize_multiplier, max_steps,
                                                                     into_valid_volume_only ? SDFGPU_PROJECT_INTO_VALID_VOLUME
                                                                                            : SDFGPU_PROJECT_OUT_OF_COLLISION,
                                                                     points_xyz, n, out_points, out_status, out_steps));
    }
    // Reference-shaped: one location per input like ProjectOutOfCollisionToMinimumDistance3d, plus the statuses (a location
    // is the reference's answer only where its status is SDFGPU_PROJECT_CONVERGED; elsewhere the reference throws).
    std::vector<Eigen::Vector3d> ProjectOutOfCollisionToMinimumDistanceBatch(const std::vector<Eigen::Vector3d>& locations,
                                                                             const double minimum_distance,
                                                                             std::vector<uint8_t>* statuses = nullptr,
                                                                             const double stepsize_multiplier = 1.0 / 8.0) const {
        const std::vector<double> pts = Flatten(locations);
        std::vector<double> out(pts.size());
        std::vector<uint8_t> st(locations.size());
        ProjectBatch(pts.data(), (int64_t)locations.size(), minimum_distance, stepsize_multiplier, false, 0, out.data(), st.data(), nullptr);
        std::vector<Eigen::Vector3d> r(locations.size());
        for (size_t i = 0; i < r.size(); ++i) r[i] = Eigen::Vector3d(out[3 * i], out[3 * i + 1], out[3 * i + 2]);
        if (statuses) *statuses = std::move(st);
        return r;
    }
    std::vector<Eigen::Vector3d> ProjectOutOfCollisionBatch(const std::vector<Eigen::Vector3d>& locations,
                                                            std::vector<uint8_t>* statuses = nullptr,
                                                            const double stepsize_multiplier = 1.0 / 8.0) const {
        return ProjectOutOfCollisionToMinimumDistanceBatch(locations, 0.0, statuses, stepsize_multiplier);
    }

    // n world-frame points (n x 3 doubles) -> what n calls of SignedDistanceField::QueryGradient4d return for `kind`
    // (SDFGPU_QUERY_SMOOTH_GRADIENT with `window`, SDFGPU_QUERY_AUTODIFF_GRADIENT, SDFGPU_QUERY_DISTANCE_TO_BOUNDARY), from one
    // kernel (sdfgpu_query_gradients, include/sdfgpu.h "Interpolated gradients"):
    //   out_value[n]       the estimate (OOB value outside), or the signed displacement to the nearest face
    //   out_gradient[3 n]  world frame; NaN where GetSmoothGradient / GetAutoDiffGradient return an empty vector or throw
    //   out_status[n]      SDFGPU_QUERY_*
    // Any output may be null.
    void QueryGradientsBatch(const double* points_xyz, const int64_t n, const int kind, const double window, double* out_value,
                             double* out_gradient, uint8_t* out_status) const {
        if (!d_sdf_) throw std::runtime_error("DeviceSignedDistanceField is not initialized");
        double w2g[12];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) w2g[r * 4 + c] = inverse_origin_.matrix()(r, c);
        const std::lock_guard<std::mutex> lock(ctx_->mutex);
        sdf_generation::ThrowOnStatus(handle_, sdfgpu_query_gradients(handle_, d_sdf_, nx_, ny_, nz_, resolution_, w2g, oob_, kind, window,
                                                                      points_xyz, n, out_value, out_gradient, out_status));
    }
    // Reference-shaped: one std::vector<double> per location like GetAutoDiffGradient3d (3 components, or empty outside the grid
    // or for a non-finite location); the estimates (EstimateDistance3d's .first) in *values when asked.
    std::vector<std::vector<double>> GetAutoDiffGradientBatch(const std::vector<Eigen::Vector3d>& locations,
                                                              std::vector<double>* values = nullptr,
                                                              std::vector<uint8_t>* statuses = nullptr) const {
        return GradientBatch(locations, SDFGPU_QUERY_AUTODIFF_GRADIENT, 0.0, values, statuses);
    }
    // ... like GetSmoothGradient3d (empty where the reference returns empty or throws; *statuses tells which)
    std::vector<std::vector<double>> GetSmoothGradientBatch(const std::vector<Eigen::Vector3d>& locations, const double nominal_window_size,
                                                            std::vector<uint8_t>* statuses = nullptr) const {
        return GradientBatch(locations, SDFGPU_QUERY_SMOOTH_GRADIENT, nominal_window_size, nullptr, statuses);
    }
    // ... like DistanceToBoundary3d
    std::vector<std::pair<double, bool>> DistanceToBoundaryBatch(const std::vector<Eigen::Vector3d>& locations) const {
        const std::vector<double> pts = Flatten(locations);
        std::vector<double> value(locations.size());
        std::vector<uint8_t> st(locations.size());
        QueryGradientsBatch(pts.data(), (int64_t)locations.size(), SDFGPU_QUERY_DISTANCE_TO_BOUNDARY, 0.0, value.data(), nullptr, st.data());
        std::vector<std::pair<double, bool>> out(locations.size());
        for (size_t i = 0; i < out.size(); ++i) out[i] = std::make_pair(value[i], st[i] == SDFGPU_QUERY_OK);
        return out;
    }

    // The reference's container, downloaded on first use (and again after DevicePointer() handed out write access).
    const SignedDistanceField& Host() const {
        if (!host_) {
            if (!d_sdf_) throw std::runtime_error("DeviceSignedDistanceField is not initialized");
            std::unique_ptr<SignedDistanceField> h(new SignedDistanceField(SignedDistanceField::ForBuild{}, origin_, frame_, resolution_, nx_, ny_, nz_, oob_));
            const std::lock_guard<std::mutex> lock(ctx_->mutex);
            sdf_generation::ThrowOnStatus(handle_, sdfgpu_copy_to_host(handle_, h->MutableDataForBuild(), d_sdf_,
                                                                       (size_t)NumCells() * sizeof(float), nullptr));
            host_ = std::move(h);
        }
        return *host_;
    }
    bool HostCopyExists() const { return (bool)host_; }

private:
    std::vector<std::vector<double>> GradientBatch(const std::vector<Eigen::Vector3d>& locations, const int kind, const double window,
                                                   std::vector<double>* values, std::vector<uint8_t>* statuses) const {
        const std::vector<double> pts = Flatten(locations);
        std::vector<double> value(locations.size()), grad(locations.size() * 3);
        std::vector<uint8_t> st(locations.size());
        QueryGradientsBatch(pts.data(), (int64_t)locations.size(), kind, window, value.data(), grad.data(), st.data());
        std::vector<std::vector<double>> out(locations.size());
        for (size_t i = 0; i < out.size(); ++i)
            if (st[i] == SDFGPU_QUERY_OK) out[i] = std::vector<double>{grad[3 * i], grad[3 * i + 1], grad[3 * i + 2]};
        if (values) *values = std::move(value);
        if (statuses) *statuses = std::move(st);
        return out;
    }
    static std::vector<double> Flatten(const std::vector<Eigen::Vector3d>& locations) {
        std::vector<double> pts(locations.size() * 3);
        for (size_t i = 0; i < locations.size(); ++i) { pts[3 * i] = locations[i].x(); pts[3 * i + 1] = locations[i].y(); pts[3 * i + 2] = locations[i].z(); }
        return pts;
    }
    void Release() {
        if (d_sdf_ && ctx_) {
            const std::lock_guard<std::mutex> lock(ctx_->mutex);
            (void)sdfgpu_device_free(handle_, d_sdf_);
        }
        d_sdf_ = nullptr;
        host_.reset();
        ctx_.reset();                                             // (may destroy the context: this field was its last owner)
        handle_ = nullptr;
    }
    void MoveFrom(DeviceSignedDistanceField& o) {
        origin_ = o.origin_; inverse_origin_ = o.inverse_origin_; frame_ = std::move(o.frame_); resolution_ = o.resolution_;
        nx_ = o.nx_; ny_ = o.ny_; nz_ = o.nz_; oob_ = o.oob_; ctx_ = std::move(o.ctx_); handle_ = o.handle_; d_sdf_ = o.d_sdf_; extrema_ = o.extrema_;
        host_ = std::move(o.host_);
        o.d_sdf_ = nullptr;
        o.handle_ = nullptr;
    }

    Eigen::Isometry3d origin_, inverse_origin_;
    std::string frame_;
    double resolution_ = 1.0;
    int64_t nx_ = 0, ny_ = 0, nz_ = 0;
    float oob_ = 0.0f;
    std::shared_ptr<sdf_generation::SharedGpuContext> ctx_;       // keeps the context (and so d_sdf_) alive
    sdfgpu_handle handle_ = nullptr;
    float* d_sdf_ = nullptr;
    std::pair<double, double> extrema_{0.0, 0.0};
    mutable std::unique_ptr<SignedDistanceField> host_;
};

}  // namespace sdf_tools
