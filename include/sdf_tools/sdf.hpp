// SignedDistanceField -- result container of the SDF build path, API-compatible with the subset
// of sdf_tools::SignedDistanceField (reference include/sdf_tools/sdf.hpp) that the hot path and the
// pysdf_tools surface use: constructors (:34-81), lock-guarded SetValue (:236-264), GetGradient /
// GetGridAlignedGradient / GetFullGradient (:341-526), EstimateDistance (:699-961), serialisation
// and file / message forms (src/sdf_tools/sdf.cpp:213-502), the local extrema map (sdf.cpp:23-207, on the GPU) and projection
// out of collision / into the valid volume (:996-1190; batched on the GPU through DeviceSignedDistanceField::ProjectBatch), and
// the smooth and autodiff gradients and DistanceToBoundary (:528-653, :963-988; batched on the GPU through
// DeviceSignedDistanceField::QueryGradientsBatch).  ExportForDisplay / ExportForDisplayCollisionOnly (sdf.cpp:504-640) take their selection and
// colour map from the GPU (include/sdfgpu.h "Display export", include/sdf_tools/display.hpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "arc_utilities/serialization.hpp"
#include "arc_utilities/voxel_grid.hpp"
#include "arc_utilities/zlib_helpers.hpp"
#include "sdf_tools/autodiff.hpp"
#include "sdf_tools/display.hpp"
#include "sdf_tools/eigen_lite.hpp"
#include "sdf_tools/gpu_context.hpp"

namespace sdf_tools {
using VoxelGrid::GRID_INDEX;

// Plain mirror of msg/SDF.msg for builds without ROS (field names kept).
struct SDF {
    struct Header { uint32_t seq = 0; double stamp = 0.0; std::string frame_id; } header;
    std::vector<uint8_t> serialized_sdf;
    bool is_compressed = false;
};

namespace detail {
// A std::vector<float> of n elements whose storage nobody has written: the pages of a 512^3 field (512 MiB) are then first
// touched by the thread team that drains the device-to-host copy into it -- in parallel, once -- instead of by one thread
// value-initialising 134 M floats that the drain overwrites (measured in round 4: the largest part of a 241 ms class call
// around 0.14 ms of kernels).  The container type must stay std::vector<float> (GetImmutableRawData() returns it by
// reference, reference include/sdf_tools/sdf.hpp / VoxelGrid), and the standard offers no way to size one without writing
// its elements, so on libstdc++ the three pointers of an empty vector are pointed at memory from its own allocator
// (begin, end, end of storage -- a layout that has not changed since GCC 3; checked against a normally built vector at run
// time); anywhere else, or if the check fails, the vector is built the ordinary way and only speed is lost.
inline std::vector<float> UninitializedFloatVector(const size_t n) {
    // OPT-IN (round 6): the trick overwrites a std::vector's representation -- undefined behaviour by the letter of the standard, and
    // invisible to an instrumented vector -- so it is compiled only when the client defines SDF_TOOLS_VECTOR_ADOPT (the in-tree
    // builds of pysdf_tools and the examples do; INTEGRATION.md's drop-in recipe does not), never in debug / sanitizer builds of
    // libstdc++.  Without it the storage is value-initialised the ordinary way: +75 ... 100 ms per 512^3 result (measured: profiles/r06_redzone_suite_and_fuzz.txt).
#if defined(SDF_TOOLS_VECTOR_ADOPT) && defined(__GLIBCXX__) && !defined(_GLIBCXX_DEBUG) && !defined(_GLIBCXX_SANITIZE_VECTOR) && \
    !defined(__SANITIZE_ADDRESS__) && !defined(__SANITIZE_THREAD__) && !defined(SDF_TOOLS_NO_VECTOR_ADOPT)
    static_assert(sizeof(std::vector<float>) == 3 * sizeof(float*), "std::vector<float> is not three pointers");
    static const bool layout_ok = []() {
        std::vector<float> probe(3);
        probe.reserve(5);
        float* rep[3];
        std::memcpy(rep, static_cast<const void*>(&probe), sizeof rep);
        return rep[0] == probe.data() && rep[1] == probe.data() + probe.size() && rep[2] == probe.data() + probe.capacity();
    }();
    if (layout_ok && n > 0) {
        std::vector<float> v;
        float* const p = std::allocator<float>().allocate(n);      // (operator new: untouched pages for large n)
        float* rep[3] = {p, p + n, p + n};
        std::memcpy(static_cast<void*>(&v), rep, sizeof rep);      // v now owns p; its destructor deallocates through the same allocator
        return v;
    }
#endif
    return std::vector<float>(n);
}
}  // namespace detail

class SignedDistanceField : public VoxelGrid::VoxelGrid<float> {
protected:
    std::string frame_;
    bool locked_;

public:
    // Tag of the constructor the build seams use: every cell is about to be overwritten by the device-to-host drain, so the
    // array is NOT filled with OOB_value first (detail::UninitializedFloatVector).  Cells are indeterminate until then.
    struct ForBuild {};
    SignedDistanceField(ForBuild, const Eigen::Isometry3d& origin_transform, const std::string& frame, double resolution,
                        int64_t x_cells, int64_t y_cells, int64_t z_cells, float OOB_value)
        : Base(), frame_(frame), locked_(false) {
        if (x_cells <= 0 || y_cells <= 0 || z_cells <= 0) throw std::invalid_argument("cell counts must be positive");
        std::vector<float> storage = detail::UninitializedFloatVector((size_t)(x_cells * y_cells * z_cells));
        Setup(origin_transform, resolution, resolution, resolution, x_cells, y_cells, z_cells, OOB_value, OOB_value, &storage);
    }

    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    typedef std::shared_ptr<SignedDistanceField> Ptr;
    typedef std::shared_ptr<const SignedDistanceField> ConstPtr;
    using Base = ::VoxelGrid::VoxelGrid<float>;

    SignedDistanceField(const std::string& frame, double resolution, double x_size, double y_size, double z_size, float OOB_value)
        : Base(resolution, x_size, y_size, z_size, OOB_value), frame_(frame), locked_(false) {}
    SignedDistanceField(const Eigen::Isometry3d& origin_transform, const std::string& frame, double resolution,
                        double x_size, double y_size, double z_size, float OOB_value)
        : Base(origin_transform, resolution, x_size, y_size, z_size, OOB_value), frame_(frame), locked_(false) {}
    SignedDistanceField(const std::string& frame, double resolution, int64_t x_cells, int64_t y_cells, int64_t z_cells, float OOB_value)
        : Base(resolution, x_cells, y_cells, z_cells, OOB_value), frame_(frame), locked_(false) {}
    SignedDistanceField(const Eigen::Isometry3d& origin_transform, const std::string& frame, double resolution,
                        int64_t x_cells, int64_t y_cells, int64_t z_cells, float OOB_value)
        : Base(origin_transform, resolution, x_cells, y_cells, z_cells, OOB_value), frame_(frame), locked_(false) {}
    SignedDistanceField() : Base(), frame_(""), locked_(false) {}

    Base* Clone() const override { return new SignedDistanceField(*this); }

    double GetResolution() const { return GetCellSizes().x(); }
    std::string GetFrame() const { return frame_; }

    // ---- display export (reference sdf.cpp:504-640; include/sdfgpu.h "Display export") ------------------------------------------------
    // Every cell as a point, coloured by the GPU's colour map: green by d / max for d > 0, red by d / min for d < 0, blue for 0 and NaN.
    visualization_msgs::Marker ExportForDisplay(const float alpha = 0.01f) const {
        visualization_msgs::Marker m = display::MakeMarker(frame_, "sdf_display", GetOriginTransform(), GetResolution());
        const size_t n = data_.size();
        if (n == 0) return m;
        std::vector<float> rgba(n * 4);
        {
            const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
            const std::lock_guard<std::mutex> lock(ctx->mutex);
            sdf_generation::ThrowOnStatus(ctx->handle, sdfgpu_display_sdf_colors(ctx->handle, data_.data(), GetNumXCells(), GetNumYCells(),
                                                                                 GetNumZCells(), alpha, rgba.data()));
        }
        display::Cells c;
        c.nx = GetNumXCells(); c.ny = GetNumYCells(); c.nz = GetNumZCells(); c.cell_sizes = GetCellSizes();
        m.points.resize(n);
        m.colors.resize(n);
        display::ParallelFor(n, [&](const size_t lo, const size_t hi) {
            for (size_t i = lo; i < hi; ++i) {
                m.points[i] = display::PointOf(c, (uint32_t)i);
                m.colors[i] = display::MakeColor(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]);
            }
        });
        return m;
    }
    // The cells with d <= 0 as points of one colour (the marker's `color`: red with the caller's alpha); no per-point colours.
    visualization_msgs::Marker ExportForDisplayCollisionOnly(const float alpha = 0.01f) const {
        visualization_msgs::Marker m = display::MakeMarker(frame_, "sdf_display", GetOriginTransform(), GetResolution());
        m.color = display::MakeColor(1.0f, 0.0f, 0.0f, alpha);
        if (data_.empty()) return m;
        display::Selection s;
        s.indices.resize(data_.size());
        int64_t total = 0;
        {
            const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
            const std::lock_guard<std::mutex> lock(ctx->mutex);
            sdf_generation::ThrowOnStatus(ctx->handle, sdfgpu_display_select_sdf(ctx->handle, data_.data(), GetNumXCells(), GetNumYCells(), GetNumZCells(),
                                                                                 s.indices.data(), (int64_t)s.indices.size(), &total));
        }
        s.indices.resize((size_t)total);
        display::Cells c;
        c.nx = GetNumXCells(); c.ny = GetNumYCells(); c.nz = GetNumZCells(); c.cell_sizes = GetCellSizes();
        display::Append(m, c, s, 0, s.indices.size(), false, [](uint32_t, uint32_t) { return std_msgs::ColorRGBA(); });
        return m;
    }
    void SetFrame(const std::string& f) { frame_ = f; }
    bool IsLocked() const { return locked_; }
    void Lock() { locked_ = true; }
    void Unlock() { locked_ = false; }

    // Writes are refused while locked (reference sdf.hpp:236-264).
    bool SetValue(const int64_t x, const int64_t y, const int64_t z, const float& value) override {
        if (IndexInBounds(x, y, z) && !locked_) { AccessIndex(GetDataIndex(x, y, z)) = value; return true; }
        return false;
    }
    bool SetValue(const GRID_INDEX& i, const float& value) override { return SetValue(i.x, i.y, i.z, value); }
    bool SetValue4d(const Eigen::Vector4d& l, const float& value) override { return SetValue(LocationToGridIndex4d(l), value); }
    bool SetValue3d(const Eigen::Vector3d& l, const float& value) override { return SetValue(LocationToGridIndex3d(l), value); }
    bool SetValue(const double x, const double y, const double z, const float& value) override {
        return SetValue(LocationToGridIndex(x, y, z), value);
    }
    // The build path writes the whole field at once (device -> host copy lands here).
    float* MutableDataForBuild() { return locked_ ? nullptr : data_.data(); }

    // ---- gradients (reference sdf.hpp:341-526) ----------------------------------------------
    std::vector<double> GetGridAlignedGradient(const int64_t x, const int64_t y, const int64_t z,
                                               const bool enable_edge_gradients = false) const {
        if (!IndexInBounds(x, y, z)) return std::vector<double>();
        const int64_t nx = GetNumXCells(), ny = GetNumYCells(), nz = GetNumZCells();
        auto at = [&](int64_t a, int64_t b, int64_t c) -> float { return AccessIndex(GetDataIndex(a, b, c)); };
        if (x > 0 && y > 0 && z > 0 && x < nx - 1 && y < ny - 1 && z < nz - 1) {
            // central differences: float subtraction, double scale (:447-458)
            const double inv_twice_resolution = 1.0 / (2.0 * GetResolution());
            const double gx = (at(x + 1, y, z) - at(x - 1, y, z)) * inv_twice_resolution;
            const double gy = (at(x, y + 1, z) - at(x, y - 1, z)) * inv_twice_resolution;
            const double gz = (at(x, y, z + 1) - at(x, y, z - 1)) * inv_twice_resolution;
            return std::vector<double>{gx, gy, gz};
        }
        if (!enable_edge_gradients) return std::vector<double>();
        // clamped one-sided differences on the boundary shell (:464-512)
        const int64_t lx = std::max<int64_t>(0, x - 1), hx = std::min(nx - 1, x + 1);
        const int64_t ly = std::max<int64_t>(0, y - 1), hy = std::min(ny - 1, y + 1);
        const int64_t lz = std::max<int64_t>(0, z - 1), hz = std::min(nz - 1, z + 1);
        const double ix = (double)(hx - lx) * GetResolution(), iy = (double)(hy - ly) * GetResolution(),
                     iz = (double)(hz - lz) * GetResolution();
        double gx = 0.0, gy = 0.0, gz = 0.0;
        if (ix > 0.0) gx = ((double)at(hx, y, z) - (double)at(lx, y, z)) * (1.0 / ix);
        if (iy > 0.0) gy = ((double)at(x, hy, z) - (double)at(x, ly, z)) * (1.0 / iy);
        if (iz > 0.0) gz = ((double)at(x, y, hz) - (double)at(x, y, lz)) * (1.0 / iz);
        return std::vector<double>{gx, gy, gz};
    }

    // Grid-aligned gradient rotated into the world frame (:405-430).
    std::vector<double> GetGradient(const int64_t x, const int64_t y, const int64_t z, const bool enable_edge_gradients = false) const {
        const std::vector<double> g = GetGridAlignedGradient(x, y, z, enable_edge_gradients);
        if (g.size() != 3) return std::vector<double>();
        const Eigen::Quaterniond q(origin_transform_.rotation());
        const Eigen::Quaterniond r = q * (Eigen::Quaterniond(0.0, g[0], g[1], g[2]) * q.inverse());
        return std::vector<double>{r.x(), r.y(), r.z()};
    }
    std::vector<double> GetGradient(const GRID_INDEX& i, const bool e = false) const { return GetGradient(i.x, i.y, i.z, e); }
    std::vector<double> GetGradient4d(const Eigen::Vector4d& l, const bool e = false) const {
        const GRID_INDEX i = LocationToGridIndex4d(l);
        return IndexInBounds(i) ? GetGradient(i, e) : std::vector<double>();
    }
    std::vector<double> GetGradient3d(const Eigen::Vector3d& l, const bool e = false) const {
        const GRID_INDEX i = LocationToGridIndex3d(l);
        return IndexInBounds(i) ? GetGradient(i, e) : std::vector<double>();
    }
    std::vector<double> GetGradient(const double x, const double y, const double z, const bool e = false) const {
        return GetGradient4d(Eigen::Vector4d(x, y, z, 1.0), e);
    }

    // Every cell's world-frame gradient at once, [x][y][z][3] doubles, computed by ONE kernel on the MI355X
    // (sdfgpu_gradient) instead of nx*ny*nz GetGradient calls: the values are those of GetGradient(x, y, z,
    // enable_edge_gradients) bit for bit (same float-subtract / double-scale arithmetic, :447-512); cells for which
    // the reference returns an empty vector hold `empty_fill` in all three components.  A rotated origin frame
    // applies the reference's quaternion sandwich (:405-430) on the host to the grid-aligned values.
    std::vector<double> GetFullGradientFlat(const bool enable_edge_gradients, const double empty_fill) const {
        const int64_t nx = GetNumXCells(), ny = GetNumYCells(), nz = GetNumZCells();
        std::vector<double> g((size_t)(nx * ny * nz) * 3);
        if (g.empty()) return g;
        const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
        const std::lock_guard<std::mutex> lock(ctx->mutex);
        sdfgpu_handle h = ctx->handle;
        sdf_generation::ThrowOnStatus(h, sdfgpu_gradient(h, data_.data(), nx, ny, nz, GetResolution(),
                                                         enable_edge_gradients ? 1 : 0, g.data(), 1));
        const Eigen::Quaterniond q(origin_transform_.rotation());
        const bool identity = q.w() == 1.0 && q.x() == 0.0 && q.y() == 0.0 && q.z() == 0.0;
        const Eigen::Quaterniond qi = q.inverse();
        // The reference returns an EMPTY vector for a cell on the boundary shell when edge gradients are off (:464): those
        // cells get `empty_fill`.  Emptiness is decided from the index, not from the value: a genuine NaN (inf - inf on a grid
        // without filled or without free voxels) is what the reference returns there too and must stay.
        const int64_t sx = ny * nz;
        if (!identity) {
            for (size_t i = 0; i < g.size(); i += 3) {
                const Eigen::Quaterniond r = q * (Eigen::Quaterniond(0.0, g[i], g[i + 1], g[i + 2]) * qi);
                g[i] = r.x(); g[i + 1] = r.y(); g[i + 2] = r.z();
            }
        }                                                     // (identity frame: q * (0, g) * q^-1 == g exactly, nothing to do)
        if (!enable_edge_gradients) {
            // ... written over the six faces only (a loop over all cells with two divisions each cost far more than
            // the kernel -- 134 M iterations at 512^3 for 1.6 M shell cells)
            auto fill = [&](int64_t x, int64_t y, int64_t z) { double* c = &g[(size_t)(x * sx + y * nz + z) * 3]; c[0] = c[1] = c[2] = empty_fill; };
            for (int64_t x = 0; x < nx; ++x) {
                const bool xface = x == 0 || x == nx - 1;
                for (int64_t y = 0; y < ny; ++y) {
                    if (xface || y == 0 || y == ny - 1) { for (int64_t z = 0; z < nz; ++z) fill(x, y, z); }
                    else { fill(x, y, 0); fill(x, y, nz - 1); }
                }
            }
        }
        return g;
    }

    using GradientFunction = std::function<std::vector<double>(int64_t, int64_t, int64_t, bool)>;
    // Every cell's gradient via a caller-supplied function (:341-358); default cell = 3 x OOB value.
    ::VoxelGrid::VoxelGrid<std::vector<double>> GetFullGradient(const GradientFunction& gradient_function,
                                                              const bool enable_edge_gradients = false) const {
        ::VoxelGrid::VoxelGrid<std::vector<double>> grid(origin_transform_, GetResolution(), GetNumXCells(), GetNumYCells(),
                                                       GetNumZCells(), std::vector<double>(3, oob_value_));
        for (int64_t x = 0; x < GetNumXCells(); ++x)
            for (int64_t y = 0; y < GetNumYCells(); ++y)
                for (int64_t z = 0; z < GetNumZCells(); ++z)
                    grid.SetValue(x, y, z, gradient_function(x, y, z, enable_edge_gradients));
        return grid;
    }

    // ---- local extrema map (reference src/sdf_tools/sdf.cpp:23-207, sdf.hpp:1202-1218) ----------------------------
    // For every cell, the extremum its gradient walk reaches (include/sdfgpu.h "Local extrema and convex segments", DESIGN.md
    // section 15), computed on the GPU: the index of the fixed point, or of the cycle node the scan enters first, or 0xFFFFFFFF
    // where the walk leaves the grid.  4 B per cell, for callers that do not need the reference's 24.
    std::vector<uint32_t> ComputeLocalExtremaIndices() const {
        const int64_t nx = GetNumXCells(), ny = GetNumYCells(), nz = GetNumZCells();
        std::vector<uint32_t> idx((size_t)(nx * ny * nz));
        if (idx.empty()) return idx;
        const Eigen::Quaterniond q(origin_transform_.rotation());
        const Eigen::Quaterniond qi = q.inverse();
        const double q_and_qinv[8] = {q.w(), q.x(), q.y(), q.z(), qi.w(), qi.x(), qi.y(), qi.z()};
        const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
        const std::lock_guard<std::mutex> lock(ctx->mutex);
        sdf_generation::ThrowOnStatus(ctx->handle, sdfgpu_local_extrema(ctx->handle, data_.data(), nx, ny, nz, GetResolution(), q_and_qinv,
                                                                        idx.data()));
        return idx;
    }

    // The reference's map: grid-frame cell centre of each cell's extremum, (+inf, +inf, +inf) where the walk leaves the grid.
    ::VoxelGrid::VoxelGrid<Eigen::Vector3d> ComputeLocalExtremaMap() const {
        const double ninf = -std::numeric_limits<double>::infinity(), inf = std::numeric_limits<double>::infinity();
        ::VoxelGrid::VoxelGrid<Eigen::Vector3d> map(origin_transform_, GetResolution(), GetNumXCells(), GetNumYCells(), GetNumZCells(),
                                                   Eigen::Vector3d(ninf, ninf, ninf));
        const std::vector<uint32_t> idx = ComputeLocalExtremaIndices();
        const int64_t ny = GetNumYCells(), nz = GetNumZCells();
        std::vector<Eigen::Vector3d>& out = map.GetMutableRawData();
        for (size_t i = 0; i < idx.size(); ++i) {
            const uint32_t e = idx[i];
            if (e == 0xFFFFFFFFu) { out[i] = Eigen::Vector3d(inf, inf, inf); continue; }
            const Eigen::Vector4d l = GridIndexToLocationGridFrame((int64_t)e / (ny * nz), ((int64_t)e / nz) % ny, (int64_t)e % nz);
            out[i] = Eigen::Vector3d(l(0), l(1), l(2));
        }
        return map;
    }

    // ---- trilinear distance estimate (:699-961) ----------------------------------------------
protected:
    double CorrectedCenterDistance(const int64_t x, const int64_t y, const int64_t z) const {
        if (!IndexInBounds(x, y, z)) throw std::invalid_argument("Index out of bounds");
        const double d = (double)AccessIndex(GetDataIndex(x, y, z));
        const double half = GetResolution() * 0.5;              // shrink by half a cell toward the surface (:773-796)
        return d >= 0.0 ? d - half : d + half;
    }
    static std::pair<int64_t, int64_t> AxisInterpolationIndices(const int64_t i, const int64_t n, const double offset) {
        int64_t lower = i, upper = i;                            // (:798-833)
        if (offset >= 0.0) {
            upper = i + 1;
            if (upper >= n) { upper = i; lower = i - 1; if (lower < 0) lower = i; }
        } else {
            lower = i - 1;
            if (lower < 0) { upper = i + 1; lower = i; if (upper >= n) upper = i; }
        }
        return std::make_pair(lower, upper);
    }
    static double Bilinear(double l1, double h1, double l2, double h2, double q1, double q2, double ll, double lh, double hl, double hh) {
        // (multiplier * [h1-q1, q1-l1]) * [[ll, lh], [hl, hh]] * [h2-q2, q2-l2]^T, evaluated left to right (:699-727)
        return BilinearT<double>(l1, h1, l2, h2, q1, q2, ll, lh, hl, hh);
    }
    // EstimateDistanceInterpolateFromNeighborsGridFrame (:836-915) over T = double or AutoDiff3 (autodiff.hpp): the cell (x, y,
    // z) is inside the grid; the corners are chosen from the value of q.
    template <typename T>
    T EstimateFromNeighborsGridFrameT(const T& q0, const T& q1, const T& q2, const int64_t x, const int64_t y, const int64_t z) const {
        const Eigen::Vector4d c = GridIndexToLocationGridFrame(x, y, z);
        const auto xi = AxisInterpolationIndices(x, GetNumXCells(), ValueOf(q0) - c(0));
        const auto yi = AxisInterpolationIndices(y, GetNumYCells(), ValueOf(q1) - c(1));
        const auto zi = AxisInterpolationIndices(z, GetNumZCells(), ValueOf(q2) - c(2));
        const Eigen::Vector4d lo = GridIndexToLocationGridFrame(xi.first, yi.first, zi.first);
        auto D = [&](int64_t a, int64_t b, int64_t cc) { return CorrectedCenterDistance(a, b, cc); };
        return TrilinearT<T>(lo(0), lo(1), lo(2), GetResolution(), q0, q1, q2, D(xi.first, yi.first, zi.first),
                             D(xi.first, yi.first, zi.second), D(xi.first, yi.second, zi.first), D(xi.first, yi.second, zi.second),
                             D(xi.second, yi.first, zi.first), D(xi.second, yi.first, zi.second), D(xi.second, yi.second, zi.first),
                             D(xi.second, yi.second, zi.second));            // (slope (pz - mz) * (1 / res), :745-771)
    }
    double EstimateFromNeighborsGridFrame(const Eigen::Vector4d& q, const int64_t x, const int64_t y, const int64_t z) const {
        return EstimateFromNeighborsGridFrameT<double>(q(0), q(1), q(2), x, y, z);
    }

public:
    std::pair<double, bool> EstimateDistance4d(const Eigen::Vector4d& location) const {
        const GRID_INDEX i = LocationToGridIndex4d(location);
        if (!IndexInBounds(i)) return std::make_pair((double)GetOOBValue(), false);
        return std::make_pair(EstimateFromNeighborsGridFrame(inverse_origin_transform_ * location, i.x, i.y, i.z), true);
    }
    std::pair<double, bool> EstimateDistance3d(const Eigen::Vector3d& l) const { return EstimateDistance4d(Eigen::Vector4d(l.x(), l.y(), l.z(), 1.0)); }
    std::pair<double, bool> EstimateDistance(const double x, const double y, const double z) const {
        return EstimateDistance4d(Eigen::Vector4d(x, y, z, 1.0));
    }

    // ---- smooth and autodiff gradients, DistanceToBoundary (:528-653, :963-988) -----------------------------------------------
    // One core, QueryGradient4d, answers all three kinds without throwing for a point, and is the yardstick of the GPU
    // (sdfgpu_query_gradients, include/sdfgpu.h "Interpolated gradients"): its arithmetic order IS the specification --
    // eigen_lite's left-to-right sums, no fused multiply-add, the operators of AutoDiff3 (autodiff.hpp).  Byte equality with real
    // Eigen (AutoDiffScalar, its matrix products and Transform * vector) is UNVERIFIED: Eigen is not installed here.
    //   SDFGPU_QUERY_AUTODIFF_GRADIENT: the location (x, y, z, 1) seeded with Unit(0..2) goes through W = inverse_origin_transform_
    //     and the trilinear estimate as AutoDiff3; value = EstimateDistance4d's bits, gradient = the derivatives (world frame).
    //   SDFGPU_QUERY_SMOOTH_GRADIENT: w = |window|; the seven EstimateDistance calls at p and p -+ w along each world axis, then
    //     per axis (d+ - d-) / ((a + w) - (a - w)), else (d - d-) / (a - (a - w)), else (d+ - d) / ((a + w) - a), as
    //     ComputeAxisSmoothGradient (:656-697) decides; value = the estimate at p.  A window of 0 gives 0 / 0 = NaN.
    //   SDFGPU_QUERY_DISTANCE_TO_BOUNDARY: (a, b, c) = W (p, 1); each displacement std::min(a, size - a) (size = cells * res);
    //     inside when all are >= 0; value = the displacement with the first least |displacement| (strict <, as minCoeff).
    // A window end or point "in the grid" is decided on the floored doubles (GridFrameCell), never by an int64 cast.
    // Two deviations from the reference (the precedent is the projection members): a NaN or infinite coordinate passed to a
    // smooth or autodiff member throws std::invalid_argument (the reference casts NaN to int64), and so does a non-finite
    // window.  The core reports the former as SDFGPU_QUERY_NON_FINITE (value and gradient NaN) and throws for the latter.
    struct GradientQueryResult {
        double value;                                            // estimate (oob outside), or the boundary displacement
        double gradient[3];                                      // world frame; NaN where the reference returns no vector
        uint8_t status;                                          // SDFGPU_QUERY_*
    };

    GradientQueryResult QueryGradient4d(const Eigen::Vector4d& location, const int kind, const double window = 0.0) const {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        GradientQueryResult r{nan, {nan, nan, nan}, (uint8_t)SDFGPU_QUERY_OK};
        const double x = location(0), y = location(1), z = location(2);
        if (kind == SDFGPU_QUERY_DISTANCE_TO_BOUNDARY) {
            const std::pair<double, bool> b = DistanceToBoundary4d(location);
            r.value = b.first;
            r.status = b.second ? (uint8_t)SDFGPU_QUERY_OK : (uint8_t)SDFGPU_QUERY_OUTSIDE;
            return r;
        }
        if (kind != SDFGPU_QUERY_SMOOTH_GRADIENT && kind != SDFGPU_QUERY_AUTODIFF_GRADIENT)
            throw std::invalid_argument("QueryGradient4d: unknown kind " + std::to_string(kind));
        if (!std::isfinite(window)) throw std::invalid_argument("GetSmoothGradient: the window size must be finite");
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) { r.status = SDFGPU_QUERY_NON_FINITE; return r; }
        const Eigen::Vector4d q = inverse_origin_transform_ * Eigen::Vector4d(x, y, z, 1.0);
        GRID_INDEX index;
        if (!GridFrameCell(q, index)) { r.value = (double)GetOOBValue(); r.status = SDFGPU_QUERY_OUTSIDE; return r; }
        if (kind == SDFGPU_QUERY_AUTODIFF_GRADIENT) {
            const AutoDiff3 p0 = AutoDiff3::Seed(x, 0), p1 = AutoDiff3::Seed(y, 1), p2 = AutoDiff3::Seed(z, 2);
            double w2g[12];
            for (int row = 0; row < 3; ++row)
                for (int col = 0; col < 4; ++col) w2g[row * 4 + col] = inverse_origin_transform_.matrix()(row, col);
            const AutoDiff3 g0 = TransformRowT(w2g, p0, p1, p2), g1 = TransformRowT(w2g + 4, p0, p1, p2), g2 = TransformRowT(w2g + 8, p0, p1, p2);
            const AutoDiff3 d = EstimateFromNeighborsGridFrameT<AutoDiff3>(g0, g1, g2, index.x, index.y, index.z);
            r.value = d.v;
            r.gradient[0] = d.d[0]; r.gradient[1] = d.d[1]; r.gradient[2] = d.d[2];
            return r;
        }
        const double w = std::abs(window);
        const std::pair<double, bool> c = EstimateInGrid(x, y, z);
        r.value = c.first;
        const double p[3] = {x, y, z};
        for (int axis = 0; axis < 3; ++axis) {
            double lo[3] = {x, y, z}, hi[3] = {x, y, z};
            lo[axis] = p[axis] - w;
            hi[axis] = p[axis] + w;
            const std::pair<double, bool> m = EstimateInGrid(lo[0], lo[1], lo[2]), pl = EstimateInGrid(hi[0], hi[1], hi[2]);
            // ComputeAxisSmoothGradient (:656-697); the query point is available here
            if (m.second && pl.second) r.gradient[axis] = (pl.first - m.first) / (hi[axis] - lo[axis]);
            else if (m.second) r.gradient[axis] = (c.first - m.first) / (p[axis] - lo[axis]);
            else if (pl.second) r.gradient[axis] = (pl.first - c.first) / (hi[axis] - p[axis]);
            else {
                r.gradient[0] = r.gradient[1] = r.gradient[2] = nan;
                r.status = SDFGPU_QUERY_WINDOW_TOO_LARGE;
                return r;
            }
        }
        return r;
    }

    // reference-named members
    std::vector<double> GetSmoothGradient(const double x, const double y, const double z, const double nominal_window_size) const {
        return GradientVector(QueryGradient4d(Eigen::Vector4d(x, y, z, 1.0), SDFGPU_QUERY_SMOOTH_GRADIENT, nominal_window_size));
    }
    std::vector<double> GetSmoothGradient3d(const Eigen::Vector3d& location, const double nominal_window_size) const {
        return GetSmoothGradient(location.x(), location.y(), location.z(), nominal_window_size);
    }
    std::vector<double> GetSmoothGradient4d(const Eigen::Vector4d& location, const double nominal_window_size) const {
        return GetSmoothGradient(location(0), location(1), location(2), nominal_window_size);
    }
    std::vector<double> GetSmoothGradient(const GRID_INDEX& index, const double nominal_window_size) const {
        return GetSmoothGradient4d(GridIndexToLocation(index), nominal_window_size);
    }
    std::vector<double> GetSmoothGradient(const int64_t x_index, const int64_t y_index, const int64_t z_index,
                                          const double nominal_window_size) const {
        return GetSmoothGradient4d(GridIndexToLocation(x_index, y_index, z_index), nominal_window_size);
    }
    // (the reference notes "TODO: this does not work if you query at cell centers!": there the corners switch sides, and the
    // derivative is the one-sided one of the corners chosen -- kept as is)
    std::vector<double> GetAutoDiffGradient(const double x, const double y, const double z) const {
        return GradientVector(QueryGradient4d(Eigen::Vector4d(x, y, z, 1.0), SDFGPU_QUERY_AUTODIFF_GRADIENT));
    }
    std::vector<double> GetAutoDiffGradient3d(const Eigen::Vector3d& location) const {
        return GetAutoDiffGradient(location.x(), location.y(), location.z());
    }
    std::vector<double> GetAutoDiffGradient4d(const Eigen::Vector4d& location) const {
        return GetAutoDiffGradient(location(0), location(1), location(2));
    }
    std::vector<double> GetAutoDiffGradient(const GRID_INDEX& index) const { return GetAutoDiffGradient4d(GridIndexToLocation(index)); }
    std::vector<double> GetAutoDiffGradient(const int64_t x_index, const int64_t y_index, const int64_t z_index) const {
        return GetAutoDiffGradient4d(GridIndexToLocation(x_index, y_index, z_index));
    }

    std::pair<double, bool> DistanceToBoundary(const double x, const double y, const double z) const {
        return DistanceToBoundary4d(Eigen::Vector4d(x, y, z, 1.0));
    }
    std::pair<double, bool> DistanceToBoundary3d(const Eigen::Vector3d& location) const {
        return DistanceToBoundary(location.x(), location.y(), location.z());
    }
    std::pair<double, bool> DistanceToBoundary4d(const Eigen::Vector4d& location) const {
        const Eigen::Vector4d a = inverse_origin_transform_ * location;
        const double displacements[3] = {std::min(a(0), x_size_ - a(0)), std::min(a(1), y_size_ - a(1)), std::min(a(2), z_size_ - a(2))};
        const bool point_inside = displacements[0] >= 0.0 && displacements[1] >= 0.0 && displacements[2] >= 0.0;
        int min_index = 0;                                       // Eigen's minCoeff(&i): the first least, strict <
        double least = std::abs(displacements[0]);
        for (int i = 1; i < 3; ++i)
            if (std::abs(displacements[i]) < least) { least = std::abs(displacements[i]); min_index = i; }
        return {displacements[min_index], point_inside};
    }

protected:
    // EstimateDistance(x, y, z) with the cell decided on the floored doubles
    std::pair<double, bool> EstimateInGrid(const double x, const double y, const double z) const {
        const Eigen::Vector4d q = inverse_origin_transform_ * Eigen::Vector4d(x, y, z, 1.0);
        GRID_INDEX index;
        if (!GridFrameCell(q, index)) return std::make_pair((double)GetOOBValue(), false);
        return std::make_pair(EstimateFromNeighborsGridFrame(q, index.x, index.y, index.z), true);
    }
    static std::vector<double> GradientVector(const GradientQueryResult& r) {
        switch (r.status) {
            case SDFGPU_QUERY_OK: return std::vector<double>{r.gradient[0], r.gradient[1], r.gradient[2]};
            case SDFGPU_QUERY_OUTSIDE: return std::vector<double>();
            case SDFGPU_QUERY_WINDOW_TOO_LARGE: throw std::runtime_error("Window size for GetSmoothGradient is too large for SDF");
            default: throw std::invalid_argument("Cannot compute a gradient at a non-finite location");
        }
    }

public:

    // ---- projection out of collision / into the valid volume (:996-1190) ----------------------------------------------------
    // One counted walk is the core of every member below and the yardstick of the GPU (sdfgpu_project_points, include/sdfgpu.h
    // "Projection"): its arithmetic order IS the specification -- eigen_lite's left-to-right sums, no fused multiply-add (the
    // in-tree builds pass -ffp-contract=off or target no FMA).  Byte equality with real Eigen is UNVERIFIED: Eigen is not
    // installed here and its vectorised norm() may sum in another order.
    // Two deviations from the reference, which loops without a bound and casts NaN coordinates to int64:
    //   - a walk stops after `max_steps` steps (0 = the library default, sdfgpu_project_step_limit): the reference-named members
    //     throw std::runtime_error naming the limit, the counted walk reports SDFGPU_PROJECT_STEP_LIMIT;
    //   - a NaN or infinite coordinate is refused: std::invalid_argument, or SDFGPU_PROJECT_NON_FINITE.
    struct ProjectionResult {
        Eigen::Vector4d location;                                // world frame (grid frame from the GridFrame core)
        uint8_t status;                                          // SDFGPU_PROJECT_*
        int32_t steps;
    };

    // The step limit a walk with these arguments uses; std::invalid_argument for a step that is not positive and finite or a
    // negative max_steps.
    int ProjectionStepLimit(const double stepsize_multiplier, const int max_steps = 0) const {
        int limit = 0;
        if (sdfgpu_project_step_limit(GetNumXCells(), GetNumYCells(), GetNumZCells(), stepsize_multiplier, max_steps, &limit) != SDFGPU_OK)
            throw std::invalid_argument("projection: stepsize_multiplier must be positive and finite and max_steps >= 0");
        return limit;
    }

    // ProjectOutOfCollisionToMinimumDistanceGridFrame (:1071-1122) with the walk counted and bounded.  A failed walk keeps the
    // last location it reached.
    ProjectionResult ProjectOutOfCollisionToMinimumDistanceGridFrameCounted(const Eigen::Vector4d& grid_frame_location,
                                                                           const double minimum_distance,
                                                                           const double stepsize_multiplier, const int step_limit) const {
        ProjectionResult r{grid_frame_location, (uint8_t)SDFGPU_PROJECT_CONVERGED, 0};
        Eigen::Vector4d& p = r.location;
        const double minimum_distance_with_margin = minimum_distance + GetResolution() * stepsize_multiplier * 1e-4;
        const double max_stepsize = GetResolution() * stepsize_multiplier;
        GRID_INDEX index;
        if (!GridFrameCell(p, index)) { r.status = SDFGPU_PROJECT_LEFT_GRID; return r; }
        double sdf_dist = EstimateFromNeighborsGridFrame(p, index.x, index.y, index.z);
        while (sdf_dist <= minimum_distance) {
            if (r.steps >= step_limit) { r.status = SDFGPU_PROJECT_STEP_LIMIT; return r; }
            const std::vector<double> gradient = GetGridAlignedGradient(index.x, index.y, index.z, true);
            if (gradient.size() != 3) { r.status = SDFGPU_PROJECT_NO_GRADIENT; return r; }
            const Eigen::Vector4d grad_vector(gradient[0], gradient[1], gradient[2], 0.0);
            if (!(grad_vector.norm() > GetResolution() * 0.25)) { r.status = SDFGPU_PROJECT_FLAT_GRADIENT; return r; }
            const double step_distance = std::min(max_stepsize, minimum_distance_with_margin - sdf_dist);
            p += grad_vector.normalized() * step_distance;
            r.steps++;
            if (!GridFrameCell(p, index)) { r.status = SDFGPU_PROJECT_LEFT_GRID; return r; }
            sdf_dist = EstimateFromNeighborsGridFrame(p, index.x, index.y, index.z);
        }
        return r;
    }

    // The whole world-frame call, counted: ProjectOutOfCollisionToMinimumDistance4d (:1041-1069) or, with
    // into_valid_volume_only, ProjectIntoValidVolumeToMinimumDistance4d (:1158-1190).  Never throws for a point; throws
    // std::invalid_argument for bad arguments (ProjectionStepLimit).
    ProjectionResult ProjectCounted4d(const Eigen::Vector4d& location, const double minimum_distance, const double stepsize_multiplier,
                                      const bool into_valid_volume_only, const int max_steps = 0) const {
        const int step_limit = ProjectionStepLimit(stepsize_multiplier, max_steps);
        if (!std::isfinite(location(0)) || !std::isfinite(location(1)) || !std::isfinite(location(2)))
            return ProjectionResult{location, (uint8_t)SDFGPU_PROJECT_NON_FINITE, 0};
        if (into_valid_volume_only)
            return ProjectionResult{ClampIntoValidVolume(location, minimum_distance), (uint8_t)SDFGPU_PROJECT_CONVERGED, 0};
        GRID_INDEX index;
        const Eigen::Vector4d start = GridFrameCell(inverse_origin_transform_ * location, index) ? location
                                                                                               : ClampIntoValidVolume(location, 0.0);
        ProjectionResult r = ProjectOutOfCollisionToMinimumDistanceGridFrameCounted(inverse_origin_transform_ * start, minimum_distance,
                                                                                   stepsize_multiplier, step_limit);
        r.location = GetOriginTransform() * r.location;
        return r;
    }

    // reference-named members (:996-1190); max_steps is an addition with a default (see above)
    Eigen::Vector4d ProjectOutOfCollisionToMinimumDistance4d(const Eigen::Vector4d& location, const double minimum_distance,
                                                             const double stepsize_multiplier = 1.0 / 8.0, const int max_steps = 0) const {
        return ThrowOnProjectionStatus(ProjectCounted4d(location, minimum_distance, stepsize_multiplier, false, max_steps));
    }
    Eigen::Vector3d ProjectOutOfCollisionToMinimumDistance(const double x, const double y, const double z, const double minimum_distance,
                                                           const double stepsize_multiplier = 1.0 / 8.0, const int max_steps = 0) const {
        return Head3(ProjectOutOfCollisionToMinimumDistance4d(Eigen::Vector4d(x, y, z, 1.0), minimum_distance, stepsize_multiplier, max_steps));
    }
    Eigen::Vector3d ProjectOutOfCollisionToMinimumDistance3d(const Eigen::Vector3d& location, const double minimum_distance,
                                                             const double stepsize_multiplier = 1.0 / 8.0, const int max_steps = 0) const {
        return ProjectOutOfCollisionToMinimumDistance(location.x(), location.y(), location.z(), minimum_distance, stepsize_multiplier, max_steps);
    }
    Eigen::Vector4d ProjectOutOfCollision4d(const Eigen::Vector4d& location, const double stepsize_multiplier = 1.0 / 8.0,
                                            const int max_steps = 0) const {
        return ProjectOutOfCollisionToMinimumDistance4d(location, 0.0, stepsize_multiplier, max_steps);
    }
    Eigen::Vector3d ProjectOutOfCollision(const double x, const double y, const double z, const double stepsize_multiplier = 1.0 / 8.0,
                                          const int max_steps = 0) const {
        return Head3(ProjectOutOfCollision4d(Eigen::Vector4d(x, y, z, 1.0), stepsize_multiplier, max_steps));
    }
    Eigen::Vector3d ProjectOutOfCollision3d(const Eigen::Vector3d& location, const double stepsize_multiplier = 1.0 / 8.0,
                                            const int max_steps = 0) const {
        return ProjectOutOfCollision(location.x(), location.y(), location.z(), stepsize_multiplier, max_steps);
    }
    Eigen::Vector4d ProjectIntoValidVolumeToMinimumDistance4d(const Eigen::Vector4d& location, const double minimum_distance) const {
        if (!std::isfinite(location(0)) || !std::isfinite(location(1)) || !std::isfinite(location(2)))
            throw std::invalid_argument("Cannot project a non-finite location");
        return ClampIntoValidVolume(location, minimum_distance);
    }
    Eigen::Vector4d ProjectIntoValidVolume4d(const Eigen::Vector4d& location) const {
        return ProjectIntoValidVolumeToMinimumDistance4d(location, 0.0);
    }
    Eigen::Vector3d ProjectIntoValidVolumeToMinimumDistance(const double x, const double y, const double z, const double minimum_distance) const {
        return Head3(ProjectIntoValidVolumeToMinimumDistance4d(Eigen::Vector4d(x, y, z, 1.0), minimum_distance));
    }
    Eigen::Vector3d ProjectIntoValidVolumeToMinimumDistance3d(const Eigen::Vector3d& location, const double minimum_distance) const {
        return ProjectIntoValidVolumeToMinimumDistance(location.x(), location.y(), location.z(), minimum_distance);
    }
    Eigen::Vector3d ProjectIntoValidVolume(const double x, const double y, const double z) const {
        return Head3(ProjectIntoValidVolume4d(Eigen::Vector4d(x, y, z, 1.0)));
    }
    Eigen::Vector3d ProjectIntoValidVolume3d(const Eigen::Vector3d& location) const {
        return ProjectIntoValidVolume(location.x(), location.y(), location.z());
    }

protected:
    static Eigen::Vector3d Head3(const Eigen::Vector4d& v) { return Eigen::Vector3d(v(0), v(1), v(2)); }
    // PointInFrameToGridIndex4d + IndexInBounds, decided on the floored doubles before any cast to int64 (the reference casts
    // first, which is undefined for coordinates beyond int64; for every other input the answer is the same).
    bool GridFrameCell(const Eigen::Vector4d& p, GRID_INDEX& index) const {
        const double fx = std::floor(p(0) * inv_cell_x_size_), fy = std::floor(p(1) * inv_cell_y_size_),
                     fz = std::floor(p(2) * inv_cell_z_size_);
        if (!(fx >= 0.0 && fy >= 0.0 && fz >= 0.0 && fx < (double)GetNumXCells() && fy < (double)GetNumYCells() && fz < (double)GetNumZCells()))
            return false;
        index = GRID_INDEX((int64_t)fx, (int64_t)fy, (int64_t)fz);
        return true;
    }
    // ProjectIntoValidVolumeToMinimumDistance4d's body (:1158-1190): the input itself when no coordinate moves
    Eigen::Vector4d ClampIntoValidVolume(const Eigen::Vector4d& location, const double minimum_distance) const {
        const Eigen::Vector4d g = inverse_origin_transform_ * location;
        const double dist_margin = minimum_distance + GetResolution() * 1e-4;
        const double x = std::min(x_size_ - dist_margin, std::max(dist_margin, g(0)));
        const double y = std::min(y_size_ - dist_margin, std::max(dist_margin, g(1)));
        const double z = std::min(z_size_ - dist_margin, std::max(dist_margin, g(2)));
        if (x != g(0) || y != g(1) || z != g(2)) return GetOriginTransform() * Eigen::Vector4d(x, y, z, 1.0);
        return location;
    }
    Eigen::Vector4d ThrowOnProjectionStatus(const ProjectionResult& r) const {
        switch (r.status) {
            case SDFGPU_PROJECT_CONVERGED: return r.location;
            case SDFGPU_PROJECT_FLAT_GRADIENT: throw std::runtime_error("Encountered flat gradient - stuck");
            case SDFGPU_PROJECT_NO_GRADIENT: throw std::runtime_error("Failed to compute gradient - out of SDF?");
            case SDFGPU_PROJECT_LEFT_GRID: throw std::invalid_argument("Index out of bounds");
            case SDFGPU_PROJECT_NON_FINITE: throw std::invalid_argument("Cannot project a non-finite location");
            default:
                throw std::runtime_error("Projection did not converge within the step limit of " + std::to_string(r.steps) + " steps");
        }
    }

public:

    // ---- serialisation (src/sdf_tools/sdf.cpp:213-502) ------------------------------------------
    using FloatSerializer = std::function<uint64_t(const float&, std::vector<uint8_t>&)>;
    using FloatDeserializer = std::function<std::pair<float, uint64_t>(const std::vector<uint8_t>&, const uint64_t)>;

    uint64_t SerializeSelf(std::vector<uint8_t>& buffer,
                           const FloatSerializer& value_serializer = arc_utilities::SerializeFixedSizePOD<float>) const override {
        (void)value_serializer;
        const uint64_t start = buffer.size();
        BaseSerializeSelf(buffer, arc_utilities::SerializeFixedSizePOD<float>);
        arc_utilities::SerializeString(frame_, buffer);
        arc_utilities::SerializeFixedSizePOD<uint8_t>((uint8_t)locked_, buffer);
        return buffer.size() - start;
    }
    uint64_t DeserializeSelf(const std::vector<uint8_t>& buffer, const uint64_t current,
                             const FloatDeserializer& value_deserializer = arc_utilities::DeserializeFixedSizePOD<float>) override {
        (void)value_deserializer;
        uint64_t pos = current;
        pos += BaseDeserializeSelf(buffer, pos, arc_utilities::DeserializeFixedSizePOD<float>);
        const auto f = arc_utilities::DeserializeString(buffer, pos); pos += f.second;
        const auto l = arc_utilities::DeserializeFixedSizePOD<uint8_t>(buffer, pos); pos += l.second;
        frame_ = f.first;
        locked_ = (bool)l.first;
        return pos - current;
    }

    static void SaveToFile(const SignedDistanceField& sdf, const std::string& filepath, const bool compress) {
        std::vector<uint8_t> buffer;
        sdf.SerializeSelf(buffer);
        std::ofstream out(filepath, std::ios::out | std::ios::binary);
        const std::vector<uint8_t> body = compress ? ZlibHelpers::CompressBytes(buffer) : buffer;
        out.write(compress ? "SDFZ" : "SDFR", 4);                 // 4-byte magic (:392-416)
        out.write(reinterpret_cast<const char*>(body.data()), (std::streamsize)body.size());
    }
    static SignedDistanceField LoadFromFile(const std::string& filepath) {
        std::ifstream in(filepath, std::ios::in | std::ios::binary);
        if (!in.good()) throw std::invalid_argument("File does not exist");
        std::vector<uint8_t> all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (all.size() < 4) throw std::invalid_argument("File is too small");
        const std::string magic(all.begin(), all.begin() + 4);
        std::vector<uint8_t> body(all.begin() + 4, all.end());
        SignedDistanceField sdf;
        if (magic == "SDFZ") sdf.DeserializeSelf(ZlibHelpers::DecompressBytes(body), 0);
        else if (magic == "SDFR") sdf.DeserializeSelf(body, 0);
        else throw std::invalid_argument("File has invalid header [" + magic + "]");
        return sdf;
    }
    static SDF GetMessageRepresentation(const SignedDistanceField& sdf) {
        SDF msg;                                                  // always zlib-compressed (:472-483)
        msg.header.frame_id = sdf.GetFrame();
        std::vector<uint8_t> buffer;
        sdf.SerializeSelf(buffer);
        msg.serialized_sdf = ZlibHelpers::CompressBytes(buffer);
        msg.is_compressed = true;
        return msg;
    }
    static SignedDistanceField LoadFromMessageRepresentation(const SDF& message) {
        SignedDistanceField sdf;
        if (message.is_compressed) sdf.DeserializeSelf(ZlibHelpers::DecompressBytes(message.serialized_sdf), 0);
        else sdf.DeserializeSelf(message.serialized_sdf, 0);
        return sdf;
    }
};

}  // namespace sdf_tools
