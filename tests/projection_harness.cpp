// projection_harness.cpp -- drives SignedDistanceField's projection members (include/sdf_tools/sdf.hpp) from Python through a
// plain C interface, for tests/test_projection_cpu.py: a field of any contents and origin, the counted walk, the reference-named
// members with the exception each one throws, and EstimateDistance.  Built with -ffp-contract=off against include/ and
// libsdfgpu.so (sdfgpu_project_step_limit); no GPU is used.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "sdf_tools/sdf.hpp"

using sdf_tools::SignedDistanceField;

namespace {
void copy_msg(const char* what, char* msg, int len) {
    if (msg && len > 0) { std::strncpy(msg, what, (size_t)len - 1); msg[len - 1] = 0; }
}
void put(const Eigen::Vector4d& v, double* out) { out[0] = v(0); out[1] = v(1); out[2] = v(2); out[3] = v(3); }
void put(const Eigen::Vector3d& v, double* out) { out[0] = v(0); out[1] = v(1); out[2] = v(2); out[3] = 1.0; }
}  // namespace

extern "C" {

// origin: 16 doubles, row-major 4x4; data: nx * ny * nz floats, [x][y][z]
void* ph_create(int64_t nx, int64_t ny, int64_t nz, double res, const double* origin, const float* data, float oob) {
    Eigen::Isometry3d t = Eigen::Isometry3d::Identity();
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) t.matrix()(r, c) = origin[r * 4 + c];
    SignedDistanceField* s = new SignedDistanceField(t, "world", res, nx, ny, nz, oob);
    for (int64_t x = 0; x < nx; ++x)
        for (int64_t y = 0; y < ny; ++y)
            for (int64_t z = 0; z < nz; ++z) s->SetValue(x, y, z, data[(x * ny + y) * nz + z]);
    return s;
}

void ph_destroy(void* h) { delete static_cast<SignedDistanceField*>(h); }

// ProjectCounted4d: returns the status, out[0..3] the world-frame location, *steps the steps
int ph_counted(void* h, double x, double y, double z, double minimum_distance, double stepsize_multiplier, int into_valid_volume_only,
               int max_steps, double* out, int* steps, char* msg, int msglen) {
    const SignedDistanceField& s = *static_cast<SignedDistanceField*>(h);
    try {
        const SignedDistanceField::ProjectionResult r =
            s.ProjectCounted4d(Eigen::Vector4d(x, y, z, 1.0), minimum_distance, stepsize_multiplier, into_valid_volume_only != 0, max_steps);
        put(r.location, out);
        *steps = r.steps;
        return r.status;
    } catch (const std::invalid_argument& e) {
        copy_msg(e.what(), msg, msglen);
        return -2;
    }
}

// The reference-named members.  kind: 0 ProjectOutOfCollision, 1 ProjectOutOfCollisionToMinimumDistance, 2 ProjectIntoValidVolume,
// 3 ProjectIntoValidVolumeToMinimumDistance; form: 0 (x, y, z), 1 3d, 2 4d.  Returns 0 (out[0..3] = result), 1 std::runtime_error,
// 2 std::invalid_argument (msg = what()).  max_steps < 0: the reference's signature (the default limit).
int ph_member(void* h, int kind, int form, double x, double y, double z, double minimum_distance, double stepsize_multiplier, int max_steps,
              double* out, char* msg, int msglen) {
    const SignedDistanceField& s = *static_cast<SignedDistanceField*>(h);
    const Eigen::Vector3d v3(x, y, z);
    const Eigen::Vector4d v4(x, y, z, 1.0);
    const int ms = max_steps < 0 ? 0 : max_steps;
    try {
        switch (kind * 3 + form) {
            case 0: put(max_steps < 0 ? s.ProjectOutOfCollision(x, y, z, stepsize_multiplier) : s.ProjectOutOfCollision(x, y, z, stepsize_multiplier, ms), out); break;
            case 1: put(s.ProjectOutOfCollision3d(v3, stepsize_multiplier, ms), out); break;
            case 2: put(s.ProjectOutOfCollision4d(v4, stepsize_multiplier, ms), out); break;
            case 3:
                put(max_steps < 0 ? s.ProjectOutOfCollisionToMinimumDistance(x, y, z, minimum_distance, stepsize_multiplier)
                                  : s.ProjectOutOfCollisionToMinimumDistance(x, y, z, minimum_distance, stepsize_multiplier, ms), out);
                break;
            case 4: put(s.ProjectOutOfCollisionToMinimumDistance3d(v3, minimum_distance, stepsize_multiplier, ms), out); break;
            case 5: put(s.ProjectOutOfCollisionToMinimumDistance4d(v4, minimum_distance, stepsize_multiplier, ms), out); break;
            case 6: put(s.ProjectIntoValidVolume(x, y, z), out); break;
            case 7: put(s.ProjectIntoValidVolume3d(v3), out); break;
            case 8: put(s.ProjectIntoValidVolume4d(v4), out); break;
            case 9: put(s.ProjectIntoValidVolumeToMinimumDistance(x, y, z, minimum_distance), out); break;
            case 10: put(s.ProjectIntoValidVolumeToMinimumDistance3d(v3, minimum_distance), out); break;
            case 11: put(s.ProjectIntoValidVolumeToMinimumDistance4d(v4, minimum_distance), out); break;
            default: return -1;
        }
        return 0;
    } catch (const std::invalid_argument& e) {
        copy_msg(e.what(), msg, msglen);
        return 2;
    } catch (const std::runtime_error& e) {
        copy_msg(e.what(), msg, msglen);
        return 1;
    }
}

// EstimateDistance(x, y, z): returns 1 inside the grid (d = the estimate), 0 outside
int ph_estimate(void* h, double x, double y, double z, double* d) {
    const std::pair<double, bool> r = static_cast<SignedDistanceField*>(h)->EstimateDistance(x, y, z);
    *d = r.first;
    return r.second ? 1 : 0;
}

int ph_step_limit(void* h, double stepsize_multiplier, int max_steps) {
    try {
        return static_cast<SignedDistanceField*>(h)->ProjectionStepLimit(stepsize_multiplier, max_steps);
    } catch (const std::invalid_argument&) {
        return -1;
    }
}

}  // extern "C"
