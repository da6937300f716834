// sdf_builder -- sdf_tools::SDF_Builder (reference include/sdf_tools/sdf_builder.hpp, src/sdf_tools/sdf_builder.cpp): from the
// shapes of a planning scene to a collision map and a signed distance field.  The reference places a cube of side `resolution` at
// every voxel centre and asks MoveIt whether it collides with the world, one check per voxel on one host thread; here the shapes go to
// the GPU (a few KB, and the meshes' vertices and triangles), the same predicate is decided there for every voxel (include/sdfgpu.h
// "Shape rasteriser" and "Planes and triangle meshes", DESIGN.md sections 26 and 27) and the bit field it writes feeds the SDF build
// in place.  No per-voxel data crosses the bus on the way in.
//
// What is kept: the names, the USE_* constants, the exception texts, the cached results, the virtual border off.
// What differs, because there is no ROS here:
//   - no ros::NodeHandle; in place of the planning-scene service name an optional std::function<PlanningScene(uint8_t mode)> that is
//     called with the mode where the reference calls the service.  Without it the non-cached modes throw the reference's "No planning
//     scene available".
//   - the mode selects which parts of the fetched scene are kept (the reference asks the service for those components only):
//     USE_ONLY_OCTOMAP the octomap, USE_ONLY_COLLISION_OBJECTS the collision objects, USE_FULL_PLANNING_SCENE both.
//     UpdatePlanningSceneFromMessage keeps the whole message.
//   - the messages are the plain mirrors of planning_scene.hpp; the octomap arrives as boxes.
//   - primitives are boxes, spheres and cylinders; a cone is refused with std::invalid_argument naming the object (the reference
//     hands it to FCL).  Meshes are taken as their surface (a triangle soup: a probe wholly inside a closed mesh is empty) and planes
//     as infinite and without thickness, each with a pose of its own; one without a pose, with a vertex index out of range, a vertex,
//     a normal or a pose that is not finite, or a zero normal is refused in the same way.
//   - whether FCL counts exact contact as a collision, and whether it reads meshes and planes as said, is UNVERIFIED (FCL and MoveIt
//     are not available to this project); here touching counts.
// Extensions: UpdateSDFDevice (the field stays in HBM) and UpdateTaggedCollisionMap (object ids: the 1-based index of the collision
// object, and one more id for the octomap).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "arc_utilities/voxel_grid.hpp"
#include "sdf_tools/device_sdf.hpp"
#include "sdf_tools/gpu_context.hpp"
#include "sdf_tools/planning_scene.hpp"
#include "sdf_tools/sdf.hpp"
#include "sdf_tools/tagged_object_collision_map.hpp"
#include "sdfgpu.h"

namespace sdf_tools {

static const uint8_t USE_CACHED = 0x00;
static const uint8_t USE_ONLY_OCTOMAP = 0x01;
static const uint8_t USE_ONLY_COLLISION_OBJECTS = 0x02;
static const uint8_t USE_FULL_PLANNING_SCENE = 0x03;

// How a collision object's meshes are filled (an extension; SetMeshFill, SetObjectMeshFill).  SURFACE, the default, is the reading
// above: a triangle soup.  SOLID also fills the cells whose centres lie inside a closed mesh (even-odd, per mesh: include/sdfgpu.h
// "Solid meshes"); a mesh that is not closed is refused.
static const uint8_t MESH_FILL_SURFACE = 0x00;
static const uint8_t MESH_FILL_SOLID = 0x01;

class SDF_Builder {
public:
    using PlanningSceneSource = std::function<moveit_msgs::PlanningScene(uint8_t update_mode)>;

protected:
    bool initialized_;
    bool has_cached_sdf_;
    bool has_cached_collmap_;
    bool has_planning_scene_;
    Eigen::Isometry3d origin_transform_;
    std::string frame_;
    double x_size_;
    double y_size_;
    double z_size_;
    double resolution_;
    float OOB_value_;
    SignedDistanceField cached_sdf_;
    VoxelGrid::VoxelGrid<uint8_t> cached_collmap_;
    moveit_msgs::PlanningScene planning_scene_;
    PlanningSceneSource planning_scene_source_;
    uint8_t mesh_fill_ = MESH_FILL_SURFACE;
    std::map<std::string, uint8_t> object_mesh_fill_;      // CollisionObject::id -> mode, where it differs from mesh_fill_

    // a device allocation of the handle, freed on every way out (the caller holds the context's mutex)
    struct Scratch {
        sdfgpu_handle h;
        void* p = nullptr;
        Scratch(sdfgpu_handle handle, const size_t bytes) : h(handle) {
            sdf_generation::ThrowOnStatus(h, sdfgpu_device_malloc(h, bytes ? bytes : 256, &p));
        }
        ~Scratch() { if (p) (void)sdfgpu_device_free(h, p); }
        Scratch(const Scratch&) = delete;
        Scratch& operator=(const Scratch&) = delete;
    };

    void Origin16(double out[16]) const {
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) out[4 * r + c] = origin_transform_.matrix()(r, c);
    }

    static void Multiply(const double a[16], const double b[16], double out[16]) {
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) out[4 * i + j] = a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j] + a[4 * i + 2] * b[8 + j] + a[4 * i + 3] * b[12 + j];
    }

    // what the rasterisers take: the shape list, and the meshes with their shared vertex and triangle arrays
    struct SceneGeometry {
        std::vector<sdfgpu_shape> shapes;
        std::vector<sdfgpu_mesh> meshes;               // taken as their surface
        std::vector<sdfgpu_mesh> solid_meshes;         // filled inside as well; runs of the same two arrays
        std::vector<size_t> solid_objects;             // the collision object of each solid mesh
        bool HasMeshes() const { return !meshes.empty() || !solid_meshes.empty(); }
        std::vector<double> vertices;
        std::vector<uint32_t> triangles;
    };

    // The kept scene in list order: every collision object's primitives, then its planes (object id = its 1-based index), then the
    // octomap's boxes (one more id); every object's meshes beside them under the same id.  Refuses what the rasterisers do not
    // decide, before the GPU is touched.
    SceneGeometry SceneShapes() const {
        SceneGeometry scene;
        std::vector<sdfgpu_shape>& shapes = scene.shapes;
        const std::vector<moveit_msgs::CollisionObject>& objects = planning_scene_.world.collision_objects;
        for (size_t o = 0; o < objects.size(); ++o) {
            const moveit_msgs::CollisionObject& object = objects[o];
            if (object.meshes.size() != object.mesh_poses.size())
                throw std::invalid_argument("Collision object '" + object.id + "' has meshes without a pose each (" + std::to_string(object.meshes.size()) +
                                            " meshes, " + std::to_string(object.mesh_poses.size()) + " mesh poses)");
            if (object.planes.size() != object.plane_poses.size())
                throw std::invalid_argument("Collision object '" + object.id + "' has planes without a pose each (" + std::to_string(object.planes.size()) +
                                            " planes, " + std::to_string(object.plane_poses.size()) + " plane poses)");
            if (object.primitives.size() != object.primitive_poses.size())
                throw std::invalid_argument("Collision object '" + object.id + "' has a different number of primitives and primitive poses");
            for (size_t k = 0; k < object.primitives.size(); ++k) {
                const shape_msgs::SolidPrimitive& primitive = object.primitives[k];
                sdfgpu_shape s = sdfgpu_shape();
                size_t wanted = 0;
                if (primitive.type == shape_msgs::SolidPrimitive::BOX) { s.type = SDFGPU_SHAPE_BOX; wanted = 3; }
                else if (primitive.type == shape_msgs::SolidPrimitive::SPHERE) { s.type = SDFGPU_SHAPE_SPHERE; wanted = 1; }
                else if (primitive.type == shape_msgs::SolidPrimitive::CYLINDER) { s.type = SDFGPU_SHAPE_CYLINDER; wanted = 2; }
                else if (primitive.type == shape_msgs::SolidPrimitive::CONE)
                    throw std::invalid_argument("Collision object '" + object.id + "' has a cone (only boxes, spheres and cylinders are rasterised)");
                else throw std::invalid_argument("Collision object '" + object.id + "' has a primitive of unknown type");
                if (primitive.dimensions.size() < wanted) throw std::invalid_argument("Collision object '" + object.id + "' has a primitive with too few dimensions");
                for (size_t d = 0; d < wanted; ++d) {
                    if (!(std::isfinite(primitive.dimensions[d]) && primitive.dimensions[d] >= 0.0))
                        throw std::invalid_argument("Collision object '" + object.id + "' has a primitive with a negative or non-finite dimension");
                    s.dims[d] = primitive.dimensions[d];
                }
                s.object_id = (uint32_t)(o + 1);
                PoseToMatrix(object.primitive_poses[k], s.pose);
                for (int i = 0; i < 12; ++i)
                    if (!std::isfinite(s.pose[i])) throw std::invalid_argument("Collision object '" + object.id + "' has a primitive pose that is not finite");
                shapes.push_back(s);
            }
            // a plane a x + b y + c z + d = 0 of the pose's frame: through p0 = (-d / (a^2 + b^2 + c^2)) (a, b, c), normal (a, b, c)
            for (size_t k = 0; k < object.planes.size(); ++k) {
                const double* coef = object.planes[k].coef;
                const double nn = coef[0] * coef[0] + coef[1] * coef[1] + coef[2] * coef[2];
                const double scale = -coef[3] / nn;
                if (!(std::isfinite(coef[0]) && std::isfinite(coef[1]) && std::isfinite(coef[2]) && nn > 0.0 && std::isfinite(scale) &&
                      std::isfinite(scale * coef[0]) && std::isfinite(scale * coef[1]) && std::isfinite(scale * coef[2])))
                    throw std::invalid_argument("Collision object '" + object.id + "' has a plane with a zero or non-finite normal");
                sdfgpu_shape s = sdfgpu_shape();
                s.type = SDFGPU_SHAPE_PLANE;
                s.object_id = (uint32_t)(o + 1);
                for (int d = 0; d < 3; ++d) s.dims[d] = coef[d];
                double frame[16];
                PoseToMatrix(object.plane_poses[k], frame);
                const double local[16] = {1.0, 0.0, 0.0, scale * coef[0], 0.0, 1.0, 0.0, scale * coef[1], 0.0, 0.0, 1.0, scale * coef[2], 0.0, 0.0, 0.0, 1.0};
                Multiply(frame, local, s.pose);
                for (int i = 0; i < 12; ++i)
                    if (!std::isfinite(s.pose[i])) throw std::invalid_argument("Collision object '" + object.id + "' has a plane pose that is not finite");
                shapes.push_back(s);
            }
            for (size_t k = 0; k < object.meshes.size(); ++k) {
                const shape_msgs::Mesh& mesh = object.meshes[k];
                sdfgpu_mesh m = sdfgpu_mesh();
                m.object_id = (uint32_t)(o + 1);
                m.first_triangle = (int64_t)(scene.triangles.size() / 3);
                m.n_triangles = (int64_t)mesh.triangles.size();
                m.first_vertex = (int64_t)(scene.vertices.size() / 3);
                m.n_vertices = (int64_t)mesh.vertices.size();
                PoseToMatrix(object.mesh_poses[k], m.pose);
                for (int i = 0; i < 12; ++i)
                    if (!std::isfinite(m.pose[i])) throw std::invalid_argument("Collision object '" + object.id + "' has a mesh pose that is not finite");
                for (const geometry_msgs::Point& v : mesh.vertices) {
                    if (!(std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z)))
                        throw std::invalid_argument("Collision object '" + object.id + "' has a mesh with a vertex that is not finite");
                    scene.vertices.push_back(v.x); scene.vertices.push_back(v.y); scene.vertices.push_back(v.z);
                }
                for (const shape_msgs::MeshTriangle& t : mesh.triangles)
                    for (int i = 0; i < 3; ++i) {
                        if ((size_t)t.vertex_indices[i] >= mesh.vertices.size())
                            throw std::invalid_argument("Collision object '" + object.id + "' has a mesh with a vertex index out of range");
                        scene.triangles.push_back(t.vertex_indices[i]);
                    }
                const std::map<std::string, uint8_t>::const_iterator own = object_mesh_fill_.find(object.id);
                if ((own == object_mesh_fill_.end() ? mesh_fill_ : own->second) == MESH_FILL_SOLID) {
                    scene.solid_meshes.push_back(m);
                    scene.solid_objects.push_back(o);
                } else {
                    scene.meshes.push_back(m);
                }
                if ((int64_t)(scene.meshes.size() + scene.solid_meshes.size()) > (int64_t)SDFGPU_MAX_MESHES)
                    throw std::invalid_argument("The planning scene has more than " + std::to_string(SDFGPU_MAX_MESHES) + " meshes, the rasteriser takes no more");
                if ((int64_t)(scene.triangles.size() / 3) > (int64_t)SDFGPU_MAX_TRIANGLES)
                    throw std::invalid_argument("The planning scene has more than " + std::to_string(SDFGPU_MAX_TRIANGLES) + " triangles, the rasteriser takes no more");
            }
        }
        const octomap_msgs::OctomapBoxesWithPose& octomap = planning_scene_.world.octomap;
        if (octomap.octomap.centers.size() != octomap.octomap.sizes.size()) throw std::invalid_argument("The octomap has a different number of centers and sizes");
        double frame[16];
        PoseToMatrix(octomap.origin, frame);
        for (size_t k = 0; k < octomap.octomap.centers.size(); ++k) {
            const double size = octomap.octomap.sizes[k];
            const geometry_msgs::Point& c = octomap.octomap.centers[k];
            if (!(std::isfinite(size) && size >= 0.0 && std::isfinite(c.x) && std::isfinite(c.y) && std::isfinite(c.z)))
                throw std::invalid_argument("The octomap has a box that is negative or not finite");
            sdfgpu_shape s = sdfgpu_shape();
            s.type = SDFGPU_SHAPE_BOX;
            s.object_id = (uint32_t)(objects.size() + 1);
            s.dims[0] = s.dims[1] = s.dims[2] = size;
            const double local[16] = {1.0, 0.0, 0.0, c.x, 0.0, 1.0, 0.0, c.y, 0.0, 0.0, 1.0, c.z, 0.0, 0.0, 0.0, 1.0};
            Multiply(frame, local, s.pose);
            shapes.push_back(s);
        }
        if ((int64_t)shapes.size() > (int64_t)SDFGPU_MAX_SHAPES)
            throw std::invalid_argument("The planning scene has " + std::to_string(shapes.size()) + " shapes, the rasteriser takes " + std::to_string(SDFGPU_MAX_SHAPES));
        if (!scene.solid_meshes.empty()) {                 // on the host, no GPU: an even number of triangles on every edge
            int64_t bad_mesh = -1, bad_triangle = -1;
            if (sdfgpu_check_closed_meshes(scene.solid_meshes.data(), (int64_t)scene.solid_meshes.size(), scene.vertices.data(),
                                           (int64_t)(scene.vertices.size() / 3), scene.triangles.data(), (int64_t)(scene.triangles.size() / 3), &bad_mesh,
                                           &bad_triangle) != SDFGPU_OK)
                throw std::invalid_argument("Collision object '" + (bad_mesh >= 0 ? objects[scene.solid_objects[(size_t)bad_mesh]].id : std::string("?")) +
                                            "' has a mesh that is to be filled as a solid but is not closed (an edge of its triangle " +
                                            std::to_string(bad_triangle) + " is used by an odd number of triangles)");
        }
        return scene;
    }

    // scene -> device, rasterised on the null stream of the context into whichever of the three outputs is given: the shape list
    // first, then the surface meshes, then the solid meshes (at most SDFGPU_MAX_SOLID_MESHES a call), each accumulated onto the same
    // outputs (a scene without meshes enqueues the shape rasteriser alone, one without solid meshes what it always did).  Nothing
    // is waited for; the scratch is freed when this returns (hipFree waits for the device, so the work enqueued here has finished by
    // then).  The caller holds the context's mutex.
    void RasterizeOnDevice(sdfgpu_handle h, const SceneGeometry& scene, const int64_t nx, const int64_t ny, const int64_t nz, uint32_t* d_bits, uint8_t* d_mask,
                           uint32_t* d_ids) const {
        double origin[16];
        Origin16(origin);
        const std::vector<sdfgpu_shape>& shapes = scene.shapes;
        Scratch d_shapes(h, shapes.size() * sizeof(sdfgpu_shape));
        if (!shapes.empty())
            sdf_generation::ThrowOnStatus(h, sdfgpu_copy_from_host(h, d_shapes.p, shapes.data(), shapes.size() * sizeof(sdfgpu_shape), nullptr));
        sdf_generation::ThrowOnStatus(h, sdfgpu_rasterize_shapes_device(h, shapes.empty() ? nullptr : static_cast<const sdfgpu_shape*>(d_shapes.p),
                                                                        (int64_t)shapes.size(), origin, resolution_, nx, ny, nz, d_bits, d_mask, d_ids, nullptr,
                                                                        nullptr));
        if (!scene.HasMeshes()) return;
        // (the record buffers of the kind of mesh the scene does not have are not allocated: a scene of surface meshes alone
        // allocates, enqueues and frees what it always did)
        std::unique_ptr<Scratch> d_meshes, d_solid;
        if (!scene.meshes.empty()) d_meshes.reset(new Scratch(h, scene.meshes.size() * sizeof(sdfgpu_mesh)));
        Scratch d_vertices(h, scene.vertices.size() * sizeof(double));
        Scratch d_triangles(h, scene.triangles.size() * sizeof(uint32_t));
        if (!scene.vertices.empty())
            sdf_generation::ThrowOnStatus(h, sdfgpu_copy_from_host(h, d_vertices.p, scene.vertices.data(), scene.vertices.size() * sizeof(double), nullptr));
        if (!scene.triangles.empty())
            sdf_generation::ThrowOnStatus(h, sdfgpu_copy_from_host(h, d_triangles.p, scene.triangles.data(), scene.triangles.size() * sizeof(uint32_t), nullptr));
        if (!scene.meshes.empty()) {
            sdf_generation::ThrowOnStatus(h, sdfgpu_copy_from_host(h, d_meshes->p, scene.meshes.data(), scene.meshes.size() * sizeof(sdfgpu_mesh), nullptr));
            sdf_generation::ThrowOnStatus(h, sdfgpu_rasterize_meshes_device(h, static_cast<const sdfgpu_mesh*>(d_meshes->p), (int64_t)scene.meshes.size(),
                                                                            static_cast<const double*>(d_vertices.p), (int64_t)(scene.vertices.size() / 3),
                                                                            static_cast<const uint32_t*>(d_triangles.p), (int64_t)(scene.triangles.size() / 3), origin,
                                                                            resolution_, nx, ny, nz, d_bits, d_mask, d_ids, 1, nullptr, nullptr));
        }
        if (scene.solid_meshes.empty()) return;
        d_solid.reset(new Scratch(h, scene.solid_meshes.size() * sizeof(sdfgpu_mesh)));
        sdf_generation::ThrowOnStatus(h, sdfgpu_copy_from_host(h, d_solid->p, scene.solid_meshes.data(), scene.solid_meshes.size() * sizeof(sdfgpu_mesh), nullptr));
        for (size_t first = 0; first < scene.solid_meshes.size(); first += (size_t)SDFGPU_MAX_SOLID_MESHES) {
            const size_t count = std::min(scene.solid_meshes.size() - first, (size_t)SDFGPU_MAX_SOLID_MESHES);
            sdf_generation::ThrowOnStatus(h, sdfgpu_rasterize_solid_meshes_device(h, static_cast<const sdfgpu_mesh*>(d_solid->p) + first, (int64_t)count,
                                                                                  static_cast<const double*>(d_vertices.p), (int64_t)(scene.vertices.size() / 3),
                                                                                  static_cast<const uint32_t*>(d_triangles.p), (int64_t)(scene.triangles.size() / 3),
                                                                                  origin, resolution_, nx, ny, nz, d_bits, d_mask, d_ids, 1, nullptr, nullptr));
        }
    }

    // the reference's UpdateSDF / UpdateCollisionMap preamble: the exceptions, and the scene the mode asks for
    void PrepareScene(const uint8_t update_mode) {
        if (!initialized_) throw std::invalid_argument("SDF Builder has not been initialized");
        if (update_mode == USE_CACHED) {
            if (!has_planning_scene_) throw std::invalid_argument("No planning scene available");
            return;
        }
        if (update_mode != USE_ONLY_COLLISION_OBJECTS && update_mode != USE_ONLY_OCTOMAP && update_mode != USE_FULL_PLANNING_SCENE)
            throw std::invalid_argument("Invalid update mode (mode not recognized)");
        if (!planning_scene_source_) throw std::invalid_argument("No planning scene available");
        moveit_msgs::PlanningScene scene = planning_scene_source_(update_mode);
        if (update_mode == USE_ONLY_COLLISION_OBJECTS) scene.world.octomap = octomap_msgs::OctomapBoxesWithPose();
        if (update_mode == USE_ONLY_OCTOMAP) scene.world.collision_objects.clear();
        planning_scene_ = std::move(scene);
        has_planning_scene_ = true;
    }

    // scene -> the bit field (shapes, then meshes onto the same bits), the SDF built from it in place (virtual border off, as in the
    // reference): all on the null stream of the context, nothing waited for.  The caller holds the context's mutex.
    void BuildOnDevice(sdfgpu_handle h, const SceneGeometry& scene, const VoxelGrid::VoxelGrid<uint8_t>& geometry, float* d_sdf) const {
        const int64_t nx = geometry.GetNumXCells(), ny = geometry.GetNumYCells(), nz = geometry.GetNumZCells();
        Scratch d_bits(h, (size_t)((nx * ny * nz + 31) / 32) * 4);
        RasterizeOnDevice(h, scene, nx, ny, nz, static_cast<uint32_t*>(d_bits.p), nullptr, nullptr);
        sdf_generation::ThrowOnStatus(h, sdfgpu_build_bits_device(h, static_cast<const uint32_t*>(d_bits.p), nx, ny, nz, resolution_, 0, d_sdf, nullptr));
        // (the scratch is freed when this returns: hipFree waits for the device, so the work enqueued above has finished by then)
    }

    SignedDistanceField UpdateSDFFromPlanningScene() {
        const SceneGeometry shapes = SceneShapes();                             // (refusals come before the GPU is touched)
        const VoxelGrid::VoxelGrid<uint8_t> temp_grid(origin_transform_, resolution_, x_size_, y_size_, z_size_, 0);
        const int64_t nx = temp_grid.GetNumXCells(), ny = temp_grid.GetNumYCells(), nz = temp_grid.GetNumZCells();
        SignedDistanceField new_sdf(SignedDistanceField::ForBuild{}, origin_transform_, frame_, resolution_, nx, ny, nz, OOB_value_);
        {
            const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
            const std::lock_guard<std::mutex> lock(ctx->mutex);
            sdfgpu_handle h = ctx->handle;
            Scratch d_sdf(h, (size_t)(nx * ny * nz) * sizeof(float));
            BuildOnDevice(h, shapes, temp_grid, static_cast<float*>(d_sdf.p));
            sdf_generation::ThrowOnStatus(h, sdfgpu_copy_to_host(h, new_sdf.MutableDataForBuild(), d_sdf.p, (size_t)(nx * ny * nz) * sizeof(float), nullptr));
        }
        cached_sdf_ = new_sdf;
        has_cached_sdf_ = true;
        return new_sdf;
    }

    VoxelGrid::VoxelGrid<uint8_t> UpdateCollisionMapFromPlanningScene() {
        VoxelGrid::VoxelGrid<uint8_t> collision_field(origin_transform_, resolution_, x_size_, y_size_, z_size_, 0);
        const SceneGeometry scene = SceneShapes();
        const std::vector<sdfgpu_shape>& shapes = scene.shapes;
        const int64_t nx = collision_field.GetNumXCells(), ny = collision_field.GetNumYCells(), nz = collision_field.GetNumZCells();
        double origin[16];
        Origin16(origin);
        {
            const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
            const std::lock_guard<std::mutex> lock(ctx->mutex);
            sdfgpu_handle h = ctx->handle;
            if (!scene.HasMeshes()) {
                sdf_generation::ThrowOnStatus(h, sdfgpu_rasterize_shapes(h, shapes.empty() ? nullptr : shapes.data(), (int64_t)shapes.size(), origin, resolution_, nx,
                                                                         ny, nz, nullptr, collision_field.GetMutableRawData().data(), nullptr));
            } else {                                                            // shapes, then meshes onto the same mask; one download
                Scratch d_mask(h, (size_t)(nx * ny * nz));
                RasterizeOnDevice(h, scene, nx, ny, nz, nullptr, static_cast<uint8_t*>(d_mask.p), nullptr);
                sdf_generation::ThrowOnStatus(h, sdfgpu_copy_to_host(h, collision_field.GetMutableRawData().data(), d_mask.p, (size_t)(nx * ny * nz), nullptr));
            }
        }
        cached_collmap_ = collision_field;
        has_cached_collmap_ = true;
        return collision_field;
    }

public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW

    SDF_Builder(const Eigen::Isometry3d& origin_transform, const std::string& frame, const double x_size, const double y_size, const double z_size,
                const double resolution, const float OOB_value, const PlanningSceneSource& planning_scene_source = PlanningSceneSource())
        : initialized_(true), has_cached_sdf_(false), has_cached_collmap_(false), has_planning_scene_(false), origin_transform_(origin_transform),
          frame_(frame), x_size_(x_size), y_size_(y_size), z_size_(z_size), resolution_(resolution), OOB_value_(OOB_value),
          planning_scene_source_(planning_scene_source) {}

    // the grid centred on the frame's origin, as the reference's second constructor places it
    SDF_Builder(const std::string& frame, const double x_size, const double y_size, const double z_size, const double resolution, const float OOB_value,
                const PlanningSceneSource& planning_scene_source = PlanningSceneSource())
        : initialized_(true), has_cached_sdf_(false), has_cached_collmap_(false), has_planning_scene_(false), frame_(frame), x_size_(x_size),
          y_size_(y_size), z_size_(z_size), resolution_(resolution), OOB_value_(OOB_value), planning_scene_source_(planning_scene_source) {
        origin_transform_.setTranslation(-x_size * 0.5, -y_size * 0.5, -z_size * 0.5);
    }

    SDF_Builder()
        : initialized_(false), has_cached_sdf_(false), has_cached_collmap_(false), has_planning_scene_(false), x_size_(0.0), y_size_(0.0), z_size_(0.0),
          resolution_(0.0), OOB_value_(0.0f) {}

    void UpdatePlanningSceneFromMessage(const moveit_msgs::PlanningScene& planning_scene) {
        planning_scene_ = planning_scene;
        has_planning_scene_ = true;
    }

    SignedDistanceField UpdateSDF(const uint8_t update_mode) {
        PrepareScene(update_mode);
        return UpdateSDFFromPlanningScene();
    }

    // How meshes are filled from the next update on: MESH_FILL_SURFACE (the default) or MESH_FILL_SOLID; per collision object
    // (CollisionObject::id) with SetObjectMeshFill, which overrides the builder's mode for that object.
    void SetMeshFill(const uint8_t mode) {
        if (mode != MESH_FILL_SURFACE && mode != MESH_FILL_SOLID) throw std::invalid_argument("Invalid mesh fill mode (mode not recognized)");
        mesh_fill_ = mode;
    }

    void SetObjectMeshFill(const std::string& object_id, const uint8_t mode) {
        if (mode != MESH_FILL_SURFACE && mode != MESH_FILL_SOLID) throw std::invalid_argument("Invalid mesh fill mode (mode not recognized)");
        object_mesh_fill_[object_id] = mode;
    }

    const SignedDistanceField& GetCachedSDF() const {
        if (has_cached_sdf_) return cached_sdf_;
        throw std::invalid_argument("No cached SDF available");
    }

    VoxelGrid::VoxelGrid<uint8_t> UpdateCollisionMap(const uint8_t update_mode) {
        PrepareScene(update_mode);
        return UpdateCollisionMapFromPlanningScene();
    }

    const VoxelGrid::VoxelGrid<uint8_t>& GetCachedCollisionMap() const {
        if (has_cached_collmap_) return cached_collmap_;
        throw std::invalid_argument("No cached Collision Map available");
    }

    // ---- extensions (no counterpart in the reference) ----------------------------------------------------------------------------------
    // UpdateSDF whose result stays in HBM (batched queries, projections and gradients run there; Host() downloads it if asked).  The
    // cached SDF is not touched.
    DeviceSignedDistanceField UpdateSDFDevice(const uint8_t update_mode) {
        PrepareScene(update_mode);
        const SceneGeometry shapes = SceneShapes();
        const VoxelGrid::VoxelGrid<uint8_t> temp_grid(origin_transform_, resolution_, x_size_, y_size_, z_size_, 0);
        DeviceSignedDistanceField new_sdf(origin_transform_, frame_, resolution_, temp_grid.GetNumXCells(), temp_grid.GetNumYCells(),
                                          temp_grid.GetNumZCells(), OOB_value_);
        const std::lock_guard<std::mutex> lock(new_sdf.Context()->mutex);
        BuildOnDevice(new_sdf.Handle(), shapes, temp_grid, new_sdf.DevicePointer());
        double max_distance = 0.0, min_distance = 0.0;
        sdf_generation::ThrowOnStatus(new_sdf.Handle(), sdfgpu_get_extrema(new_sdf.Handle(), &max_distance, &min_distance));
        new_sdf.SetExtrema(std::make_pair(max_distance, min_distance));
        return new_sdf;
    }

    // The collision map with object ids: a filled cell (occupancy 1) carries the id of the first shape in scene order that its probe
    // meets -- the 1-based index of the collision object, or the number of collision objects + 1 for the octomap; empty cells carry
    // occupancy 0 and id 0.  With meshes it is the smallest id among the shapes and meshes the probe meets, which is the same thing:
    // ids ascend with scene order.
    TaggedObjectCollisionMapGrid UpdateTaggedCollisionMap(const uint8_t update_mode) {
        PrepareScene(update_mode);
        TaggedObjectCollisionMapGrid map(origin_transform_, frame_, resolution_, x_size_, y_size_, z_size_, TAGGED_OBJECT_COLLISION_CELL());
        const SceneGeometry scene = SceneShapes();
        const std::vector<sdfgpu_shape>& shapes = scene.shapes;
        const int64_t nx = map.GetNumXCells(), ny = map.GetNumYCells(), nz = map.GetNumZCells();
        std::vector<uint32_t> ids((size_t)(nx * ny * nz));
        double origin[16];
        Origin16(origin);
        {
            const std::shared_ptr<sdf_generation::SharedGpuContext> ctx = sdf_generation::GpuContext::Shared();
            const std::lock_guard<std::mutex> lock(ctx->mutex);
            sdfgpu_handle h = ctx->handle;
            if (!scene.HasMeshes()) {
                sdf_generation::ThrowOnStatus(h, sdfgpu_rasterize_shapes(h, shapes.empty() ? nullptr : shapes.data(), (int64_t)shapes.size(), origin, resolution_, nx,
                                                                         ny, nz, nullptr, nullptr, ids.data()));
            } else {
                Scratch d_ids(h, ids.size() * sizeof(uint32_t));
                RasterizeOnDevice(h, scene, nx, ny, nz, nullptr, nullptr, static_cast<uint32_t*>(d_ids.p));
                sdf_generation::ThrowOnStatus(h, sdfgpu_copy_to_host(h, ids.data(), d_ids.p, ids.size() * sizeof(uint32_t), nullptr));
            }
        }
        std::vector<TAGGED_OBJECT_COLLISION_CELL>& cells = map.GetMutableRawData();
        for (size_t i = 0; i < ids.size(); ++i)
            if (ids[i] != 0u) cells[i] = TAGGED_OBJECT_COLLISION_CELL(1.0f, ids[i]);
        return map;
    }
};

}  // namespace sdf_tools
