// SDF_Builder's refusals of meshes and planes (include/sdf_tools/sdf_builder.hpp): every one is a std::invalid_argument thrown before
// the GPU is touched, so this runs without one.  tests/test_mesh_raster_cpu.py builds and runs it, once more under the sanitizers;
// it prints one line per check and returns the number of failures.
#include <cmath>
#include <functional>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>

#include "sdf_tools/sdf_builder.hpp"

static int failures = 0;

static void Expect(const char* what, const std::function<void()>& call, const std::string& text) {
    try {
        call();
        std::cout << "FAIL " << what << ": nothing thrown" << std::endl;
        ++failures;
    } catch (const std::invalid_argument& e) {
        const bool ok = std::string(e.what()).find(text) != std::string::npos;
        std::cout << (ok ? "ok   " : "FAIL ") << what << ": " << e.what() << std::endl;
        if (!ok) ++failures;
    } catch (const std::exception& e) {
        std::cout << "FAIL " << what << ": another exception: " << e.what() << std::endl;
        ++failures;
    }
}

static shape_msgs::Mesh Triangle() {
    shape_msgs::Mesh mesh;
    mesh.vertices.resize(3);
    mesh.vertices[1].x = 0.2;
    mesh.vertices[2].y = 0.2;
    shape_msgs::MeshTriangle t;
    t.vertex_indices[1] = 1; t.vertex_indices[2] = 2;
    mesh.triangles.push_back(t);
    return mesh;
}

int main() {
    using namespace sdf_tools;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    SDF_Builder builder("world", 1.0, 1.0, 1.0, 0.1, 100.0f);
    geometry_msgs::Pose identity;
    identity.orientation.w = 1.0;
    const auto with = [&](const std::function<void(moveit_msgs::CollisionObject&)>& change) {
        moveit_msgs::PlanningScene scene;
        moveit_msgs::CollisionObject object;
        object.id = "thing";
        change(object);
        scene.world.collision_objects.push_back(object);
        builder.UpdatePlanningSceneFromMessage(scene);
    };

    with([&](moveit_msgs::CollisionObject& o) { o.meshes = {Triangle(), Triangle()}; o.mesh_poses = {identity}; });
    Expect("meshes without a pose each", [&] { builder.UpdateSDF(USE_CACHED); }, "Collision object 'thing' has meshes without a pose each (2 meshes, 1 mesh poses)");
    Expect("the same through the collision map", [&] { builder.UpdateCollisionMap(USE_CACHED); }, "'thing' has meshes");
    with([&](moveit_msgs::CollisionObject& o) { o.planes.resize(1); o.planes[0].coef[2] = 1.0; });
    Expect("planes without a pose each", [&] { builder.UpdateTaggedCollisionMap(USE_CACHED); }, "Collision object 'thing' has planes without a pose each (1 planes, 0 plane poses)");
    with([&](moveit_msgs::CollisionObject& o) { o.meshes = {Triangle()}; o.mesh_poses = {identity}; o.meshes[0].triangles[0].vertex_indices[2] = 3; });
    Expect("a vertex index out of range", [&] { builder.UpdateSDF(USE_CACHED); }, "'thing' has a mesh with a vertex index out of range");
    Expect("the same through the device SDF", [&] { builder.UpdateSDFDevice(USE_CACHED); }, "'thing' has a mesh with a vertex index out of range");
    with([&](moveit_msgs::CollisionObject& o) { o.meshes = {Triangle()}; o.mesh_poses = {identity}; o.meshes[0].vertices[1].z = nan; });
    Expect("a NaN vertex", [&] { builder.UpdateCollisionMap(USE_CACHED); }, "'thing' has a mesh with a vertex that is not finite");
    with([&](moveit_msgs::CollisionObject& o) { o.meshes = {Triangle()}; o.mesh_poses = {identity}; o.meshes[0].vertices[0].x = -inf; });
    Expect("an infinite vertex", [&] { builder.UpdateCollisionMap(USE_CACHED); }, "'thing' has a mesh with a vertex that is not finite");
    with([&](moveit_msgs::CollisionObject& o) { o.meshes = {Triangle()}; o.mesh_poses = {identity}; o.mesh_poses[0].position.y = inf; });
    Expect("an infinite mesh pose", [&] { builder.UpdateSDF(USE_CACHED); }, "'thing' has a mesh pose that is not finite");
    with([&](moveit_msgs::CollisionObject& o) { o.meshes = {Triangle()}; o.mesh_poses = {identity}; o.mesh_poses[0].orientation.w = 0.0; });
    Expect("a zero quaternion on a mesh", [&] { builder.UpdateSDF(USE_CACHED); }, "'thing' has a mesh pose that is not finite");
    with([&](moveit_msgs::CollisionObject& o) { o.planes.resize(1); o.plane_poses = {identity}; o.planes[0].coef[3] = 1.0; });
    Expect("a zero normal", [&] { builder.UpdateCollisionMap(USE_CACHED); }, "'thing' has a plane with a zero or non-finite normal");
    with([&](moveit_msgs::CollisionObject& o) { o.planes.resize(1); o.plane_poses = {identity}; o.planes[0].coef[0] = nan; o.planes[0].coef[1] = 1.0; });
    Expect("a NaN normal", [&] { builder.UpdateCollisionMap(USE_CACHED); }, "'thing' has a plane with a zero or non-finite normal");
    with([&](moveit_msgs::CollisionObject& o) { o.planes.resize(1); o.plane_poses = {identity}; o.planes[0].coef[2] = 1.0; o.planes[0].coef[3] = inf; });
    Expect("an infinite offset", [&] { builder.UpdateCollisionMap(USE_CACHED); }, "'thing' has a plane with a zero or non-finite normal");
    with([&](moveit_msgs::CollisionObject& o) { o.planes.resize(1); o.plane_poses = {identity}; o.planes[0].coef[2] = 1.0; o.plane_poses[0].position.x = nan; });
    Expect("a NaN plane pose", [&] { builder.UpdateSDF(USE_CACHED); }, "'thing' has a plane pose that is not finite");
    // a cone is refused as before, also beside a mesh and a plane that are fine
    with([&](moveit_msgs::CollisionObject& o) {
        o.meshes = {Triangle()}; o.mesh_poses = {identity};
        o.planes.resize(1); o.plane_poses = {identity}; o.planes[0].coef[2] = 1.0;
        shape_msgs::SolidPrimitive cone;
        cone.type = shape_msgs::SolidPrimitive::CONE;
        cone.dimensions = {0.2, 0.1};
        o.primitives = {cone}; o.primitive_poses = {identity};
    });
    Expect("a cone", [&] { builder.UpdateSDF(USE_CACHED); }, "Collision object 'thing' has a cone (only boxes, spheres and cylinders are rasterised)");
    // the totals: more meshes than the rasteriser takes (empty ones count)
    {
        moveit_msgs::PlanningScene scene;
        moveit_msgs::CollisionObject object;
        object.id = "many";
        object.meshes.resize((size_t)SDFGPU_MAX_MESHES + 1);
        object.mesh_poses.assign(object.meshes.size(), identity);
        scene.world.collision_objects.push_back(object);
        builder.UpdatePlanningSceneFromMessage(scene);
        Expect("more meshes than the limit", [&] { builder.UpdateSDF(USE_CACHED); }, "more than 65536 meshes");
    }
    std::cout << failures << " failures" << std::endl;
    return failures;
}
