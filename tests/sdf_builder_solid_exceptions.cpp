// SDF_Builder's refusals under MESH_FILL_SOLID (include/sdf_tools/sdf_builder.hpp): an open mesh that is to be filled as a solid is a
// std::invalid_argument naming the object, thrown before the GPU is touched, so this runs without one.  tests/test_mesh_solid_cpu.py
// builds and runs it, once more under the sanitizers; it prints one line per check and returns the number of failures.
#include <functional>
#include <iostream>
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

// a tetrahedron; `triangles` of its four faces
static shape_msgs::Mesh Tetrahedron(int triangles) {
    shape_msgs::Mesh mesh;
    mesh.vertices.resize(4);
    mesh.vertices[1].x = 0.3; mesh.vertices[2].y = 0.3; mesh.vertices[3].z = 0.3;
    const uint32_t faces[4][3] = {{0, 2, 1}, {0, 1, 3}, {0, 3, 2}, {1, 2, 3}};
    for (int f = 0; f < triangles; ++f) {
        shape_msgs::MeshTriangle t;
        for (int i = 0; i < 3; ++i) t.vertex_indices[i] = faces[f][i];
        mesh.triangles.push_back(t);
    }
    return mesh;
}

int main() {
    using namespace sdf_tools;
    SDF_Builder builder("world", 1.0, 1.0, 1.0, 0.1, 100.0f);
    geometry_msgs::Pose identity;
    identity.orientation.w = 1.0;
    moveit_msgs::PlanningScene scene;
    moveit_msgs::CollisionObject closed, open;
    closed.id = "closed thing";
    closed.meshes = {Tetrahedron(4)};
    closed.mesh_poses = {identity};
    open.id = "open thing";
    open.meshes = {Tetrahedron(4), Tetrahedron(3)};
    open.mesh_poses = {identity, identity};
    scene.world.collision_objects = {closed, open};
    builder.UpdatePlanningSceneFromMessage(scene);

    Expect("an unknown mode", [&] { builder.SetMeshFill(2); }, "Invalid mesh fill mode");
    Expect("an unknown mode for an object", [&] { builder.SetObjectMeshFill("open thing", 7); }, "Invalid mesh fill mode");
    builder.SetMeshFill(MESH_FILL_SOLID);
    const std::string text = "Collision object 'open thing' has a mesh that is to be filled as a solid but is not closed (an edge of its triangle 0";
    Expect("an open mesh under SOLID", [&] { builder.UpdateSDF(USE_CACHED); }, text);
    Expect("the same through the collision map", [&] { builder.UpdateCollisionMap(USE_CACHED); }, text);
    Expect("the same through the tagged map", [&] { builder.UpdateTaggedCollisionMap(USE_CACHED); }, text);
    Expect("the same through the device SDF", [&] { builder.UpdateSDFDevice(USE_CACHED); }, text);
    builder.SetMeshFill(MESH_FILL_SURFACE);
    builder.SetObjectMeshFill("open thing", MESH_FILL_SOLID);
    Expect("an open mesh of an object set to SOLID", [&] { builder.UpdateSDF(USE_CACHED); }, text);
    std::cout << failures << " failures" << std::endl;
    return failures;
}
