// SDF_Builder's exceptions (include/sdf_tools/sdf_builder.hpp), the reference's texts (src/sdf_tools/sdf_builder.cpp:119-279) and the
// refusals of what the rasteriser does not decide: every one is thrown before the GPU is touched, so this runs without one.
// tests/test_scene_raster_cpu.py builds and runs it; it prints one line per check and returns the number of failures.
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

int main() {
    using namespace sdf_tools;
    SDF_Builder empty;
    Expect("default-constructed UpdateSDF", [&] { empty.UpdateSDF(USE_CACHED); }, "SDF Builder has not been initialized");
    Expect("default-constructed UpdateCollisionMap", [&] { empty.UpdateCollisionMap(USE_FULL_PLANNING_SCENE); }, "SDF Builder has not been initialized");
    SDF_Builder plain("world", 1.0, 1.0, 1.0, 0.1, 100.0f);
    Expect("cached mode without a scene", [&] { plain.UpdateSDF(USE_CACHED); }, "No planning scene available");
    Expect("collision map, cached mode without a scene", [&] { plain.UpdateCollisionMap(USE_CACHED); }, "No planning scene available");
    for (const uint8_t mode : {USE_ONLY_OCTOMAP, USE_ONLY_COLLISION_OBJECTS, USE_FULL_PLANNING_SCENE}) {
        Expect("a fetching mode without a source", [&] { plain.UpdateSDF(mode); }, "No planning scene available");
        Expect("collision map, a fetching mode without a source", [&] { plain.UpdateCollisionMap(mode); }, "No planning scene available");
    }
    Expect("an unknown mode", [&] { plain.UpdateSDF(0x04); }, "Invalid update mode (mode not recognized)");
    Expect("collision map, an unknown mode", [&] { plain.UpdateCollisionMap(0x7f); }, "Invalid update mode (mode not recognized)");
    Expect("no cached SDF", [&] { plain.GetCachedSDF(); }, "No cached SDF available");
    Expect("no cached collision map", [&] { plain.GetCachedCollisionMap(); }, "No cached Collision Map available");

    moveit_msgs::PlanningScene scene;
    moveit_msgs::CollisionObject object;
    object.id = "thing";
    object.primitives.resize(1);
    object.primitive_poses.resize(1);
    object.primitive_poses[0].orientation.w = 1.0;
    object.primitives[0].type = shape_msgs::SolidPrimitive::CONE;
    object.primitives[0].dimensions = {0.2, 0.1};
    scene.world.collision_objects.push_back(object);
    plain.UpdatePlanningSceneFromMessage(scene);
    Expect("a cone", [&] { plain.UpdateCollisionMap(USE_CACHED); }, "'thing' has a cone");
    Expect("a cone, SDF", [&] { plain.UpdateSDF(USE_CACHED); }, "'thing' has a cone");
    scene.world.collision_objects[0].primitives[0].type = shape_msgs::SolidPrimitive::SPHERE;
    scene.world.collision_objects[0].primitives[0].dimensions = {-0.2};
    plain.UpdatePlanningSceneFromMessage(scene);
    Expect("a negative radius", [&] { plain.UpdateCollisionMap(USE_CACHED); }, "negative or non-finite dimension");
    scene.world.collision_objects[0].primitives[0].dimensions = {};
    plain.UpdatePlanningSceneFromMessage(scene);
    Expect("a sphere without a radius", [&] { plain.UpdateCollisionMap(USE_CACHED); }, "too few dimensions");
    scene.world.collision_objects[0].primitives[0].dimensions = {0.2};
    scene.world.collision_objects[0].meshes.resize(1);
    plain.UpdatePlanningSceneFromMessage(scene);
    Expect("a mesh", [&] { plain.UpdateCollisionMap(USE_CACHED); }, "'thing' has meshes");
    scene.world.collision_objects[0].meshes.clear();
    scene.world.collision_objects[0].planes.resize(1);
    plain.UpdatePlanningSceneFromMessage(scene);
    Expect("a plane", [&] { plain.UpdateTaggedCollisionMap(USE_CACHED); }, "'thing' has planes");
    scene.world.collision_objects[0].planes.clear();
    scene.world.collision_objects[0].primitive_poses.clear();
    plain.UpdatePlanningSceneFromMessage(scene);
    Expect("a primitive without a pose", [&] { plain.UpdateSDFDevice(USE_CACHED); }, "different number of primitives and primitive poses");
    // the source is called with the mode, and its exception passes through
    SDF_Builder fetching("world", 1.0, 1.0, 1.0, 0.1, 100.0f, [](uint8_t mode) -> moveit_msgs::PlanningScene {
        throw std::invalid_argument("source called with mode " + std::to_string((int)mode));
    });
    Expect("the source sees the mode", [&] { fetching.UpdateSDF(USE_ONLY_OCTOMAP); }, "source called with mode 1");
    Expect("the source sees the mode (full)", [&] { fetching.UpdateCollisionMap(USE_FULL_PLANNING_SCENE); }, "source called with mode 3");
    std::cout << failures << " failures" << std::endl;
    return failures;
}
