// sdf_builder -- a client of sdf_tools::SDF_Builder written as a reference client would write it: a planning scene with two collision
// objects and an octomap, a builder over a grid in a rotated frame, the collision map and the SDF in every update mode, the cached
// getters.  Usage: sdf_builder_example [output directory]
// With a directory, the results are written there as raw arrays (x -> y -> z order), for tests/test_gpu_sdf_builder.py:
//   collision_map_<mode>.u8, sdf_<mode>.f32 (mode: full, objects, octomap, cached), tagged_ids.u32, device_sdf.f32
// The scene's numbers are repeated in that test.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "sdf_tools/sdf_builder.hpp"

namespace {

geometry_msgs::Pose MakePose(double px, double py, double pz, double qw, double qx, double qy, double qz) {
    geometry_msgs::Pose pose;
    pose.position.x = px; pose.position.y = py; pose.position.z = pz;
    pose.orientation.w = qw; pose.orientation.x = qx; pose.orientation.y = qy; pose.orientation.z = qz;
    return pose;
}

shape_msgs::SolidPrimitive MakePrimitive(uint8_t type, std::vector<double> dimensions) {
    shape_msgs::SolidPrimitive primitive;
    primitive.type = type;
    primitive.dimensions = std::move(dimensions);
    return primitive;
}

moveit_msgs::PlanningScene MakeScene() {
    moveit_msgs::PlanningScene scene;
    scene.name = "example";
    moveit_msgs::CollisionObject table;
    table.id = "table";
    table.primitives.push_back(MakePrimitive(shape_msgs::SolidPrimitive::BOX, {0.9, 0.6, 0.1}));
    table.primitive_poses.push_back(MakePose(0.1, -0.05, -0.3, 0.9, 0.1, -0.2, 0.3));
    table.primitives.push_back(MakePrimitive(shape_msgs::SolidPrimitive::CYLINDER, {0.5, 0.06}));
    table.primitive_poses.push_back(MakePose(0.1, -0.05, -0.55, 0.9, 0.1, -0.2, 0.3));
    moveit_msgs::CollisionObject ball;
    ball.id = "ball";
    ball.primitives.push_back(MakePrimitive(shape_msgs::SolidPrimitive::SPHERE, {0.17}));
    ball.primitive_poses.push_back(MakePose(0.2, 0.1, -0.12, 1.0, 0.0, 0.0, 0.0));       // (it overlaps the table: the table's id wins there)
    scene.world.collision_objects = {table, ball};
    scene.world.octomap.origin = MakePose(-0.3, 0.2, 0.3, 0.8, -0.3, 0.1, 0.2);
    for (int i = 0; i < 40; ++i) {
        geometry_msgs::Point c;
        c.x = 0.05 * (i % 8); c.y = 0.05 * (i / 8); c.z = 0.1 * ((i * 7) % 3);
        scene.world.octomap.octomap.centers.push_back(c);
        scene.world.octomap.octomap.sizes.push_back(i % 5 == 0 ? 0.1 : 0.05);
    }
    return scene;
}

template <typename T>
void Write(const std::string& dir, const std::string& name, const T* data, size_t count) {
    if (dir.empty()) return;
    FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    if (!f || std::fwrite(data, sizeof(T), count, f) != count) throw std::runtime_error("cannot write " + name);
    std::fclose(f);
}

size_t Filled(const VoxelGrid::VoxelGrid<uint8_t>& map) {
    size_t filled = 0;
    for (const uint8_t v : map.GetImmutableRawData()) filled += v;
    return filled;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "";
    try {
        double origin16[16];
        sdf_tools::PoseToMatrix(MakePose(-0.37, -1.33, -0.02, 0.83, -0.21, 0.4, 0.32), origin16);
        Eigen::Matrix4d m;
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m(r, c) = origin16[4 * r + c];
        const Eigen::Isometry3d origin(m);
        int fetched = 0;
        sdf_tools::SDF_Builder builder(origin, "world", 1.6, 1.4, 1.8, 0.04, 1e6f, [&](uint8_t) { ++fetched; return MakeScene(); });

        const struct { uint8_t mode; const char* name; } modes[] = {{sdf_tools::USE_FULL_PLANNING_SCENE, "full"}, {sdf_tools::USE_ONLY_COLLISION_OBJECTS, "objects"},
                                                                  {sdf_tools::USE_ONLY_OCTOMAP, "octomap"}, {sdf_tools::USE_CACHED, "cached"}};
        for (const auto& mode : modes) {
            const VoxelGrid::VoxelGrid<uint8_t> map = builder.UpdateCollisionMap(mode.mode);
            const sdf_tools::SignedDistanceField sdf = builder.UpdateSDF(mode.mode);
            std::cout << mode.name << ": " << map.GetNumXCells() << " x " << map.GetNumYCells() << " x " << map.GetNumZCells() << " cells, " << Filled(map)
                      << " filled, distance at the grid's centre " << sdf.GetImmutable(map.GetNumXCells() / 2, map.GetNumYCells() / 2, map.GetNumZCells() / 2).first
                      << std::endl;
            Write(dir, std::string("collision_map_") + mode.name + ".u8", map.GetImmutableRawData().data(), map.GetImmutableRawData().size());
            Write(dir, std::string("sdf_") + mode.name + ".f32", sdf.GetImmutableRawData().data(), sdf.GetImmutableRawData().size());
            if (Filled(builder.GetCachedCollisionMap()) != Filled(map) || builder.GetCachedSDF().GetImmutableRawData() != sdf.GetImmutableRawData())
                throw std::runtime_error("the cached results differ from the returned ones");
        }
        std::cout << "the scene was fetched " << fetched << " times" << std::endl;       // (twice per non-cached mode)

        builder.UpdatePlanningSceneFromMessage(MakeScene());
        const sdf_tools::TaggedObjectCollisionMapGrid tagged = builder.UpdateTaggedCollisionMap(sdf_tools::USE_CACHED);
        std::vector<uint32_t> ids;
        for (const auto& cell : tagged.GetImmutableRawData()) ids.push_back(cell.object_id);
        Write(dir, "tagged_ids.u32", ids.data(), ids.size());
        sdf_tools::DeviceSignedDistanceField device_sdf = builder.UpdateSDFDevice(sdf_tools::USE_CACHED);
        const sdf_tools::SignedDistanceField& host = device_sdf.Host();
        Write(dir, "device_sdf.f32", host.GetImmutableRawData().data(), host.GetImmutableRawData().size());
        std::cout << "device-resident SDF: extrema " << device_sdf.GetExtrema().first << " " << device_sdf.GetExtrema().second << std::endl;

        // a cone is refused, by name
        moveit_msgs::PlanningScene with_cone = MakeScene();
        with_cone.world.collision_objects[1].primitives[0].type = shape_msgs::SolidPrimitive::CONE;
        with_cone.world.collision_objects[1].primitives[0].dimensions = {0.2, 0.1};
        builder.UpdatePlanningSceneFromMessage(with_cone);
        try {
            builder.UpdateCollisionMap(sdf_tools::USE_CACHED);
            std::cerr << "a cone was not refused" << std::endl;
            return 1;
        } catch (const std::invalid_argument& e) {
            std::cout << "refused: " << e.what() << std::endl;
        }
    } catch (const std::exception& e) {
        std::cerr << "sdf_builder example failed: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "sdf_builder example done" << std::endl;
    return 0;
}
