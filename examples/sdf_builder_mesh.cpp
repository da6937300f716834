// sdf_builder_mesh -- sdf_tools::SDF_Builder on a scene with a mesh and a plane: a box given as 12 triangles beside the same box as a
// primitive, and a floor plane.  The primitive fills its inside, the mesh only the voxels its surface passes through; the plane
// fills the layer of voxels it cuts.  Usage: sdf_builder_mesh_example
#include <iostream>
#include <stdexcept>
#include <vector>

#include "sdf_tools/sdf_builder.hpp"

namespace {

geometry_msgs::Pose MakePose(double px, double py, double pz, double qw, double qx, double qy, double qz) {
    geometry_msgs::Pose pose;
    pose.position.x = px; pose.position.y = py; pose.position.z = pz;
    pose.orientation.w = qw; pose.orientation.x = qx; pose.orientation.y = qy; pose.orientation.z = qz;
    return pose;
}

// the box of full extents (x, y, z) about the origin as 8 vertices and 12 triangles
shape_msgs::Mesh BoxMesh(double x, double y, double z) {
    shape_msgs::Mesh mesh;
    for (int k = 0; k < 8; ++k) {
        geometry_msgs::Point p;
        p.x = (k & 1 ? 0.5 : -0.5) * x; p.y = (k & 2 ? 0.5 : -0.5) * y; p.z = (k & 4 ? 0.5 : -0.5) * z;
        mesh.vertices.push_back(p);
    }
    const uint32_t faces[12][3] = {{0, 1, 3}, {0, 3, 2}, {4, 6, 7}, {4, 7, 5}, {0, 4, 5}, {0, 5, 1}, {2, 3, 7}, {2, 7, 6}, {0, 2, 6}, {0, 6, 4}, {1, 5, 7}, {1, 7, 3}};
    for (const auto& f : faces) {
        shape_msgs::MeshTriangle t;
        for (int i = 0; i < 3; ++i) t.vertex_indices[i] = f[i];
        mesh.triangles.push_back(t);
    }
    return mesh;
}

size_t Count(const sdf_tools::TaggedObjectCollisionMapGrid& map, uint32_t id) {
    size_t count = 0;
    for (const auto& cell : map.GetImmutableRawData()) count += cell.object_id == id;
    return count;
}

}  // namespace

int main() {
    try {
        moveit_msgs::PlanningScene scene;
        scene.name = "mesh example";
        moveit_msgs::CollisionObject solid, shell, floor;
        solid.id = "box as a primitive";
        shape_msgs::SolidPrimitive box;
        box.type = shape_msgs::SolidPrimitive::BOX;
        box.dimensions = {0.4, 0.3, 0.5};
        solid.primitives.push_back(box);
        solid.primitive_poses.push_back(MakePose(-0.35, 0.0, 0.1, 0.9, 0.1, -0.2, 0.3));
        shell.id = "box as 12 triangles";
        shell.meshes.push_back(BoxMesh(0.4, 0.3, 0.5));
        shell.mesh_poses.push_back(MakePose(0.35, 0.0, 0.1, 0.9, 0.1, -0.2, 0.3));
        floor.id = "floor";
        shape_msgs::Plane plane;                                              // z = -0.51: 0 x + 0 y + 1 z + 0.51 = 0 (inside a layer of voxels)
        plane.coef[2] = 1.0; plane.coef[3] = 0.51;
        floor.planes.push_back(plane);
        floor.plane_poses.push_back(MakePose(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0));
        scene.world.collision_objects = {solid, shell, floor};

        sdf_tools::SDF_Builder builder("world", 1.6, 1.2, 1.4, 0.025, 1e6f);
        builder.UpdatePlanningSceneFromMessage(scene);
        const VoxelGrid::VoxelGrid<uint8_t> map = builder.UpdateCollisionMap(sdf_tools::USE_CACHED);
        const sdf_tools::TaggedObjectCollisionMapGrid tagged = builder.UpdateTaggedCollisionMap(sdf_tools::USE_CACHED);
        const sdf_tools::SignedDistanceField sdf = builder.UpdateSDF(sdf_tools::USE_CACHED);
        size_t filled = 0;
        for (const uint8_t v : map.GetImmutableRawData()) filled += v;
        const size_t n_solid = Count(tagged, 1), n_shell = Count(tagged, 2), n_floor = Count(tagged, 3);
        std::cout << map.GetNumXCells() << " x " << map.GetNumYCells() << " x " << map.GetNumZCells() << " cells, " << filled << " filled: " << n_solid
                  << " by the primitive, " << n_shell << " by the mesh's surface, " << n_floor << " by the floor" << std::endl;
        if (filled != n_solid + n_shell + n_floor) throw std::runtime_error("the collision map and the tagged map disagree");
        if (!(n_shell > 0 && n_shell < n_solid)) throw std::runtime_error("the mesh should fill its surface only");
        if (n_floor != (size_t)(map.GetNumXCells() * map.GetNumYCells())) throw std::runtime_error("the floor should fill one layer");
        // the centres of the two boxes in the grid: inside the primitive the distance is negative, inside the closed mesh positive
        const double inside_solid = sdf.GetImmutable(-0.35, 0.0, 0.1).first, inside_shell = sdf.GetImmutable(0.35, 0.0, 0.1).first;
        std::cout << "distance at the primitive's centre " << inside_solid << ", at the mesh's centre " << inside_shell << std::endl;
        if (!(inside_solid < 0.0 && inside_shell > 0.0)) throw std::runtime_error("unexpected signs");
    } catch (const std::exception& e) {
        std::cerr << "sdf_builder_mesh example failed: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "sdf_builder_mesh example done" << std::endl;
    return 0;
}
