// sdf_builder_solid -- sdf_tools::SDF_Builder with MESH_FILL_SOLID: a closed mesh (a box given as 12 triangles) filled inside, beside
// the same box as a primitive.  Under the default, MESH_FILL_SURFACE, the SDF at the mesh's centre is positive; as a solid it is
// negative and equals the primitive's.  Usage: sdf_builder_solid_example
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

}  // namespace

int main() {
    try {
        moveit_msgs::PlanningScene scene;
        scene.name = "solid mesh example";
        moveit_msgs::CollisionObject primitive, mesh;
        primitive.id = "box as a primitive";
        shape_msgs::SolidPrimitive box;
        box.type = shape_msgs::SolidPrimitive::BOX;
        box.dimensions = {0.4, 0.3, 0.5};
        primitive.primitives.push_back(box);
        primitive.primitive_poses.push_back(MakePose(-0.4, 0.0, 0.0, 0.9, 0.1, -0.2, 0.3));
        mesh.id = "box as 12 triangles";
        mesh.meshes.push_back(BoxMesh(0.4, 0.3, 0.5));
        mesh.mesh_poses.push_back(MakePose(0.4, 0.0, 0.0, 0.9, 0.1, -0.2, 0.3));      // the same box, 0.8 m = 32 voxels further along x
        scene.world.collision_objects = {primitive, mesh};

        sdf_tools::SDF_Builder builder("world", 1.6, 1.2, 1.4, 0.025, 1e6f);
        builder.UpdatePlanningSceneFromMessage(scene);
        const double as_surface = builder.UpdateSDF(sdf_tools::USE_CACHED).GetImmutable(0.4, 0.0, 0.0).first;
        builder.SetMeshFill(sdf_tools::MESH_FILL_SOLID);                       // or SetObjectMeshFill("box as 12 triangles", ...) for this object alone
        const sdf_tools::SignedDistanceField sdf = builder.UpdateSDF(sdf_tools::USE_CACHED);
        const double as_solid = sdf.GetImmutable(0.4, 0.0, 0.0).first, in_primitive = sdf.GetImmutable(-0.4, 0.0, 0.0).first;
        std::cout << "distance at the mesh's centre: " << as_surface << " as a surface, " << as_solid << " as a solid; at the primitive's centre "
                  << in_primitive << std::endl;
        if (!(as_surface > 0.0 && as_solid < 0.0 && as_solid == in_primitive)) throw std::runtime_error("unexpected distances");
        // an open mesh cannot be a solid: refused before the GPU is touched
        scene.world.collision_objects[1].meshes[0].triangles.pop_back();
        builder.UpdatePlanningSceneFromMessage(scene);
        try {
            builder.UpdateSDF(sdf_tools::USE_CACHED);
            throw std::runtime_error("an open mesh was accepted");
        } catch (const std::invalid_argument& e) {
            std::cout << "refused: " << e.what() << std::endl;
        }
    } catch (const std::exception& e) {
        std::cerr << "sdf_builder_solid example failed: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "sdf_builder_solid example done" << std::endl;
    return 0;
}
