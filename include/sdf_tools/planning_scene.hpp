// planning_scene -- plain mirrors of the messages sdf_tools::SDF_Builder (sdf_builder.hpp) reads, for builds without ROS and MoveIt, in
// the style of display.hpp: shape_msgs::SolidPrimitive, Mesh and Plane, geometry_msgs::Pose (display.hpp's), moveit_msgs::CollisionObject,
// PlanningSceneWorld and PlanningScene keep the field names and constants of the messages, as far as the builder reads them.
//
// The octomap is the exception: octomap_msgs::OctomapWithPose carries a serialised tree, and the octomap library that reads it is not
// part of this project.  Its mirror holds what MoveIt's world makes of the tree: one axis-aligned box per occupied leaf, centres and
// edge lengths in the octomap's frame, and the pose of that frame.  A client with the octomap library fills it from
// tree.begin_leafs() (leaf centre, leaf size) for the occupied leaves.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "sdf_tools/display.hpp"

namespace shape_msgs {
struct SolidPrimitive {
    enum : uint8_t { BOX = 1, SPHERE = 2, CYLINDER = 3, CONE = 4 };
    enum : uint8_t { BOX_X = 0, BOX_Y = 1, BOX_Z = 2, SPHERE_RADIUS = 0, CYLINDER_HEIGHT = 0, CYLINDER_RADIUS = 1, CONE_HEIGHT = 0, CONE_RADIUS = 1 };
    uint8_t type = 0;
    std::vector<double> dimensions;
};
struct MeshTriangle { uint32_t vertex_indices[3] = {0, 0, 0}; };
struct Mesh { std::vector<MeshTriangle> triangles; std::vector<geometry_msgs::Point> vertices; };
struct Plane { double coef[4] = {0.0, 0.0, 0.0, 0.0}; };
}  // namespace shape_msgs

namespace octomap_msgs {
// occupied leaves as boxes (see the head of this file); sizes[i] is the edge length of the leaf at centers[i]
struct OctomapBoxes {
    std_msgs::Header header;
    std::vector<geometry_msgs::Point> centers;
    std::vector<double> sizes;
};
struct OctomapBoxesWithPose {
    std_msgs::Header header;
    geometry_msgs::Pose origin;
    OctomapBoxes octomap;
    OctomapBoxesWithPose() { origin.orientation.w = 1.0; }
};
}  // namespace octomap_msgs

namespace moveit_msgs {
struct CollisionObject {
    enum : int8_t { ADD = 0, REMOVE = 1, APPEND = 2, MOVE = 3 };
    std_msgs::Header header;
    std::string id;
    std::vector<shape_msgs::SolidPrimitive> primitives;
    std::vector<geometry_msgs::Pose> primitive_poses;
    std::vector<shape_msgs::Mesh> meshes;
    std::vector<geometry_msgs::Pose> mesh_poses;
    std::vector<shape_msgs::Plane> planes;
    std::vector<geometry_msgs::Pose> plane_poses;
    int8_t operation = ADD;
};
struct PlanningSceneWorld {
    std::vector<CollisionObject> collision_objects;
    octomap_msgs::OctomapBoxesWithPose octomap;
};
struct PlanningScene {
    std::string name;
    PlanningSceneWorld world;
    bool is_diff = false;
};
}  // namespace moveit_msgs

namespace sdf_tools {

// geometry_msgs::Pose -> row-major 4 x 4 (shape frame -> the pose's parent frame).  The quaternion is normalised, then Eigen's
// toRotationMatrix products in their order (tests/resample_restated.py quaternion_origin states the same products).
inline void PoseToMatrix(const geometry_msgs::Pose& pose, double out[16]) {
    double w = pose.orientation.w, x = pose.orientation.x, y = pose.orientation.y, z = pose.orientation.z;
    const double n = std::sqrt(w * w + x * x + y * y + z * z);
    w = w / n; x = x / n; y = y / n; z = z / n;
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double m[16] = {1.0 - (tyy + tzz), txy - twz, txz + twy, pose.position.x,
                          txy + twz, 1.0 - (txx + tzz), tyz - twx, pose.position.y,
                          txz - twy, tyz + twx, 1.0 - (txx + tyy), pose.position.z,
                          0.0, 0.0, 0.0, 1.0};
    for (int i = 0; i < 16; ++i) out[i] = m[i];
}

}  // namespace sdf_tools
