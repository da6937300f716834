// display_export -- client code written like the reference's (src/sdf_tools_tutorial.cpp:97-147): build the tutorial scene, export
// the collision map, its surfaces, its components and the SDF for display, and print what a test can check.  One line per marker:
//   <name> ns=<ns> frame=<frame> id type action scale points colors first=<x y z> sum=<sum of the point coordinates>
#include <cstdio>

#include "sdf_tools/collision_map.hpp"
#include "sdf_tools/tagged_object_collision_map.hpp"

static void Print(const char* name, const visualization_msgs::Marker& m) {
    double sum = 0.0;
    for (const geometry_msgs::Point& p : m.points) sum += p.x + p.y + p.z;
    const geometry_msgs::Point first = m.points.empty() ? geometry_msgs::Point() : m.points[0];
    std::printf("%s ns=%s frame=%s id=%d type=%d action=%d scale=%.17g pose=%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g points=%zu colors=%zu first=%.17g,%.17g,%.17g sum=%.17g\n",
                name, m.ns.c_str(), m.header.frame_id.c_str(), m.id, m.type, m.action, m.scale.x, m.pose.position.x, m.pose.position.y,
                m.pose.position.z, m.pose.orientation.x, m.pose.orientation.y, m.pose.orientation.z, m.pose.orientation.w, m.points.size(),
                m.colors.size(), first.x, first.y, first.z, sum);
}

int main() {
    const double resolution = 0.25;
    Eigen::Isometry3d origin = Eigen::Isometry3d::Identity();
    origin.setTranslation(-5.0, -5.0, -5.0);
    sdf_tools::CollisionMapGrid map(origin, "tutorial_frame", resolution, (int64_t)40, (int64_t)40, (int64_t)40, sdf_tools::COLLISION_CELL(0.0f));
    for (int64_t x = 0; x < 20; ++x)
        for (int64_t y = 0; y < 20; ++y)
            for (int64_t z = 0; z < 20; ++z) map.SetValue(x, y, z, sdf_tools::COLLISION_CELL(1.0f));
    map.SetValue((int64_t)39, (int64_t)39, (int64_t)39, sdf_tools::COLLISION_CELL(0.5f));
    const std_msgs::ColorRGBA red = sdf_tools::display::MakeColor(1.0f, 0.0f, 0.0f, 1.0f), none = std_msgs::ColorRGBA(),
                              grey = sdf_tools::display::MakeColor(0.5f, 0.5f, 0.5f, 0.5f);
    Print("map", map.ExportForDisplay(red, none, grey));
    Print("surfaces", map.ExportSurfacesForDisplay(red, grey, grey));
    const visualization_msgs::MarkerArray separate = map.ExportSurfacesForSeparateDisplay(red, grey, grey);
    for (const visualization_msgs::Marker& m : separate.markers) Print("separate", m);
    map.UpdateConnectedComponents();
    Print("components", map.ExportConnectedComponentsForDisplay(false));
    const auto sdf = map.ExtractSignedDistanceField(1e6f, true, false);
    Print("sdf", sdf.first.ExportForDisplay(0.5f));
    Print("sdf_collision", sdf.first.ExportForDisplayCollisionOnly(0.5f));

    sdf_tools::TaggedObjectCollisionMapGrid tagged(origin, "tutorial_frame", resolution, (int64_t)8, (int64_t)8, (int64_t)8,
                                                   sdf_tools::TAGGED_OBJECT_COLLISION_CELL(0.0f, 0u));
    for (int64_t z = 0; z < 8; ++z) {
        tagged.SetValue((int64_t)1, (int64_t)1, z, sdf_tools::TAGGED_OBJECT_COLLISION_CELL(1.0f, 7u));
        tagged.SetValue((int64_t)0, (int64_t)2, z, sdf_tools::TAGGED_OBJECT_COLLISION_CELL(1.0f, 3u));
    }
    Print("tagged", tagged.ExportForDisplay(1.0f));
    for (const visualization_msgs::Marker& m : tagged.ExportForDisplayUniqueNs(1.0f).markers) Print("unique", m);
    for (const visualization_msgs::Marker& m : tagged.ExportForDisplayUniqueNs(1.0f, {7u, 9u, 3u}).markers) Print("listed", m);
    return 0;
}
