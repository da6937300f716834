// pysdf_tools -- pybind11 module with the surface of the reference's src/sdf_tools/bindings.cpp
// (module name, class names, method names and positional argument orders, :15-106), bound to the
// in-tree mirror classes whose SDF build runs on the MI355X through the C ABI (libsdfgpu.so).
// Extras beside (not instead of) the reference-shaped methods: numpy fast paths
// (SetOccupancyFromNumpy / GetRawDataNumpy / GetFullGradientNumpy / GetComponentsNumpy) that avoid per-voxel Python calls,
// and the GIL is released for the duration of ExtractSignedDistanceField.
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <cstdint>
#include <map>
#include <cstring>
#include <type_traits>
#include <utility>

#include "arc_utilities/zlib_helpers.hpp"
#include "sdf_tools/collision_map.hpp"
#include "sdf_tools/device_sdf.hpp"
#include "sdf_tools/dynamic_spatial_hashed_collision_map.hpp"
#include "sdf_tools/sdf_builder.hpp"
#include "sdf_tools/tagged_object_collision_map.hpp"

namespace py = pybind11;
using namespace sdf_tools;
using Eigen::Isometry3d;

namespace {

Isometry3d IsometryFromArray(const py::array_t<double, py::array::c_style | py::array::forcecast>& m) {
    if (m.ndim() != 2 || m.shape(0) != 4 || m.shape(1) != 4) throw std::invalid_argument("Isometry3d expects a 4x4 matrix");
    Isometry3d t = Isometry3d::Identity();
    auto a = m.unchecked<2>();
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) t.matrix()(r, c) = a(r, c);
    return t;
}

py::tuple ToTuple(const Eigen::Vector3d& v) { return py::make_tuple(v.x(), v.y(), v.z()); }

py::array_t<double> MatrixToArray(const Isometry3d& t) {
    py::array_t<double> out({4, 4});
    auto a = out.mutable_unchecked<2>();
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) a(r, c) = t.matrix()(r, c);
    return out;
}

}  // namespace

// ExtractComponentSurfaces for Python: {component: {(x, y, z): 1}}, and the bulk form (offsets int64 [max_label + 2], indices uint32)
template <typename Grid>
py::dict SurfacesDict(const Grid& g, int types) {
    sdf_tools::ComponentSurfaceIndices s;
    {
        py::gil_scoped_release release;
        s = g.ExtractComponentSurfaceIndices((typename Grid::COMPONENT_TYPES)types);
    }
    const int64_t ny = g.GetNumYCells(), nz = g.GetNumZCells();
    py::dict out;
    for (size_t c = 0; c + 1 < s.offsets.size(); ++c) {
        if (s.offsets[c + 1] == s.offsets[c]) continue;
        py::dict cells;
        for (uint64_t i = s.offsets[c]; i < s.offsets[c + 1]; ++i) {
            const int64_t v = (int64_t)s.indices[(size_t)i], t = v / nz;
            cells[py::make_tuple(t / ny, t % ny, v % nz)] = 1;
        }
        out[py::int_(c)] = cells;
    }
    return out;
}

template <typename Grid>
py::tuple SurfacesNumpy(const Grid& g, int types) {
    sdf_tools::ComponentSurfaceIndices s;
    {
        py::gil_scoped_release release;
        s = g.ExtractComponentSurfaceIndices((typename Grid::COMPONENT_TYPES)types);
    }
    py::array_t<int64_t> offsets((py::ssize_t)s.offsets.size());
    for (size_t c = 0; c < s.offsets.size(); ++c) offsets.mutable_data()[c] = (int64_t)s.offsets[c];
    py::array_t<uint32_t> indices((py::ssize_t)s.indices.size());
    if (!s.indices.empty()) std::memcpy(indices.mutable_data(), s.indices.data(), s.indices.size() * sizeof(uint32_t));
    return py::make_tuple(offsets, indices);
}

template <typename Grid, typename Class>
void DefSurfaces(Class& cls) {
    cls.def("ExtractComponentSurfaces", [](const Grid& g, int types) { return SurfacesDict(g, types); }, py::arg("component_types_to_extract"),
            "{component: {(x, y, z): 1}} of the surface voxels whose class is in FILLED_COMPONENTS | EMPTY_COMPONENTS | UNKNOWN_COMPONENTS, "
            "from the stored components, on the GPU (include/sdfgpu.h \"Component surfaces\")")
        .def("ExtractFilledComponentSurfaces", [](const Grid& g) { return SurfacesDict(g, 1); })
        .def("ExtractEmptyComponentSurfaces", [](const Grid& g) { return SurfacesDict(g, 2); })
        .def("ExtractUnknownComponentSurfaces", [](const Grid& g) { return SurfacesDict(g, 4); })
        .def("ExtractComponentSurfaceIndicesNumpy", [](const Grid& g, int types) { return SurfacesNumpy(g, types); },
             py::arg("component_types_to_extract"),
             "(offsets int64 [max_label + 2], indices uint32): component c's surface voxels are indices[offsets[c]:offsets[c + 1]], ascending");
    cls.attr("FILLED_COMPONENTS") = py::int_(1);
    cls.attr("EMPTY_COMPONENTS") = py::int_(2);
    cls.attr("UNKNOWN_COMPONENTS") = py::int_(4);
}

// ---- display export for Python: the reference binds none of it, so these are numpy forms of the C++ methods.  A Marker becomes
// (points float64 [n, 3] in the grid frame, colors float32 [n, 4]); a MarkerArray a list of (ns, points, colors); colours go in as
// (r, g, b, a).  MarkerInfo gives what every method fills besides the elements.
static_assert(sizeof(geometry_msgs::Point) == 24 && sizeof(std_msgs::ColorRGBA) == 16, "points and colours are copied as plain arrays");

using Rgba = std::array<float, 4>;
std_msgs::ColorRGBA ColorOf(const Rgba& c) { return sdf_tools::display::MakeColor(c[0], c[1], c[2], c[3]); }

py::tuple MarkerNumpy(const visualization_msgs::Marker& m) {
    py::array_t<double> points({(py::ssize_t)m.points.size(), (py::ssize_t)3});
    py::array_t<float> colors({(py::ssize_t)m.colors.size(), (py::ssize_t)4});
    if (!m.points.empty()) std::memcpy(points.mutable_data(), m.points.data(), m.points.size() * sizeof(geometry_msgs::Point));
    if (!m.colors.empty()) std::memcpy(colors.mutable_data(), m.colors.data(), m.colors.size() * sizeof(std_msgs::ColorRGBA));
    return py::make_tuple(points, colors);
}

py::list MarkerArrayNumpy(const visualization_msgs::MarkerArray& a) {
    py::list out;
    for (const visualization_msgs::Marker& m : a.markers) {
        const py::tuple t = MarkerNumpy(m);
        out.append(py::make_tuple(m.ns, t[0], t[1]));
    }
    return out;
}

py::dict MarkerInfo(const visualization_msgs::Marker& m) {
    py::dict d;
    d["frame_id"] = m.header.frame_id;
    d["ns"] = m.ns;
    d["id"] = m.id;
    d["type"] = m.type;
    d["action"] = m.action;
    d["lifetime"] = m.lifetime;
    d["frame_locked"] = m.frame_locked;
    d["position"] = py::make_tuple(m.pose.position.x, m.pose.position.y, m.pose.position.z);
    d["orientation"] = py::make_tuple(m.pose.orientation.x, m.pose.orientation.y, m.pose.orientation.z, m.pose.orientation.w);
    d["scale"] = py::make_tuple(m.scale.x, m.scale.y, m.scale.z);
    d["color"] = py::make_tuple(m.color.r, m.color.g, m.color.b, m.color.a);
    d["points"] = m.points.size();
    d["colors"] = m.colors.size();
    return d;
}

template <typename Make>
py::tuple ReleasedMarker(Make make) {
    visualization_msgs::Marker m;
    { py::gil_scoped_release release; m = make(); }
    return MarkerNumpy(m);
}
template <typename Make>
py::list ReleasedMarkerArray(Make make) {
    visualization_msgs::MarkerArray a;
    { py::gil_scoped_release release; a = make(); }
    return MarkerArrayNumpy(a);
}

std::map<uint32_t, std_msgs::ColorRGBA> ColorMapOf(const std::map<uint32_t, Rgba>& in) {
    std::map<uint32_t, std_msgs::ColorRGBA> out;
    for (const auto& kv : in) out[kv.first] = ColorOf(kv.second);
    return out;
}

// Resample, and the cell records in bulk (uint8 [nx, ny, nz, sizeof(cell)]) so that whole grids go in and out without per-cell calls
template <typename Grid, typename Class>
void DefResample(Class& cls) {
    using Cell = typename std::remove_cv<typename std::remove_reference<decltype(std::declval<Grid>().GetOOBValue())>::type>::type;
    cls.def("Resample", [](const Grid& g, double new_resolution) { return g.Resample(new_resolution); }, py::arg("new_resolution"),
            py::call_guard<py::gil_scoped_release>(),
            "a grid over the same volume at new_resolution, on the GPU (include/sdfgpu.h \"Resample\"): each cell overwrites the result cell "
            "that holds its centre, in x -> y -> z order; result cells that hold no source centre keep the OOB value")
        .def("SetRawCellsNumpy", [](Grid& g, const py::array_t<uint8_t, py::array::c_style>& raw) {
            auto& cells = g.GetMutableRawData();
            if ((size_t)raw.size() != cells.size() * sizeof(Cell)) throw std::invalid_argument("records array must hold nx * ny * nz cells");
            // (through SetValue for the first cell: the grid's stored components and segments no longer describe it)
            std::memcpy(static_cast<void*>(cells.data()), raw.data(), (size_t)raw.size());
            if (!cells.empty()) { const Cell first = cells[0]; g.SetValue((int64_t)0, (int64_t)0, (int64_t)0, first); }
        }, "overwrite every cell record from uint8 [nx, ny, nz, cell bytes]; stored components become invalid")
        .def("GetRawCellsNumpy", [](const Grid& g) {
            py::array_t<uint8_t> out({(py::ssize_t)g.GetNumXCells(), (py::ssize_t)g.GetNumYCells(), (py::ssize_t)g.GetNumZCells(), (py::ssize_t)sizeof(Cell)});
            const auto& cells = g.GetImmutableRawData();
            std::memcpy(out.mutable_data(), static_cast<const void*>(cells.data()), cells.size() * sizeof(Cell));
            return out;
        }, "the cell records as uint8 [nx, ny, nz, cell bytes]");
}

PYBIND11_MODULE(pysdf_tools, m) {
    m.doc() = "MI355X-native drop-in for sdf_tools' pysdf_tools (SDF build on the GPU via libsdfgpu.so)";

    py::class_<COLLISION_CELL>(m, "COLLISION_CELL")
        .def(py::init<float>())
        .def(py::init<float, uint32_t>())
        .def_readwrite("occupancy", &COLLISION_CELL::occupancy)
        .def_readwrite("component", &COLLISION_CELL::component);

    py::class_<Isometry3d>(m, "Isometry3d")
        .def(py::init(&IsometryFromArray))
        .def("translation", [](const Isometry3d& t) {
            const auto v = t.translation();
            py::array_t<double> out(3);
            out.mutable_at(0) = v(0); out.mutable_at(1) = v(1); out.mutable_at(2) = v(2);
            return out;
        })
        .def("matrix", &MatrixToArray);

    py::class_<SDF>(m, "SDF")
        .def(py::init<>())
        .def_readwrite("serialized_sdf", &SDF::serialized_sdf)
        .def_readwrite("is_compressed", &SDF::is_compressed)
        .def_property("frame_id", [](const SDF& s) { return s.header.frame_id; }, [](SDF& s, const std::string& f) { s.header.frame_id = f; });

    py::class_<CollisionMap>(m, "CollisionMap")                // plain mirror of msg/CollisionMap.msg
        .def(py::init<>())
        .def_readwrite("serialized_map", &CollisionMap::serialized_map)
        .def_readwrite("is_compressed", &CollisionMap::is_compressed)
        .def_property("frame_id", [](const CollisionMap& s) { return s.header.frame_id; }, [](CollisionMap& s, const std::string& f) { s.header.frame_id = f; });

    // The tagged-object map (not in the reference's pybind surface, bindings.cpp:15-106; bound here beside it so that its wire
    // type and its SDF callers -- tagged_object_collision_map.hpp:730-915, .cpp:23-339 -- can be driven from Python tests)
    py::class_<TAGGED_OBJECT_COLLISION_CELL>(m, "TAGGED_OBJECT_COLLISION_CELL")
        .def(py::init<>())
        .def(py::init<float, uint32_t>())
        .def(py::init<float, uint32_t, uint32_t, uint32_t>())
        .def_readwrite("occupancy", &TAGGED_OBJECT_COLLISION_CELL::occupancy)
        .def_readwrite("component", &TAGGED_OBJECT_COLLISION_CELL::component)
        .def_readwrite("object_id", &TAGGED_OBJECT_COLLISION_CELL::object_id)
        .def_readwrite("convex_segment", &TAGGED_OBJECT_COLLISION_CELL::convex_segment);
    py::class_<TaggedObjectCollisionMap>(m, "TaggedObjectCollisionMap")   // plain mirror of msg/TaggedObjectCollisionMap.msg
        .def(py::init<>())
        .def_readwrite("serialized_map", &TaggedObjectCollisionMap::serialized_map)
        .def_readwrite("is_compressed", &TaggedObjectCollisionMap::is_compressed)
        .def_property("frame_id", [](const TaggedObjectCollisionMap& s) { return s.header.frame_id; },
                      [](TaggedObjectCollisionMap& s, const std::string& f) { s.header.frame_id = f; });
    py::class_<TaggedObjectCollisionMapGrid> tagged_grid(m, "TaggedObjectCollisionMapGrid");
    DefSurfaces<TaggedObjectCollisionMapGrid>(tagged_grid);
    DefResample<TaggedObjectCollisionMapGrid>(tagged_grid);
    tagged_grid
        .def("DefaultMarker", [](const TaggedObjectCollisionMapGrid& g) { return MarkerInfo(g.DefaultMarker()); },
             "what every display method fills besides ns and the elements, as a dict")
        .def("ExportForDisplay", [](const TaggedObjectCollisionMapGrid& g, float alpha, const std::vector<uint32_t>& objects_to_draw) {
            return ReleasedMarker([&]() { return g.ExportForDisplay(alpha, objects_to_draw); });
        }, py::arg("alpha") = 1.0f, py::arg("objects_to_draw") = std::vector<uint32_t>(), "(points, colors) of the cells of the listed objects (all when empty)")
        .def("ExportForDisplay", [](const TaggedObjectCollisionMapGrid& g, const std::map<uint32_t, Rgba>& color_map) {
            return ReleasedMarker([&]() { return g.ExportForDisplay(ColorMapOf(color_map)); });
        }, py::arg("color_map"))
        .def("ExportForDisplayUniqueNs", [](const TaggedObjectCollisionMapGrid& g, float alpha, const std::vector<uint32_t>& objects_to_draw) {
            return ReleasedMarkerArray([&]() { return g.ExportForDisplayUniqueNs(alpha, objects_to_draw); });
        }, py::arg("alpha") = 1.0f, py::arg("objects_to_draw") = std::vector<uint32_t>(), "[(ns, points, colors)]: one entry per drawn object")
        .def("ExportForDisplayUniqueNs", [](const TaggedObjectCollisionMapGrid& g, const std::map<uint32_t, Rgba>& color_map) {
            return ReleasedMarkerArray([&]() { return g.ExportForDisplayUniqueNs(ColorMapOf(color_map)); });
        }, py::arg("color_map"))
        .def("ExportContourOnlyForDisplay", [](const TaggedObjectCollisionMapGrid& g, float alpha, const std::vector<uint32_t>& objects_to_draw) {
            return ReleasedMarker([&]() { return g.ExportContourOnlyForDisplay(alpha, objects_to_draw); });
        }, py::arg("alpha") = 1.0f, py::arg("objects_to_draw") = std::vector<uint32_t>(),
             "(points, colors) of the outline cells of the listed objects (every id > 0 when empty): include/sdfgpu.h \"Display export: contours\"")
        .def("ExportContourOnlyForDisplay", [](const TaggedObjectCollisionMapGrid& g, const std::map<uint32_t, Rgba>& color_map) {
            return ReleasedMarker([&]() { return g.ExportContourOnlyForDisplay(ColorMapOf(color_map)); });
        }, py::arg("color_map"))
        .def("ExportContourOnlyForDisplayUniqueNs", [](const TaggedObjectCollisionMapGrid& g, float alpha, const std::vector<uint32_t>& objects_to_draw) {
            return ReleasedMarkerArray([&]() { return g.ExportContourOnlyForDisplayUniqueNs(alpha, objects_to_draw); });
        }, py::arg("alpha") = 1.0f, py::arg("objects_to_draw") = std::vector<uint32_t>(), "[(ns, points, colors)]: one entry per drawn object, in ascending id")
        .def("ExportContourOnlyForDisplayUniqueNs", [](const TaggedObjectCollisionMapGrid& g, const std::map<uint32_t, Rgba>& color_map) {
            return ReleasedMarkerArray([&]() { return g.ExportContourOnlyForDisplayUniqueNs(ColorMapOf(color_map)); });
        }, py::arg("color_map"))
        .def("ExportContourOnlyForDisplayInfo", [](const TaggedObjectCollisionMapGrid& g, float alpha) {
            return MarkerInfo(g.ExportContourOnlyForDisplay(alpha));
        }, py::arg("alpha") = 1.0f, "header, ns, id, type, action, pose, scale and the element counts of ExportContourOnlyForDisplay")
        .def("ExportForDisplayOccupancyOnly", [](const TaggedObjectCollisionMapGrid& g, const Rgba& c, const Rgba& f, const Rgba& u) {
            return ReleasedMarker([&]() { return g.ExportForDisplayOccupancyOnly(ColorOf(c), ColorOf(f), ColorOf(u)); });
        }, py::arg("collision_color"), py::arg("free_color"), py::arg("unknown_color"))
        .def("ExportConnectedComponentsForDisplay", [](const TaggedObjectCollisionMapGrid& g, bool color_unknown_components) {
            return ReleasedMarker([&]() { return g.ExportConnectedComponentsForDisplay(color_unknown_components); });
        }, py::arg("color_unknown_components"))
        .def("ExportConvexSegmentForDisplay", [](const TaggedObjectCollisionMapGrid& g, uint32_t object_id, uint32_t convex_segment) {
            return ReleasedMarker([&]() { return g.ExportConvexSegmentForDisplay(object_id, convex_segment); });
        }, py::arg("object_id"), py::arg("convex_segment"))
        .def("ExportSurfaceForDisplay", [](const TaggedObjectCollisionMapGrid& g, const std::vector<std::array<int64_t, 3>>& surface, const Rgba& color) {
            std::unordered_map<VoxelGrid::GRID_INDEX, uint8_t> map;
            for (const auto& i : surface) map[VoxelGrid::GRID_INDEX(i[0], i[1], i[2])] = 1;
            return MarkerNumpy(g.ExportSurfaceForDisplay(map, ColorOf(color)));
        }, py::arg("surface"), py::arg("color"), "host only; the elements come in the order of the hash map built from `surface`")
        .def_static("GenerateComponentColor", [](uint32_t id, float alpha) {
            const std_msgs::ColorRGBA c = TaggedObjectCollisionMapGrid::GenerateComponentColor(id, alpha);
            return py::make_tuple(c.r, c.g, c.b, c.a);
        }, py::arg("component"), py::arg("alpha") = 1.0f, "the in-tree palette (parity with arc_helpers UNVERIFIED); id 0 has alpha 0");
    tagged_grid
        .def(py::init<Isometry3d const&, std::string, double, int64_t, int64_t, int64_t, TAGGED_OBJECT_COLLISION_CELL const&>())
        .def(py::init<>())
        .def("SetValue", [](TaggedObjectCollisionMapGrid& g, int64_t x, int64_t y, int64_t z, const TAGGED_OBJECT_COLLISION_CELL& c) { return g.SetValue(x, y, z, c); })
        .def("UpdateConnectedComponents", &TaggedObjectCollisionMapGrid::UpdateConnectedComponents, py::call_guard<py::gil_scoped_release>())
        .def("GetNumConnectedComponents", &TaggedObjectCollisionMapGrid::GetNumConnectedComponents)
        .def("GetValueByIndex", [](const TaggedObjectCollisionMapGrid& g, int64_t x, int64_t y, int64_t z) { const auto q = g.GetImmutable(x, y, z); return std::make_pair(q.first, q.second); })
        .def("GetNumXCells", &TaggedObjectCollisionMapGrid::GetNumXCells)
        .def("GetNumYCells", &TaggedObjectCollisionMapGrid::GetNumYCells)
        .def("GetNumZCells", &TaggedObjectCollisionMapGrid::GetNumZCells)
        .def("GetFrame", &TaggedObjectCollisionMapGrid::GetFrame)
        .def("GetResolution", &TaggedObjectCollisionMapGrid::GetResolution)
        .def("SerializeSelf", [](const TaggedObjectCollisionMapGrid& g) { std::vector<uint8_t> b; g.SerializeSelf(b); return py::bytes(reinterpret_cast<const char*>(b.data()), b.size()); })
        .def_static("Deserialize", [](const py::bytes& data) { const std::string s = data; TaggedObjectCollisionMapGrid g; g.DeserializeSelf(std::vector<uint8_t>(s.begin(), s.end()), 0); return g; })
        .def("SaveToFile", [](const TaggedObjectCollisionMapGrid& g, const std::string& path, bool compress) { TaggedObjectCollisionMapGrid::SaveToFile(g, path, compress); })
        .def_static("LoadFromFile", &TaggedObjectCollisionMapGrid::LoadFromFile)
        .def("GetMessageRepresentation", [](const TaggedObjectCollisionMapGrid& g) { return TaggedObjectCollisionMapGrid::GetMessageRepresentation(g); })
        .def_static("LoadFromMessageRepresentation", &TaggedObjectCollisionMapGrid::LoadFromMessageRepresentation)
        .def("UpdateConvexSegments", &TaggedObjectCollisionMapGrid::UpdateConvexSegments, py::arg("connected_threshold"),
             py::arg("add_virtual_border"), py::call_guard<py::gil_scoped_release>(),
             "convex segments on the GPU (tagged_object_collision_map.cpp:552-654; include/sdfgpu.h \"Local extrema and convex segments\")")
        .def("GetNumConvexSegments", &TaggedObjectCollisionMapGrid::GetNumConvexSegments)
        .def("AreConvexSegmentsValid", &TaggedObjectCollisionMapGrid::AreConvexSegmentsValid)
        .def("GetConvexSegmentsNumpy", [](const TaggedObjectCollisionMapGrid& g) {
            py::array_t<uint32_t> out({(py::ssize_t)g.GetNumXCells(), (py::ssize_t)g.GetNumYCells(), (py::ssize_t)g.GetNumZCells()});
            uint32_t* o = out.mutable_data();
            const auto& cells = g.GetImmutableRawData();
            for (size_t i = 0; i < cells.size(); i++) o[i] = cells[i].convex_segment;
            return out;
        }, "the cells' convex segment labels as uint32 [nx, ny, nz] (0 until UpdateConvexSegments has run)")
        .def("ExtractSignedDistanceField", [](const TaggedObjectCollisionMapGrid& g, float oob_value, const std::vector<uint32_t>& objects_to_use,
                                               bool unknown_is_filled, bool add_virtual_border) {
            return g.ExtractSignedDistanceField(oob_value, objects_to_use, unknown_is_filled, add_virtual_border);
        }, py::call_guard<py::gil_scoped_release>())
        .def("MakeObjectSDFs", &TaggedObjectCollisionMapGrid::MakeObjectSDFs, py::arg("object_ids"), py::arg("unknown_is_filled"),
             py::arg("add_virtual_border"), py::call_guard<py::gil_scoped_release>(),
             "{object id: SignedDistanceField}, OOB value +inf, all ids in one batched build (sdfgpu_build_tagged_objects)")
        .def("MakeAllObjectSDFs", &TaggedObjectCollisionMapGrid::MakeAllObjectSDFs, py::arg("unknown_is_filled"), py::arg("add_virtual_border"),
             py::call_guard<py::gil_scoped_release>(), "... for every object id > 0 present in the grid");

    using VoxelGridVecd = VoxelGrid::VoxelGrid<std::vector<double>>;

    py::class_<SignedDistanceField>(m, "SignedDistanceField")
        .def(py::init<>())
        .def("ExportForDisplay", [](const SignedDistanceField& f, float alpha) { return ReleasedMarker([&]() { return f.ExportForDisplay(alpha); }); },
             py::arg("alpha") = 0.01f, "(points float64 [n, 3], colors float32 [n, 4]) of every cell, the colour map computed on the GPU")
        .def("ExportForDisplayCollisionOnly", [](const SignedDistanceField& f, float alpha) {
            return ReleasedMarker([&]() { return f.ExportForDisplayCollisionOnly(alpha); });
        }, py::arg("alpha") = 0.01f, "(points of the cells with d <= 0, an empty colour array: the marker has one colour)")
        .def("ExportForDisplayInfo", [](const SignedDistanceField& f, float alpha, bool collision_only) {
            return MarkerInfo(collision_only ? f.ExportForDisplayCollisionOnly(alpha) : f.ExportForDisplay(alpha));
        }, py::arg("alpha") = 0.01f, py::arg("collision_only") = false, "header, ns, id, type, action, pose, scale, color and the element counts")
        .def("GetRawData", &SignedDistanceField::GetImmutableRawData, "Please don't mutate this")
        .def("GetFullGradient", &SignedDistanceField::GetFullGradient)
        .def("GetResolution", &SignedDistanceField::GetResolution)
        .def("GetGradient",
             [](const SignedDistanceField& s, int64_t x, int64_t y, int64_t z, bool e) { return s.GetGradient(x, y, z, e); },
             "get the gradient based on index", py::arg("x_index"), py::arg("y_index"), py::arg("z_index"),
             py::arg("enable_edge_gradients") = false)
        .def("GetMessageRepresentation", [](const SignedDistanceField& s) { return SignedDistanceField::GetMessageRepresentation(s); })
        .def_static("LoadFromMessageRepresentation", &SignedDistanceField::LoadFromMessageRepresentation)
        .def("SaveToFile", [](const SignedDistanceField& s, const std::string& path, bool compress) { SignedDistanceField::SaveToFile(s, path, compress); })
        .def_static("LoadFromFile", &SignedDistanceField::LoadFromFile)
        .def("SerializeSelf", [](const SignedDistanceField& s) { std::vector<uint8_t> b; s.SerializeSelf(b); return py::bytes(reinterpret_cast<const char*>(b.data()), b.size()); })
        .def("DeserializeSelf",
             [](SignedDistanceField& s, const std::vector<uint8_t>& buffer, uint64_t current, py::object) { return s.DeserializeSelf(buffer, current); },
             "deserialize", py::arg("buffer"), py::arg("current"), py::arg("value_deserializer") = py::none())
        .def("GetOriginTransform", &SignedDistanceField::GetOriginTransform)
        .def("GetValueByCoordinates", [](const SignedDistanceField& s, double x, double y, double z) { const auto q = s.GetImmutable(x, y, z); return std::make_pair(q.first, q.second); },
             "Please don't mutate this", py::arg("x"), py::arg("y"), py::arg("z"))
        .def("GetValueByIndex", [](const SignedDistanceField& s, int64_t x, int64_t y, int64_t z) { const auto q = s.GetImmutable(x, y, z); return std::make_pair(q.first, q.second); },
             "Please don't mutate this", py::arg("x_index"), py::arg("y_index"), py::arg("z_index"))
        .def("GetNumXCells", &SignedDistanceField::GetNumXCells)
        .def("GetNumYCells", &SignedDistanceField::GetNumYCells)
        .def("GetNumZCells", &SignedDistanceField::GetNumZCells)
        .def("GetFrame", &SignedDistanceField::GetFrame)
        .def("EstimateDistance", [](const SignedDistanceField& s, double x, double y, double z) { return s.EstimateDistance(x, y, z); })
        // fast paths beside the reference-shaped API
        .def("GetRawDataNumpy", [](const SignedDistanceField& s) {
            py::array_t<float> out({s.GetNumXCells(), s.GetNumYCells(), s.GetNumZCells()});
            std::memcpy(out.mutable_data(), s.GetImmutableRawData().data(), s.GetImmutableRawData().size() * sizeof(float));
            return out;
        })
        .def("GetFullGradientNumpy", [](const SignedDistanceField& s, bool enable_edge_gradients) {
            const int64_t nx = s.GetNumXCells(), ny = s.GetNumYCells(), nz = s.GetNumZCells();
            // one kernel on the GPU (sdfgpu_gradient) instead of nx*ny*nz GetGradient calls; same values bit for bit.
            // Cells without a gradient (boundary shell when edge gradients are off) hold 3 x the OOB value here; the
            // reference's GetFullGradient stores an empty vector there (sdf.hpp:341-358).
            std::vector<double> g;
            {
                py::gil_scoped_release release;
                g = s.GetFullGradientFlat(enable_edge_gradients, (double)s.GetOOBValue());
            }
            py::array_t<double> out({nx, ny, nz, (int64_t)3});
            std::memcpy(out.mutable_data(), g.data(), g.size() * sizeof(double));
            return out;
        }, py::arg("enable_edge_gradients") = true)
        .def("ComputeLocalExtremaMapNumpy", [](const SignedDistanceField& s) {
            const int64_t nx = s.GetNumXCells(), ny = s.GetNumYCells(), nz = s.GetNumZCells();
            ::VoxelGrid::VoxelGrid<Eigen::Vector3d> map;
            {
                py::gil_scoped_release release;
                map = s.ComputeLocalExtremaMap();
            }
            py::array_t<double> out({nx, ny, nz, (int64_t)3});
            double* o = out.mutable_data();
            for (const Eigen::Vector3d& e : map.GetImmutableRawData()) { *o++ = e.x(); *o++ = e.y(); *o++ = e.z(); }
            return out;
        }, "ComputeLocalExtremaMap (sdf.cpp:23-207, on the GPU) as float64 [nx, ny, nz, 3]: grid-frame extremum of each cell's "
           "gradient walk, +inf where it leaves the grid")
        .def("ComputeLocalExtremaIndicesNumpy", [](const SignedDistanceField& s) {
            std::vector<uint32_t> idx;
            {
                py::gil_scoped_release release;
                idx = s.ComputeLocalExtremaIndices();
            }
            py::array_t<uint32_t> out({(py::ssize_t)s.GetNumXCells(), (py::ssize_t)s.GetNumYCells(), (py::ssize_t)s.GetNumZCells()});
            std::memcpy(out.mutable_data(), idx.data(), idx.size() * sizeof(uint32_t));
            return out;
        }, "the extremum of each cell as a linear index, uint32 [nx, ny, nz]; 0xFFFFFFFF where the walk leaves the grid")
        .def("GetFullGradientNumpyHost", [](const SignedDistanceField& s, bool enable_edge_gradients) {
            // the reference's per-voxel loop (sdf.hpp:341-358) on one host core: kept as the checker of the GPU path
            const int64_t nx = s.GetNumXCells(), ny = s.GetNumYCells(), nz = s.GetNumZCells();
            py::array_t<double> out({nx, ny, nz, (int64_t)3});
            double* p = out.mutable_data();
            const double oob = (double)s.GetOOBValue();
            for (int64_t x = 0; x < nx; x++) for (int64_t y = 0; y < ny; y++) for (int64_t z = 0; z < nz; z++) {
                const std::vector<double> g = s.GetGradient(x, y, z, enable_edge_gradients);
                for (int k = 0; k < 3; k++) *p++ = g.size() == 3 ? g[(size_t)k] : oob;
            }
            return out;
        }, py::arg("enable_edge_gradients") = true)
        // projection (reference sdf.hpp:996-1190): reference-named members, (x, y, z) forms; they raise what the reference throws
        // (RuntimeError for a flat / missing gradient and for the step limit, ValueError for "Index out of bounds" and NaN input)
        .def("ProjectOutOfCollision", [](const SignedDistanceField& s, double x, double y, double z, double stepsize_multiplier) {
            return ToTuple(s.ProjectOutOfCollision(x, y, z, stepsize_multiplier));
        }, py::arg("x"), py::arg("y"), py::arg("z"), py::arg("stepsize_multiplier") = 1.0 / 8.0)
        .def("ProjectOutOfCollisionToMinimumDistance", [](const SignedDistanceField& s, double x, double y, double z, double minimum_distance,
                                                          double stepsize_multiplier) {
            return ToTuple(s.ProjectOutOfCollisionToMinimumDistance(x, y, z, minimum_distance, stepsize_multiplier));
        }, py::arg("x"), py::arg("y"), py::arg("z"), py::arg("minimum_distance"), py::arg("stepsize_multiplier") = 1.0 / 8.0)
        .def("ProjectIntoValidVolume", [](const SignedDistanceField& s, double x, double y, double z) {
            return ToTuple(s.ProjectIntoValidVolume(x, y, z));
        }, py::arg("x"), py::arg("y"), py::arg("z"))
        .def("ProjectIntoValidVolumeToMinimumDistance", [](const SignedDistanceField& s, double x, double y, double z, double minimum_distance) {
            return ToTuple(s.ProjectIntoValidVolumeToMinimumDistance(x, y, z, minimum_distance));
        }, py::arg("x"), py::arg("y"), py::arg("z"), py::arg("minimum_distance"))
        .def("ProjectOutOfCollisionNumpyHost", [](const SignedDistanceField& s, const py::array_t<double, py::array::c_style | py::array::forcecast>& points,
                                                  double minimum_distance, double stepsize_multiplier, int max_steps, bool into_valid_volume_only) {
            // the counted host walk (SignedDistanceField::ProjectCounted4d) over [n, 3] points on one host core: the checker of
            // DeviceSignedDistanceField.ProjectBatch
            if (points.ndim() != 2 || points.shape(1) != 3) throw std::invalid_argument("points must be [n, 3] float64 (world frame)");
            const int64_t n = points.shape(0);
            (void)s.ProjectionStepLimit(stepsize_multiplier, max_steps);            // (argument check, also for n = 0)
            py::array_t<double> out({n, (int64_t)3});
            py::array_t<uint8_t> status({n});
            py::array_t<int32_t> steps({n});
            {
                py::gil_scoped_release release;
                const double* p = points.data();
                double* o = out.mutable_data();
                uint8_t* st = status.mutable_data();
                int32_t* sp = steps.mutable_data();
                for (int64_t i = 0; i < n; ++i) {
                    const SignedDistanceField::ProjectionResult r = s.ProjectCounted4d(Eigen::Vector4d(p[3 * i], p[3 * i + 1], p[3 * i + 2], 1.0),
                                                                                      minimum_distance, stepsize_multiplier, into_valid_volume_only,
                                                                                      max_steps);
                    o[3 * i] = r.location(0); o[3 * i + 1] = r.location(1); o[3 * i + 2] = r.location(2);
                    st[i] = r.status;
                    sp[i] = r.steps;
                }
            }
            return py::make_tuple(out, status, steps);
        }, py::arg("points"), py::arg("minimum_distance") = 0.0, py::arg("stepsize_multiplier") = 1.0 / 8.0, py::arg("max_steps") = 0,
           py::arg("into_valid_volume_only") = false,
           "n x ProjectOutOfCollisionToMinimumDistance3d (or ProjectIntoValidVolumeToMinimumDistance3d) counted, on one host core: "
           "(points [n, 3], status uint8 [n]: SDFGPU_PROJECT_*, steps int32 [n])") 
        // smooth and autodiff gradients, DistanceToBoundary (reference sdf.hpp:528-653, 963-988): (x, y, z) forms with the
        // reference's results (an empty list outside the grid) and exceptions (RuntimeError for a window too large for the field,
        // ValueError for a non-finite location or window)
        .def("GetSmoothGradient", [](const SignedDistanceField& s, double x, double y, double z, double nominal_window_size) {
            return s.GetSmoothGradient(x, y, z, nominal_window_size);
        }, py::arg("x"), py::arg("y"), py::arg("z"), py::arg("nominal_window_size"))
        .def("GetAutoDiffGradient", [](const SignedDistanceField& s, double x, double y, double z) { return s.GetAutoDiffGradient(x, y, z); },
             py::arg("x"), py::arg("y"), py::arg("z"))
        .def("DistanceToBoundary", [](const SignedDistanceField& s, double x, double y, double z) { return s.DistanceToBoundary(x, y, z); },
             py::arg("x"), py::arg("y"), py::arg("z"))
        .def("QueryGradientsNumpyHost", [](const SignedDistanceField& s, const py::array_t<double, py::array::c_style | py::array::forcecast>& points,
                                           int kind, double window) {
            // the host core (SignedDistanceField::QueryGradient4d) over [n, 3] points on one host core: the checker of
            // DeviceSignedDistanceField.QueryGradientsBatch
            if (points.ndim() != 2 || points.shape(1) != 3) throw std::invalid_argument("points must be [n, 3] float64 (world frame)");
            if (kind != SDFGPU_QUERY_DISTANCE_TO_BOUNDARY) (void)s.QueryGradient4d(Eigen::Vector4d(0.0, 0.0, 0.0, 1.0), kind, window);  // (argument check, also for n = 0)
            const int64_t n = points.shape(0);
            py::array_t<double> value({n});
            py::array_t<double> gradient({n, (int64_t)3});
            py::array_t<uint8_t> status({n});
            {
                py::gil_scoped_release release;
                const double* p = points.data();
                double* v = value.mutable_data();
                double* g = gradient.mutable_data();
                uint8_t* st = status.mutable_data();
                for (int64_t i = 0; i < n; ++i) {
                    const SignedDistanceField::GradientQueryResult r = s.QueryGradient4d(Eigen::Vector4d(p[3 * i], p[3 * i + 1], p[3 * i + 2], 1.0),
                                                                                          kind, window);
                    v[i] = r.value;
                    g[3 * i] = r.gradient[0]; g[3 * i + 1] = r.gradient[1]; g[3 * i + 2] = r.gradient[2];
                    st[i] = r.status;
                }
            }
            return py::make_tuple(value, gradient, status);
        }, py::arg("points"), py::arg("kind"), py::arg("window") = 0.0,
           "n x QueryGradient4d on one host core (kind SDFGPU_QUERY_*: 0 smooth with `window`, 1 autodiff, 2 distance to boundary): "
           "(value [n], gradient [n, 3], status uint8 [n]: SDFGPU_QUERY_*)")
        .def(py::init<const Isometry3d&, const std::string&, double, int64_t, int64_t, int64_t, float>(), py::arg("origin_transform"),
             py::arg("frame"), py::arg("resolution"), py::arg("x_cells"), py::arg("y_cells"), py::arg("z_cells"), py::arg("oob_value"),
             "a field of this geometry on the host, every cell oob_value")
        .def("SetRawDataNumpy", [](SignedDistanceField& s, const py::array_t<float, py::array::c_style | py::array::forcecast>& data) {
            // the whole [x][y][z] field at once (refused while locked)
            if (data.ndim() != 3 || data.shape(0) != s.GetNumXCells() || data.shape(1) != s.GetNumYCells() || data.shape(2) != s.GetNumZCells())
                throw std::invalid_argument("data must be float32 [x_cells, y_cells, z_cells]");
            float* dst = s.MutableDataForBuild();
            if (!dst) throw std::runtime_error("the field is locked");
            std::memcpy(dst, data.data(), (size_t)data.size() * sizeof(float));
        }, py::arg("data"));

    // the field left in HBM (include/sdf_tools/device_sdf.hpp): batched queries without the download.  A pybind thread is the
    // thread that owns the libsdfgpu context, so build, query and drop the object from the same Python thread.
    py::class_<sdf_tools::DeviceSignedDistanceField>(m, "DeviceSignedDistanceField")
        .def("GetResolution", &sdf_tools::DeviceSignedDistanceField::GetResolution)
        .def("GetFrame", &sdf_tools::DeviceSignedDistanceField::GetFrame)
        .def("GetNumXCells", &sdf_tools::DeviceSignedDistanceField::GetNumXCells)
        .def("GetNumYCells", &sdf_tools::DeviceSignedDistanceField::GetNumYCells)
        .def("GetNumZCells", &sdf_tools::DeviceSignedDistanceField::GetNumZCells)
        .def("GetExtrema", &sdf_tools::DeviceSignedDistanceField::GetExtrema)
        .def("HostCopyExists", &sdf_tools::DeviceSignedDistanceField::HostCopyExists)
        .def("DevicePointer", [](sdf_tools::DeviceSignedDistanceField& d) { return (uintptr_t)d.DevicePointer(); },
             "address of the [x][y][z] fp32 field in HBM (e.g. for torch / the *_device ABI)")
        .def(py::init<const Isometry3d&, const std::string&, double, int64_t, int64_t, int64_t, float>(), py::arg("origin_transform"),
             py::arg("frame"), py::arg("resolution"), py::arg("x_cells"), py::arg("y_cells"), py::arg("z_cells"), py::arg("oob_value"),
             "an empty field of this geometry in HBM (contents undefined until written through DevicePointer())")
        .def("Host", [](const sdf_tools::DeviceSignedDistanceField& d) { return d.Host(); }, "the reference's container (downloads once)")
        .def("ProjectBatch", [](const sdf_tools::DeviceSignedDistanceField& d, const py::array_t<double, py::array::c_style | py::array::forcecast>& points,
                                double minimum_distance, double stepsize_multiplier, int max_steps, bool into_valid_volume_only) {
            if (points.ndim() != 2 || points.shape(1) != 3) throw std::invalid_argument("points must be [n, 3] float64 (world frame)");
            const int64_t n = points.shape(0);
            py::array_t<double> out({n, (int64_t)3});
            py::array_t<uint8_t> status({n});
            py::array_t<int32_t> steps({n});
            {
                py::gil_scoped_release release;
                d.ProjectBatch(points.data(), n, minimum_distance, stepsize_multiplier, into_valid_volume_only, max_steps, out.mutable_data(),
                               status.mutable_data(), steps.mutable_data());
            }
            return py::make_tuple(out, status, steps);
        }, py::arg("points"), py::arg("minimum_distance") = 0.0, py::arg("stepsize_multiplier") = 1.0 / 8.0, py::arg("max_steps") = 0,
           py::arg("into_valid_volume_only") = false,
           "ProjectOutOfCollisionNumpyHost's walk for n points in one kernel (sdfgpu_project_points): (points [n, 3], status [n], steps [n])")
        .def("QueryGradientsBatch", [](const sdf_tools::DeviceSignedDistanceField& d, const py::array_t<double, py::array::c_style | py::array::forcecast>& points,
                                       int kind, double window) {
            if (points.ndim() != 2 || points.shape(1) != 3) throw std::invalid_argument("points must be [n, 3] float64 (world frame)");
            const int64_t n = points.shape(0);
            py::array_t<double> value({n});
            py::array_t<double> gradient({n, (int64_t)3});
            py::array_t<uint8_t> status({n});
            {
                py::gil_scoped_release release;
                d.QueryGradientsBatch(points.data(), n, kind, window, value.mutable_data(), gradient.mutable_data(), status.mutable_data());
            }
            return py::make_tuple(value, gradient, status);
        }, py::arg("points"), py::arg("kind"), py::arg("window") = 0.0,
           "QueryGradientsNumpyHost's answers for n points in one kernel (sdfgpu_query_gradients): (value [n], gradient [n, 3], status [n])")
        .def("QueryBatch", [](const sdf_tools::DeviceSignedDistanceField& d,
                              const py::array_t<double, py::array::c_style | py::array::forcecast>& points, bool enable_edge_gradients) {
            if (points.ndim() != 2 || points.shape(1) != 3) throw std::invalid_argument("points must be [n, 3] float64 (world frame)");
            const int64_t n = points.shape(0);
            py::array_t<double> dist({n}), grad({n, (int64_t)3});
            py::array_t<uint8_t> flags({n});
            {
                py::gil_scoped_release release;
                d.QueryBatch(points.data(), n, enable_edge_gradients, dist.mutable_data(), grad.mutable_data(), flags.mutable_data());
            }
            return py::make_tuple(dist, grad, flags);
        }, py::arg("points"), py::arg("enable_edge_gradients") = false,
           "n x EstimateDistance3d + GetGradient3d (sdf.hpp:947-953, :395-403) in one kernel: (distance [n], gradient [n, 3], flags [n]: "
           "bit 0 inside the grid, bit 1 gradient available)");

    py::class_<CollisionMapGrid> collision_grid(m, "CollisionMapGrid");
    DefSurfaces<CollisionMapGrid>(collision_grid);
    DefResample<CollisionMapGrid>(collision_grid);
    collision_grid
        .def("ExportForDisplay", [](const CollisionMapGrid& g, const Rgba& c, const Rgba& f, const Rgba& u) {
            return ReleasedMarker([&]() { return g.ExportForDisplay(ColorOf(c), ColorOf(f), ColorOf(u)); });
        }, py::arg("collision_color"), py::arg("free_color"), py::arg("unknown_color"),
             "(points float64 [n, 3], colors float32 [n, 4]) of the cells whose class colour has alpha > 0, in scan order")
        .def("ExportSurfacesForDisplay", [](const CollisionMapGrid& g, const Rgba& c, const Rgba& f, const Rgba& u) {
            return ReleasedMarker([&]() { return g.ExportSurfacesForDisplay(ColorOf(c), ColorOf(f), ColorOf(u)); });
        }, py::arg("collision_color"), py::arg("free_color"), py::arg("unknown_color"), "... of the surface cells (26-neighbour rule)")
        .def("ExportForSeparateDisplay", [](const CollisionMapGrid& g, const Rgba& c, const Rgba& f, const Rgba& u) {
            return ReleasedMarkerArray([&]() { return g.ExportForSeparateDisplay(ColorOf(c), ColorOf(f), ColorOf(u)); });
        }, py::arg("collision_color"), py::arg("free_color"), py::arg("unknown_color"), "[(ns, points, colors)] x 3: collision, free, unknown")
        .def("ExportSurfacesForSeparateDisplay", [](const CollisionMapGrid& g, const Rgba& c, const Rgba& f, const Rgba& u) {
            return ReleasedMarkerArray([&]() { return g.ExportSurfacesForSeparateDisplay(ColorOf(c), ColorOf(f), ColorOf(u)); });
        }, py::arg("collision_color"), py::arg("free_color"), py::arg("unknown_color"))
        .def("ExportConnectedComponentsForDisplay", [](const CollisionMapGrid& g, bool color_unknown_components) {
            return ReleasedMarker([&]() { return g.ExportConnectedComponentsForDisplay(color_unknown_components); });
        }, py::arg("color_unknown_components"))
        .def("ExportForDisplayInfo", [](const CollisionMapGrid& g, const Rgba& c, const Rgba& f, const Rgba& u) {
            return MarkerInfo(g.ExportForDisplay(ColorOf(c), ColorOf(f), ColorOf(u)));
        }, "header, ns, id, type, action, pose, scale and the element counts of ExportForDisplay");
    collision_grid
        .def(py::init<Isometry3d const&, std::string, double, int64_t, int64_t, int64_t, COLLISION_CELL const&>())
        .def("SetValue", [](CollisionMapGrid& g, int64_t x, int64_t y, int64_t z, const COLLISION_CELL& c) { return g.SetValue(x, y, z, c); })
        .def("SetValueByCoordinates", [](CollisionMapGrid& g, double x, double y, double z, const COLLISION_CELL& c) { return g.SetValue(x, y, z, c); })
        // wire formats (collision_map.cpp:21-62, :205-315)
        .def(py::init<>())
        .def("SerializeSelf", [](const CollisionMapGrid& g) { std::vector<uint8_t> b; g.SerializeSelf(b); return py::bytes(reinterpret_cast<const char*>(b.data()), b.size()); })
        .def_static("Deserialize", [](const py::bytes& data) { const std::string s = data; CollisionMapGrid g; g.DeserializeSelf(std::vector<uint8_t>(s.begin(), s.end()), 0); return g; })
        .def("SaveToFile", [](const CollisionMapGrid& g, const std::string& path, bool compress) { CollisionMapGrid::SaveToFile(g, path, compress); })
        .def_static("LoadFromFile", &CollisionMapGrid::LoadFromFile)
        .def("GetMessageRepresentation", [](const CollisionMapGrid& g) { return CollisionMapGrid::GetMessageRepresentation(g); })
        .def_static("LoadFromMessageRepresentation", &CollisionMapGrid::LoadFromMessageRepresentation)
        .def("GetFrame", &CollisionMapGrid::GetFrame)
        .def("GetResolution", &CollisionMapGrid::GetResolution)
        .def("GetRawData", &CollisionMapGrid::GetImmutableRawData, "Please don't mutate this")
        .def("GetValueByCoordinates", [](const CollisionMapGrid& g, double x, double y, double z) { const auto q = g.GetImmutable(x, y, z); return std::make_pair(q.first, q.second); },
             "Please don't mutate this", py::arg("x"), py::arg("y"), py::arg("z"))
        .def("GetValueByIndex", [](const CollisionMapGrid& g, int64_t x, int64_t y, int64_t z) { const auto q = g.GetImmutable(x, y, z); return std::make_pair(q.first, q.second); },
             "Please don't mutate this", py::arg("x_index"), py::arg("y_index"), py::arg("z_index"))
        .def("GetNumXCells", &CollisionMapGrid::GetNumXCells)
        .def("GetNumYCells", &CollisionMapGrid::GetNumYCells)
        .def("GetNumZCells", &CollisionMapGrid::GetNumZCells)
        .def("ExtractSignedDistanceField", &CollisionMapGrid::ExtractSignedDistanceField, py::call_guard<py::gil_scoped_release>())
        .def("ExtractSignedDistanceFieldDevice", [](const CollisionMapGrid& g, float oob_value, bool unknown_is_filled, bool add_virtual_border) {
                 auto r = g.ExtractSignedDistanceFieldDevice(oob_value, unknown_is_filled, add_virtual_border);
                 std::unique_ptr<sdf_tools::DeviceSignedDistanceField> field(new sdf_tools::DeviceSignedDistanceField(std::move(r.first)));
                 return py::make_tuple(py::cast(std::move(field)), r.second);
             }, "ExtractSignedDistanceField with the field left in HBM -> (DeviceSignedDistanceField, (max, min))")
        .def("ExtractSignedDistanceFieldViaPredicate", &CollisionMapGrid::ExtractSignedDistanceFieldViaPredicate,
             py::call_guard<py::gil_scoped_release>())
        // the reference's cell-predicate overload (sdf_generation.hpp:422-441) with a Python predicate on the cell
        .def("ExtractSignedDistanceFieldCellPredicate",
             [](const CollisionMapGrid& g, const std::function<bool(const COLLISION_CELL&)>& is_filled_fn, float oob_value) {
                 return sdf_generation::ExtractSignedDistanceField<COLLISION_CELL>(g, is_filled_fn, oob_value, g.GetFrame());
             }, py::arg("is_filled_fn"), py::arg("oob_value"))
        .def("SetOccupancyFromNumpy", [](CollisionMapGrid& g, const py::array_t<float, py::array::c_style | py::array::forcecast>& occ) {
            if (occ.ndim() != 3 || occ.shape(0) != g.GetNumXCells() || occ.shape(1) != g.GetNumYCells() || occ.shape(2) != g.GetNumZCells())
                throw std::invalid_argument("occupancy array must be [nx, ny, nz]");
            const float* p = occ.data();
            auto& cells = g.GetMutableRawData();
            for (size_t i = 0; i < cells.size(); i++) cells[i] = COLLISION_CELL(p[i]);
            g.InvalidateConnectedComponents();                      // (the cells' labels were just reset, as SetValue would)
        })
        // connected components on the GPU (collision_map.cpp:564-618); ExtractConnectedComponents stays C++-only: a list of
        // GRID_INDEX lists per component is not a usable Python value at 512^3 -- GetComponentsNumpy is the bulk accessor
        .def("UpdateConnectedComponents", &CollisionMapGrid::UpdateConnectedComponents, py::call_guard<py::gil_scoped_release>())
        .def("GetNumConnectedComponents", &CollisionMapGrid::GetNumConnectedComponents)
        .def("ComputeComponentTopology", &CollisionMapGrid::ComputeComponentTopology, py::arg("ignore_empty_components") = true,
             py::arg("recompute_connected_components") = true, py::arg("verbose") = false, py::call_guard<py::gil_scoped_release>(),
             "{component: (holes, voids)} on the GPU (collision_map.cpp:620-671; include/sdfgpu.h \"Component topology\")")
        .def("GetComponentsNumpy", [](const CollisionMapGrid& g) {
            py::array_t<uint32_t> out({(py::ssize_t)g.GetNumXCells(), (py::ssize_t)g.GetNumYCells(), (py::ssize_t)g.GetNumZCells()});
            uint32_t* o = out.mutable_data();
            const auto& cells = g.GetImmutableRawData();
            for (size_t i = 0; i < cells.size(); i++) o[i] = cells[i].component;
            return out;
        }, "the cells' component labels as uint32 [nx, ny, nz] (0 until UpdateConnectedComponents has run)");

    m.def("DecompressBytes", &ZlibHelpers::DecompressBytes);
    m.def("DeserializeFixedSizePODFloat", &arc_utilities::DeserializeFixedSizePOD<float>);
    m.def("DeserializeFixedSizePODd", &arc_utilities::DeserializeVectorOfDoubles);
    m.def("SetDevice", [](int device) { sdf_generation::GpuContext::DeviceIndex() = device; }, "GPU used by ExtractSignedDistanceField");
    m.def("SetNumGpus", [](int n) { sdf_generation::MultiGpuContext::SetNumGpus(n); },
          "n > 1: ExtractSignedDistanceField cuts the grid into x slabs over GPUs 0..n-1 (RCCL exchange); 1 = single GPU");

    py::class_<VoxelGridVecd>(m, "VoxelGrid")
        .def(py::init<>())
        .def("GetRawData", &VoxelGridVecd::GetImmutableRawData, "Please don't mutate this")
        .def("GetNumXCells", &VoxelGridVecd::GetNumXCells)
        .def("GetNumYCells", &VoxelGridVecd::GetNumYCells)
        .def("GetNumZCells", &VoxelGridVecd::GetNumZCells)
        .def("GetValueByCoordinates", [](const VoxelGridVecd& g, double x, double y, double z) { const auto q = g.GetImmutable(x, y, z); return std::make_pair(q.first, q.second); },
             "Please don't mutate this", py::arg("x"), py::arg("y"), py::arg("z"))
        .def("GetValueByIndex", [](const VoxelGridVecd& g, int64_t x, int64_t y, int64_t z) { const auto q = g.GetImmutable(x, y, z); return std::make_pair(q.first, q.second); },
             "Please don't mutate this", py::arg("x_index"), py::arg("y_index"), py::arg("z_index"))
        .def("SerializeSelf", [](const VoxelGridVecd& g) { std::vector<uint8_t> b; g.SerializeSelf(b, arc_utilities::SerializeVectorOfDoubles); return py::bytes(reinterpret_cast<const char*>(b.data()), b.size()); })
        .def("DeserializeSelf", [](VoxelGridVecd& g, const std::vector<uint8_t>& buffer, uint64_t current, py::object) {
            return g.DeserializeSelf(buffer, current, arc_utilities::DeserializeVectorOfDoubles); },
             "deserialize", py::arg("buffer"), py::arg("current"), py::arg("value_deserializer") = py::none());

    // ---- SDF_Builder and the message mirrors it reads (include/sdf_tools/sdf_builder.hpp, planning_scene.hpp) ------------------------------
    py::class_<geometry_msgs::Pose>(m, "Pose")
        .def(py::init([](const std::array<double, 3>& position, const std::array<double, 4>& orientation_xyzw) {
            geometry_msgs::Pose p;
            p.position.x = position[0]; p.position.y = position[1]; p.position.z = position[2];
            p.orientation.x = orientation_xyzw[0]; p.orientation.y = orientation_xyzw[1]; p.orientation.z = orientation_xyzw[2]; p.orientation.w = orientation_xyzw[3];
            return p;
        }), py::arg("position") = std::array<double, 3>{0.0, 0.0, 0.0}, py::arg("orientation_xyzw") = std::array<double, 4>{0.0, 0.0, 0.0, 1.0})
        .def("matrix", [](const geometry_msgs::Pose& p) {
            py::array_t<double> out({4, 4});
            sdf_tools::PoseToMatrix(p, out.mutable_data());
            return out;
        }, "row-major 4 x 4 as SDF_Builder passes it to the rasteriser");
    py::class_<shape_msgs::SolidPrimitive>(m, "SolidPrimitive")
        .def(py::init([](int type, const std::vector<double>& dimensions) {
            shape_msgs::SolidPrimitive s;
            s.type = (uint8_t)type; s.dimensions = dimensions;
            return s;
        }), py::arg("type") = 0, py::arg("dimensions") = std::vector<double>())
        .def_readwrite("type", &shape_msgs::SolidPrimitive::type)
        .def_readwrite("dimensions", &shape_msgs::SolidPrimitive::dimensions)
        .def_property_readonly_static("BOX", [](py::object) { return (int)shape_msgs::SolidPrimitive::BOX; })
        .def_property_readonly_static("SPHERE", [](py::object) { return (int)shape_msgs::SolidPrimitive::SPHERE; })
        .def_property_readonly_static("CYLINDER", [](py::object) { return (int)shape_msgs::SolidPrimitive::CYLINDER; })
        .def_property_readonly_static("CONE", [](py::object) { return (int)shape_msgs::SolidPrimitive::CONE; });
    py::class_<shape_msgs::MeshTriangle>(m, "MeshTriangle")
        .def(py::init([](const std::array<uint32_t, 3>& vertex_indices) {
            shape_msgs::MeshTriangle t;
            for (int i = 0; i < 3; ++i) t.vertex_indices[i] = vertex_indices[i];
            return t;
        }), py::arg("vertex_indices") = std::array<uint32_t, 3>{0, 0, 0})
        .def_property("vertex_indices", [](const shape_msgs::MeshTriangle& t) { return std::array<uint32_t, 3>{t.vertex_indices[0], t.vertex_indices[1], t.vertex_indices[2]}; },
                      [](shape_msgs::MeshTriangle& t, const std::array<uint32_t, 3>& v) { for (int i = 0; i < 3; ++i) t.vertex_indices[i] = v[i]; });
    py::class_<shape_msgs::Mesh>(m, "Mesh")
        .def(py::init<>())
        .def_readwrite("triangles", &shape_msgs::Mesh::triangles)
        .def_property_readonly("vertices", [](const shape_msgs::Mesh& mesh) {
            py::array_t<double> out({(py::ssize_t)mesh.vertices.size(), (py::ssize_t)3});
            if (!mesh.vertices.empty()) std::memcpy(out.mutable_data(), mesh.vertices.data(), mesh.vertices.size() * sizeof(geometry_msgs::Point));
            return out;
        }, "a copy of the vertices as a numpy array [n, 3]; set them with set_vertices")
        .def("set_vertices", [](shape_msgs::Mesh& mesh, const py::array_t<double, py::array::c_style | py::array::forcecast>& vertices) {
            if (vertices.ndim() != 2 || vertices.shape(1) != 3) throw std::invalid_argument("vertices must be [n, 3]");
            mesh.vertices.resize((size_t)vertices.shape(0));
            for (size_t i = 0; i < mesh.vertices.size(); ++i) {
                mesh.vertices[i].x = vertices.data()[3 * i]; mesh.vertices[i].y = vertices.data()[3 * i + 1]; mesh.vertices[i].z = vertices.data()[3 * i + 2];
            }
        }, py::arg("vertices"), "vertices as a numpy array [n, 3] in the mesh frame")
        .def("set_triangles", [](shape_msgs::Mesh& mesh, const py::array_t<uint32_t, py::array::c_style | py::array::forcecast>& triangles) {
            if (triangles.ndim() != 2 || triangles.shape(1) != 3) throw std::invalid_argument("triangles must be [n, 3]");
            mesh.triangles.resize((size_t)triangles.shape(0));
            for (size_t i = 0; i < mesh.triangles.size(); ++i)
                for (int k = 0; k < 3; ++k) mesh.triangles[i].vertex_indices[k] = triangles.data()[3 * i + k];
        }, py::arg("triangles"), "triangles as a numpy array [n, 3] of vertex indices");
    py::class_<shape_msgs::Plane>(m, "Plane")
        .def(py::init([](const std::array<double, 4>& coef) {
            shape_msgs::Plane p;
            for (int i = 0; i < 4; ++i) p.coef[i] = coef[i];
            return p;
        }), py::arg("coef") = std::array<double, 4>{0.0, 0.0, 0.0, 0.0})
        .def_property("coef", [](const shape_msgs::Plane& p) { return std::array<double, 4>{p.coef[0], p.coef[1], p.coef[2], p.coef[3]}; },
                      [](shape_msgs::Plane& p, const std::array<double, 4>& c) { for (int i = 0; i < 4; ++i) p.coef[i] = c[i]; });
    py::class_<moveit_msgs::CollisionObject>(m, "CollisionObject")
        .def(py::init<>())
        .def_readwrite("id", &moveit_msgs::CollisionObject::id)
        .def_readwrite("primitives", &moveit_msgs::CollisionObject::primitives)
        .def_readwrite("primitive_poses", &moveit_msgs::CollisionObject::primitive_poses)
        .def_readwrite("meshes", &moveit_msgs::CollisionObject::meshes)
        .def_readwrite("mesh_poses", &moveit_msgs::CollisionObject::mesh_poses)
        .def_readwrite("planes", &moveit_msgs::CollisionObject::planes)
        .def_readwrite("plane_poses", &moveit_msgs::CollisionObject::plane_poses);
    py::class_<octomap_msgs::OctomapBoxesWithPose>(m, "OctomapBoxesWithPose")
        .def(py::init<>())
        .def_readwrite("origin", &octomap_msgs::OctomapBoxesWithPose::origin)
        .def("SetBoxesNumpy", [](octomap_msgs::OctomapBoxesWithPose& o, const py::array_t<double, py::array::c_style | py::array::forcecast>& centers,
                                 const py::array_t<double, py::array::c_style | py::array::forcecast>& sizes) {
            if (centers.ndim() != 2 || centers.shape(1) != 3 || sizes.ndim() != 1 || sizes.shape(0) != centers.shape(0))
                throw std::invalid_argument("centers must be [n, 3] and sizes [n]");
            const size_t n = (size_t)sizes.shape(0);
            o.octomap.centers.resize(n);
            o.octomap.sizes.assign(sizes.data(), sizes.data() + n);
            for (size_t i = 0; i < n; ++i) { o.octomap.centers[i].x = centers.data()[3 * i]; o.octomap.centers[i].y = centers.data()[3 * i + 1]; o.octomap.centers[i].z = centers.data()[3 * i + 2]; }
        }, py::arg("centers"), py::arg("sizes"), "occupied leaves as boxes: centres [n, 3] and edge lengths [n] in the octomap's frame")
        .def("NumBoxes", [](const octomap_msgs::OctomapBoxesWithPose& o) { return o.octomap.centers.size(); });
    py::class_<moveit_msgs::PlanningSceneWorld>(m, "PlanningSceneWorld")
        .def(py::init<>())
        .def_readwrite("collision_objects", &moveit_msgs::PlanningSceneWorld::collision_objects)
        .def_readwrite("octomap", &moveit_msgs::PlanningSceneWorld::octomap);
    py::class_<moveit_msgs::PlanningScene>(m, "PlanningScene")
        .def(py::init<>())
        .def_readwrite("name", &moveit_msgs::PlanningScene::name)
        .def_readwrite("world", &moveit_msgs::PlanningScene::world);
    m.attr("USE_CACHED") = (int)sdf_tools::USE_CACHED;
    m.attr("USE_ONLY_OCTOMAP") = (int)sdf_tools::USE_ONLY_OCTOMAP;
    m.attr("USE_ONLY_COLLISION_OBJECTS") = (int)sdf_tools::USE_ONLY_COLLISION_OBJECTS;
    m.attr("USE_FULL_PLANNING_SCENE") = (int)sdf_tools::USE_FULL_PLANNING_SCENE;
    m.attr("MESH_FILL_SURFACE") = (int)sdf_tools::MESH_FILL_SURFACE;
    m.attr("MESH_FILL_SOLID") = (int)sdf_tools::MESH_FILL_SOLID;
    const auto collision_map_numpy = [](const VoxelGrid::VoxelGrid<uint8_t>& g) {
        py::array_t<uint8_t> out({g.GetNumXCells(), g.GetNumYCells(), g.GetNumZCells()});
        std::memcpy(out.mutable_data(), g.GetImmutableRawData().data(), g.GetImmutableRawData().size());
        return out;
    };
    py::class_<sdf_tools::SDF_Builder>(m, "SDF_Builder")
        .def(py::init<>())
        .def(py::init<const Isometry3d&, const std::string&, double, double, double, double, float, const sdf_tools::SDF_Builder::PlanningSceneSource&>(),
             py::arg("origin_transform"), py::arg("frame"), py::arg("x_size"), py::arg("y_size"), py::arg("z_size"), py::arg("resolution"),
             py::arg("OOB_value"), py::arg("planning_scene_source") = sdf_tools::SDF_Builder::PlanningSceneSource())
        .def(py::init<const std::string&, double, double, double, double, float, const sdf_tools::SDF_Builder::PlanningSceneSource&>(),
             py::arg("frame"), py::arg("x_size"), py::arg("y_size"), py::arg("z_size"), py::arg("resolution"), py::arg("OOB_value"),
             py::arg("planning_scene_source") = sdf_tools::SDF_Builder::PlanningSceneSource())
        .def("UpdatePlanningSceneFromMessage", &sdf_tools::SDF_Builder::UpdatePlanningSceneFromMessage)
        .def("SetMeshFill", [](sdf_tools::SDF_Builder& b, int mode) { b.SetMeshFill((uint8_t)mode); }, py::arg("mode"),
             "MESH_FILL_SURFACE (default) or MESH_FILL_SOLID: closed meshes are filled inside as well")
        .def("SetObjectMeshFill", [](sdf_tools::SDF_Builder& b, const std::string& object_id, int mode) { b.SetObjectMeshFill(object_id, (uint8_t)mode); },
             py::arg("object_id"), py::arg("mode"), "the mode for the meshes of one collision object, by its id")
        .def("UpdateSDF", [](sdf_tools::SDF_Builder& b, int mode) { return b.UpdateSDF((uint8_t)mode); })
        .def("GetCachedSDF", [](const sdf_tools::SDF_Builder& b) { return b.GetCachedSDF(); })
        .def("UpdateCollisionMap", [collision_map_numpy](sdf_tools::SDF_Builder& b, int mode) { return collision_map_numpy(b.UpdateCollisionMap((uint8_t)mode)); },
             "the VoxelGrid<uint8_t> of the reference as uint8 [nx, ny, nz]")
        .def("GetCachedCollisionMap", [collision_map_numpy](const sdf_tools::SDF_Builder& b) { return collision_map_numpy(b.GetCachedCollisionMap()); })
        .def("UpdateSDFDevice", [](sdf_tools::SDF_Builder& b, int mode) { return b.UpdateSDFDevice((uint8_t)mode); })
        .def("UpdateTaggedCollisionMap", [](sdf_tools::SDF_Builder& b, int mode) { return b.UpdateTaggedCollisionMap((uint8_t)mode); });
    // The sparse map that stays on the GPU.  Batch forms take numpy: locations float64 [n, 3], records uint64 [n] (a COLLISION_CELL's
    // 8 bytes: occupancy in the low word, component in the high one) or one COLLISION_CELL for the whole batch.
    using DshGrid = sdf_tools::DynamicSpatialHashedCollisionMapGrid;
    auto dsh_cells = [](const py::object& value, size_t n) {
        std::vector<COLLISION_CELL> cells;
        if (py::isinstance<COLLISION_CELL>(value)) { cells.push_back(value.cast<COLLISION_CELL>()); return cells; }
        const auto records = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>::ensure(value);
        if (!records || (size_t)records.size() != n) throw std::invalid_argument("values: one COLLISION_CELL, or uint64 records, one per location");
        cells.resize(n);
        if (n) std::memcpy(static_cast<void*>(cells.data()), records.data(), n * 8);
        return cells;
    };
    auto dsh_locations = [](const py::array_t<double, py::array::c_style | py::array::forcecast>& locations) {
        if (locations.size() % 3) throw std::invalid_argument("locations: float64 [n, 3]");
        return std::vector<double>(locations.data(), locations.data() + locations.size());
    };
    auto dsh_statuses = [](const std::vector<VoxelGrid::SET_STATUS>& statuses) {
        py::array_t<uint8_t> out((py::ssize_t)statuses.size());
        for (size_t i = 0; i < statuses.size(); ++i) out.mutable_data()[i] = (uint8_t)statuses[i];
        return out;
    };
    auto dsh_casts = [](const std::vector<DshGrid::RayCast>& casts) {
        const py::ssize_t n = (py::ssize_t)casts.size();
        py::array_t<uint8_t> status(n);
        py::array_t<int64_t> cell({n, (py::ssize_t)3});
        py::array_t<uint64_t> record(n);
        py::array_t<uint32_t> found(n), step(n);
        py::array_t<double> t(n), distance(n);
        for (py::ssize_t i = 0; i < n; ++i) {
            const DshGrid::RayCast& c = casts[(size_t)i];
            status.mutable_data()[i] = (uint8_t)c.status;
            cell.mutable_data()[3 * i] = c.cell.x; cell.mutable_data()[3 * i + 1] = c.cell.y; cell.mutable_data()[3 * i + 2] = c.cell.z;
            std::memcpy(record.mutable_data() + i, static_cast<const void*>(&c.value), 8);
            found.mutable_data()[i] = (uint32_t)c.found;
            step.mutable_data()[i] = c.step;
            t.mutable_data()[i] = c.t;
            distance.mutable_data()[i] = c.distance;
        }
        py::dict d;
        d["status"] = status; d["cell"] = cell; d["record"] = record; d["found"] = found; d["t"] = t; d["step"] = step; d["distance"] = distance;
        return d;
    };
    py::class_<DshGrid>(m, "DynamicSpatialHashedCollisionMapGrid")
        .def(py::init<>())
        .def(py::init<std::string, double, int64_t, int64_t, int64_t, COLLISION_CELL>(), py::arg("frame"), py::arg("resolution"), py::arg("chunk_x_size"),
             py::arg("chunk_y_size"), py::arg("chunk_z_size"), py::arg("OOB_value"))
        .def(py::init<Isometry3d, std::string, double, int64_t, int64_t, int64_t, COLLISION_CELL, uint64_t>(), py::arg("origin_transform"), py::arg("frame"),
             py::arg("resolution"), py::arg("chunk_x_size"), py::arg("chunk_y_size"), py::arg("chunk_z_size"), py::arg("OOB_value"), py::arg("byte_limit") = 0)
        .def("IsInitialized", &DshGrid::IsInitialized)
        .def("AreComponentsValid", &DshGrid::AreComponentsValid)
        .def("GetOriginTransform", &DshGrid::GetOriginTransform)
        .def("GetFrame", &DshGrid::GetFrame)
        .def("GetResolution", &DshGrid::GetResolution)
        .def("Get", [](const DshGrid& g, double x, double y, double z) { const auto r = g.Get(x, y, z); return py::make_tuple(r.first, (int)r.second); })
        .def("SetCell", [](DshGrid& g, double x, double y, double z, COLLISION_CELL v) { return (int)g.SetCell(x, y, z, v); })
        .def("SetChunk", [](DshGrid& g, double x, double y, double z, COLLISION_CELL v) { return (int)g.SetChunk(x, y, z, v); })
        .def("SetCells", [=](DshGrid& g, const py::array_t<double, py::array::c_style | py::array::forcecast>& locations, const py::object& values) {
            const std::vector<double> loc = dsh_locations(locations);
            return dsh_statuses(g.SetCells(loc, dsh_cells(values, loc.size() / 3)));
        }, py::arg("locations"), py::arg("values"), "uint8 statuses; as if applied one after the other in list order")
        .def("SetChunks", [=](DshGrid& g, const py::array_t<double, py::array::c_style | py::array::forcecast>& locations, const py::object& values) {
            const std::vector<double> loc = dsh_locations(locations);
            return dsh_statuses(g.SetChunks(loc, dsh_cells(values, loc.size() / 3)));
        }, py::arg("locations"), py::arg("values"))
        .def("GetBatch", [=](const DshGrid& g, const py::array_t<double, py::array::c_style | py::array::forcecast>& locations) {
            const auto got = g.GetBatch(dsh_locations(locations));
            py::array_t<uint64_t> records((py::ssize_t)got.first.size());
            py::array_t<uint8_t> statuses((py::ssize_t)got.second.size());
            if (!got.first.empty()) std::memcpy(records.mutable_data(), static_cast<const void*>(got.first.data()), got.first.size() * 8);
            for (size_t i = 0; i < got.second.size(); ++i) statuses.mutable_data()[i] = (uint8_t)got.second[i];
            return py::make_tuple(records, statuses);
        }, py::arg("locations"), "(records uint64 [n], statuses uint8 [n])")
        .def("InsertPointCloud", [](DshGrid& g, const py::array_t<float, py::array::c_style | py::array::forcecast>& points, COLLISION_CELL value) {
            if (points.size() % 3) throw std::invalid_argument("points: float32 [n, 3]");
            return g.InsertPointCloud(std::vector<float>(points.data(), points.data() + points.size()), value);
        }, py::arg("points"), py::arg("value"), "cell sets of one value; returns how many points were set")
        .def("InsertPointCloudRays", [](DshGrid& g, const py::array_t<float, py::array::c_style | py::array::forcecast>& points,
                                        const std::array<double, 3>& sensor_origin, double max_range, COLLISION_CELL free_value, COLLISION_CELL filled_value) {
            if (points.size() % 3) throw std::invalid_argument("points: float32 [n, 3]");
            const sdfgpu_dsh_ray_counts c = g.InsertPointCloudRays(std::vector<float>(points.data(), points.data() + points.size()),
                                                                   Eigen::Vector3d(sensor_origin[0], sensor_origin[1], sensor_origin[2]), max_range, free_value, filled_value);
            py::dict d;
            d["rays_hit"] = c.rays_hit; d["rays_truncated"] = c.rays_truncated; d["rays_skipped"] = c.rays_skipped;
            d["cells_carved"] = c.cells_carved; d["new_chunks"] = c.new_chunks;
            return d;
        }, py::arg("points"), py::arg("sensor_origin"), py::arg("max_range"), py::arg("free_value"), py::arg("filled_value"),
           "one frame of sensor rays: free space carved up to each point, then the points filled; returns the frame's counts")
        .def("FusePointCloudRays", [](DshGrid& g, const py::array_t<float, py::array::c_style | py::array::forcecast>& points,
                                      const std::array<double, 3>& sensor_origin, double max_range, float prob_hit, float prob_miss, float clamp_min, float clamp_max) {
            if (points.size() % 3) throw std::invalid_argument("points: float32 [n, 3]");
            DshGrid::SensorModel model;
            model.prob_hit = prob_hit; model.prob_miss = prob_miss; model.clamp_min = clamp_min; model.clamp_max = clamp_max;
            const sdfgpu_dsh_ray_counts c = g.FusePointCloudRays(std::vector<float>(points.data(), points.data() + points.size()),
                                                                 Eigen::Vector3d(sensor_origin[0], sensor_origin[1], sensor_origin[2]), max_range, model);
            py::dict d;
            d["rays_hit"] = c.rays_hit; d["rays_truncated"] = c.rays_truncated; d["rays_skipped"] = c.rays_skipped;
            d["cells_carved"] = c.cells_carved; d["new_chunks"] = c.new_chunks;
            return d;
        }, py::arg("points"), py::arg("sensor_origin"), py::arg("max_range"), py::arg("prob_hit") = 0.7f, py::arg("prob_miss") = 0.4f, py::arg("clamp_min") = 0.12f,
           py::arg("clamp_max") = 0.97f,
           "one frame of sensor rays fused into the occupancies: each passed cell updated once with prob_miss, each hit cell once with prob_hit; returns the counts")
        .def("CastRays", [=](const DshGrid& g, const py::array_t<float, py::array::c_style | py::array::forcecast>& points,
                             const std::array<double, 3>& sensor_origin, double max_range, bool unknown_is_filled, bool skip_first, bool skip_last) {
            if (points.size() % 3) throw std::invalid_argument("points: float32 [n, 3]");
            return dsh_casts(g.CastRays(std::vector<float>(points.data(), points.data() + points.size()),
                                        Eigen::Vector3d(sensor_origin[0], sensor_origin[1], sensor_origin[2]), max_range, unknown_is_filled, skip_first, skip_last));
        }, py::arg("points"), py::arg("sensor_origin"), py::arg("max_range"), py::arg("unknown_is_filled"), py::arg("skip_first") = false,
           py::arg("skip_last") = false,
           "the first blocking cell of each ray sensor -> point: a dict of arrays (status uint8, cell int64 [n, 3], record uint64, found, t, step, distance)")
        .def("CastSegments", [=](const DshGrid& g, const py::array_t<double, py::array::c_style | py::array::forcecast>& starts,
                                 const py::array_t<double, py::array::c_style | py::array::forcecast>& ends, double max_range, bool unknown_is_filled,
                                 bool skip_first, bool skip_last) {
            return dsh_casts(g.CastSegments(dsh_locations(starts), dsh_locations(ends), max_range, unknown_is_filled, skip_first, skip_last));
        }, py::arg("starts"), py::arg("ends"), py::arg("max_range"), py::arg("unknown_is_filled"), py::arg("skip_first") = false, py::arg("skip_last") = false,
           "the first blocking cell of each segment start -> end (float64 [n, 3] each): the dict of CastRays")
        .def("CastRay", [=](const DshGrid& g, const std::array<double, 3>& origin, const std::array<double, 3>& end, double max_range, bool unknown_is_filled,
                            bool skip_first, bool skip_last) {
            return dsh_casts({g.CastRay(Eigen::Vector3d(origin[0], origin[1], origin[2]), Eigen::Vector3d(end[0], end[1], end[2]), max_range, unknown_is_filled,
                                        skip_first, skip_last)});
        }, py::arg("origin"), py::arg("end"), py::arg("max_range"), py::arg("unknown_is_filled"), py::arg("skip_first") = false, py::arg("skip_last") = false,
           "one ray: the dict of CastRays with arrays of length 1")
        .def("ExtractFrontierCells", [](const DshGrid& g, const py::object& lower, int64_t nx, int64_t ny, int64_t nz, bool use_26) {
            std::vector<VoxelGrid::GRID_INDEX> cells;
            if (lower.is_none()) {
                cells = g.ExtractFrontierCells(use_26);
            } else {
                const std::array<int64_t, 3> at = lower.cast<std::array<int64_t, 3>>();
                cells = g.ExtractFrontierCells(VoxelGrid::GRID_INDEX(at[0], at[1], at[2]), nx, ny, nz, use_26);
            }
            py::array_t<int64_t> out({(py::ssize_t)cells.size(), (py::ssize_t)3});
            for (size_t i = 0; i < cells.size(); ++i) {
                out.mutable_data()[3 * i] = cells[i].x; out.mutable_data()[3 * i + 1] = cells[i].y; out.mutable_data()[3 * i + 2] = cells[i].z;
            }
            return out;
        }, py::arg("lower_index") = py::none(), py::arg("nx") = 0, py::arg("ny") = 0, py::arg("nz") = 0, py::arg("use_26") = false,
           "the frontier cells (free, with an unknown neighbour) of the whole map, or of the nx x ny x nz cells from lower_index on: int64 [n, 3] global cells")
        .def("ExtractFrontierWindowBits", [](const DshGrid& g, const std::array<int64_t, 3>& lower, int64_t nx, int64_t ny, int64_t nz, bool use_26) {
            const std::vector<uint32_t> bits = g.ExtractFrontierWindowBits(VoxelGrid::GRID_INDEX(lower[0], lower[1], lower[2]), nx, ny, nz, use_26);
            py::array_t<uint32_t> out((py::ssize_t)bits.size());
            if (!bits.empty()) std::memcpy(out.mutable_data(), bits.data(), bits.size() * 4);
            return out;
        }, py::arg("lower_index"), py::arg("nx"), py::arg("ny"), py::arg("nz"), py::arg("use_26") = false,
           "the window's frontier cells as a bit field: uint32 [ceil(nx ny nz / 32)], bit (x ny + y) nz + z")
        .def("ExtractFrontierClusters", [](const DshGrid& g, const std::array<int64_t, 3>& lower, int64_t nx, int64_t ny, int64_t nz, int64_t min_cells, bool use_26) {
            const std::vector<DshGrid::FrontierCluster> clusters =
                g.ExtractFrontierClusters(VoxelGrid::GRID_INDEX(lower[0], lower[1], lower[2]), nx, ny, nz, min_cells, use_26);
            const py::ssize_t n = (py::ssize_t)clusters.size();
            py::array_t<uint32_t> label(n);
            py::array_t<int64_t> cells(n), lo({n, (py::ssize_t)3}), hi({n, (py::ssize_t)3});
            py::array_t<double> centroid({n, (py::ssize_t)3});
            for (py::ssize_t i = 0; i < n; ++i) {
                const DshGrid::FrontierCluster& c = clusters[(size_t)i];
                label.mutable_data()[i] = c.label;
                cells.mutable_data()[i] = c.cells;
                lo.mutable_data()[3 * i] = c.lower.x; lo.mutable_data()[3 * i + 1] = c.lower.y; lo.mutable_data()[3 * i + 2] = c.lower.z;
                hi.mutable_data()[3 * i] = c.upper.x; hi.mutable_data()[3 * i + 1] = c.upper.y; hi.mutable_data()[3 * i + 2] = c.upper.z;
                centroid.mutable_data()[3 * i] = c.centroid.x(); centroid.mutable_data()[3 * i + 1] = c.centroid.y(); centroid.mutable_data()[3 * i + 2] = c.centroid.z();
            }
            py::dict d;
            d["label"] = label; d["cells"] = cells; d["lower"] = lo; d["upper"] = hi; d["centroid"] = centroid;
            return d;
        }, py::arg("lower_index"), py::arg("nx"), py::arg("ny"), py::arg("nz"), py::arg("min_cells") = 1, py::arg("use_26") = true,
           "the 6-connected pieces of the window's frontier with at least min_cells cells: a dict of arrays (label, cells, lower and upper int64 [n, 3], centroid float64 [n, 3])")
        .def("__copy__", [](const DshGrid& g) { return DshGrid(g); }, "the C++ copy: another name for the SAME device map (what one copy sets, the other reads)")
        .def("UpdateConnectedComponents", &DshGrid::UpdateConnectedComponents, py::arg("unknown_apart") = false,
             "labels the connected components of the whole map in place (the component word of every record); returns K, without a launch while the map is valid under the same rule")
        .def("GetNumConnectedComponents", &DshGrid::GetNumConnectedComponents, "(K of the last update, whether it still holds)")
        .def("update_components", [](DshGrid& g, uint32_t flags) {
            if (flags & ~(uint32_t)SDFGPU_DSH_COMPONENTS_UNKNOWN_APART) throw std::invalid_argument("update_components knows the flag DSH_COMPONENTS_UNKNOWN_APART");
            return g.UpdateConnectedComponents((flags & SDFGPU_DSH_COMPONENTS_UNKNOWN_APART) != 0);
        }, py::arg("flags") = 0, "UpdateConnectedComponents under the C ABI's flags (0, or DSH_COMPONENTS_UNKNOWN_APART = 1); returns K")
        .def("components_info", [](const DshGrid& g) {
            uint32_t count = 0, flags = 0;
            int valid = 0;
            if (g.IsInitialized()) {
                const std::lock_guard<std::mutex> lock(g.Context()->mutex);
                if (sdfgpu_dsh_components_info(g.DeviceMapHandle(), &count, &flags, &valid) != SDFGPU_OK) throw std::runtime_error("sdfgpu_dsh_components_info failed");
            }
            return py::make_tuple(count, flags, valid != 0);
        }, "(K of the last update, the flags it ran under, whether nothing has changed the map's content since): what the map keeps, host-only")
        .def("RemoveChunk", [](DshGrid& g, double x, double y, double z) { return g.RemoveChunk(x, y, z); })
        .def("RemoveChunks", [=](DshGrid& g, const py::array_t<double, py::array::c_style | py::array::forcecast>& locations) {
            const std::vector<bool> removed = g.RemoveChunks(dsh_locations(locations));
            py::array_t<uint8_t> out((py::ssize_t)removed.size());
            for (size_t i = 0; i < removed.size(); ++i) out.mutable_data()[i] = removed[i] ? 1 : 0;
            return out;
        }, py::arg("locations"), "uint8 statuses (1 = removed); as if applied one after the other in list order")
        .def("RetainBox", [](DshGrid& g, const std::array<int64_t, 3>& lower, int64_t nx, int64_t ny, int64_t nz) {
            return g.RetainBox(VoxelGrid::GRID_INDEX(lower[0], lower[1], lower[2]), nx, ny, nz);
        }, py::arg("lower_index"), py::arg("nx"), py::arg("ny"), py::arg("nz"), "removes every chunk that holds no cell of the box; returns how many")
        .def("RemoveBox", [](DshGrid& g, const std::array<int64_t, 3>& lower, int64_t nx, int64_t ny, int64_t nz) {
            return g.RemoveBox(VoxelGrid::GRID_INDEX(lower[0], lower[1], lower[2]), nx, ny, nz);
        }, py::arg("lower_index"), py::arg("nx"), py::arg("ny"), py::arg("nz"), "removes every chunk that holds a cell of the box; returns how many")
        .def("Clear", &DshGrid::Clear)
        .def("ShrinkToFit", &DshGrid::ShrinkToFit, py::arg("spare_chunks") = 0)
        .def("ExtractCollisionMapGrid", [](const DshGrid& g, const std::array<int64_t, 3>& lower, int64_t nx, int64_t ny, int64_t nz) {
            return g.ExtractCollisionMapGrid(VoxelGrid::GRID_INDEX(lower[0], lower[1], lower[2]), nx, ny, nz);
        }, py::arg("lower_index"), py::arg("nx"), py::arg("ny"), py::arg("nz"))
        .def("ExtractWindowRecords", [](const DshGrid& g, const std::array<int64_t, 3>& lower, int64_t nx, int64_t ny, int64_t nz) {
            const CollisionMapGrid grid = g.ExtractCollisionMapGrid(VoxelGrid::GRID_INDEX(lower[0], lower[1], lower[2]), nx, ny, nz);
            py::array_t<uint64_t> out({nx, ny, nz});
            std::memcpy(out.mutable_data(), static_cast<const void*>(grid.GetImmutableRawData().data()), (size_t)(nx * ny * nz) * 8);
            return out;
        }, py::arg("lower_index"), py::arg("nx"), py::arg("ny"), py::arg("nz"), "the window's records as uint64 [nx, ny, nz]")
        .def("ExtractSignedDistanceField", [](const DshGrid& g, const std::array<int64_t, 3>& lower, int64_t nx, int64_t ny, int64_t nz, float oob_value,
                                              bool unknown_is_filled, bool add_virtual_border) {
            return g.ExtractSignedDistanceField(VoxelGrid::GRID_INDEX(lower[0], lower[1], lower[2]), nx, ny, nz, oob_value, unknown_is_filled, add_virtual_border);
        }, py::arg("lower_index"), py::arg("nx"), py::arg("ny"), py::arg("nz"), py::arg("oob_value"), py::arg("unknown_is_filled"), py::arg("add_virtual_border"))
        .def("ExtractSignedDistanceFieldDevice", [](const DshGrid& g, const std::array<int64_t, 3>& lower, int64_t nx, int64_t ny, int64_t nz, float oob_value,
                                                    bool unknown_is_filled, bool add_virtual_border) {
            return g.ExtractSignedDistanceFieldDevice(VoxelGrid::GRID_INDEX(lower[0], lower[1], lower[2]), nx, ny, nz, oob_value, unknown_is_filled, add_virtual_border);
        }, py::arg("lower_index"), py::arg("nx"), py::arg("ny"), py::arg("nz"), py::arg("oob_value"), py::arg("unknown_is_filled"), py::arg("add_virtual_border"))
        .def("GetCounts", [](const DshGrid& g) {
            const sdfgpu_dsh_counts c = g.GetCounts();
            py::dict d;
            d["chunk_filled"] = c.chunk_filled; d["cell_filled"] = c.cell_filled; d["capacity_chunks"] = c.capacity_chunks;
            d["table_capacity"] = c.table_capacity; d["bytes_held"] = c.bytes_held; d["scratch_bytes"] = c.scratch_bytes; d["byte_limit"] = c.byte_limit;
            return d;
        })
        .def("ExportForDisplay", [](const DshGrid& g, const Rgba& collision_color, const Rgba& free_color, const Rgba& unknown_color) {
            visualization_msgs::MarkerArray a;
            a.markers = g.ExportForDisplay(ColorOf(collision_color), ColorOf(free_color), ColorOf(unknown_color));
            return MarkerArrayNumpy(a);
        }, py::arg("collision_color"), py::arg("free_color"), py::arg("unknown_color"),
             "0, 1 or 2 markers as [(ns, points float64 [n, 3], colors float32 [n, 4])]: chunk-filled chunks, then the cells of cell-filled chunks");
    m.def("ExtractSignedDistanceFieldBatch", [](const std::vector<const CollisionMapGrid*>& maps, float oob_value, bool unknown_is_filled,
                                                bool add_virtual_border) {
        return sdf_tools::ExtractSignedDistanceFieldBatch(maps, oob_value, unknown_is_filled, add_virtual_border);
    }, py::arg("maps"), py::arg("oob_value"), py::arg("unknown_is_filled"), py::arg("add_virtual_border"), py::call_guard<py::gil_scoped_release>(),
          "[(SignedDistanceField, (max, min))] of CollisionMapGrids of one shape in one batched build (sdfgpu_build_batch)");
}
