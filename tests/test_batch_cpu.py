"""The batch interface without a GPU: the symbols are exported by the built library and declared in the header, the Python helper
has the reference's parameter names, and ExtractSignedDistanceFieldBatch is declared where host-only code can include it."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sdfgpu_build_batch_device", "sdfgpu_get_extrema_batch", "sdfgpu_build_batch", "sdfgpu_build_tagged_objects",
           "sdfgpu_gradient_batch_device", "sdfgpu_last_batch_info")


def test_batch_symbols_are_exported_and_declared():
    from sdf_tools_amd import build
    lib = ctypes.CDLL(build.build_libsdfgpu())
    header = open(os.path.join(ROOT, "include", "sdfgpu.h")).read()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None, name
        assert re.search(r"\bint %s\(sdfgpu_handle h," % name, header), name


def test_capi_wraps_every_batch_entry_point():
    from sdf_tools_amd import capi
    for name in ("build_batch", "build_batch_device", "get_extrema_batch", "build_tagged_objects", "gradient_batch_device", "last_batch_info"):
        assert callable(getattr(capi.SdfGpu, name)), name
    L = capi.load_library()
    for name in SYMBOLS:
        assert getattr(L, name).argtypes, name


def test_utils_3d_batch_helper_has_the_reference_signature():
    from sdf_tools_amd import utils_3d
    assert list(inspect.signature(utils_3d.compute_sdf_and_gradient_batch).parameters) == ["env", "res", "origin_point", "batch_size"]


def test_batch_extraction_is_declared_for_host_only_code(tmp_path):
    src = tmp_path / "client.cpp"
    src.write_text(
        "#include <sdf_tools/collision_map.hpp>\n"
        "#include <sdf_tools/tagged_object_collision_map.hpp>\n"
        "std::vector<std::pair<sdf_tools::SignedDistanceField, std::pair<double, double>>> f(const std::vector<const sdf_tools::CollisionMapGrid*>& m) "
        "{ return sdf_tools::ExtractSignedDistanceFieldBatch(m, 0.0f, false, true); }\n"
        "std::map<uint32_t, sdf_tools::SignedDistanceField> g(const sdf_tools::TaggedObjectCollisionMapGrid& t) { return t.MakeObjectSDFs({1u, 2u}, false, true); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_pysdf_tools_binds_the_batch_calls():
    from sdf_tools_amd._bindings import load_pysdf_tools
    m = load_pysdf_tools()
    assert callable(m.ExtractSignedDistanceFieldBatch)
    assert hasattr(m.TaggedObjectCollisionMapGrid, "MakeObjectSDFs") and hasattr(m.TaggedObjectCollisionMapGrid, "MakeAllObjectSDFs")
