"""ctypes binding of the C ABI in include/sdfgpu.h (libsdfgpu.so).

This is the thin Python face of the drop-in boundary; it carries no compute.
If the HIP library is missing or no GPU is usable every entry point raises --
there is deliberately no CPU fallback (the CPU oracle lives in oracle/ and is
test infrastructure only).
"""
import ctypes
import math
import os

import numpy as np

from . import build as _build

SDFGPU_DSQ_INF = 1 << 30
_STATUS = {0: "OK", -1: "INVALID_ARGUMENT", -2: "HIP", -3: "UNSUPPORTED_SIZE", -4: "NO_DEVICE", -5: "UNRESOLVED", -6: "REDZONE"}

# every symbol include/sdfgpu.h declares (tests check that the library exports them all)
EXPORTS = [
    "sdfgpu_version", "sdfgpu_device_count", "sdfgpu_create", "sdfgpu_destroy", "sdfgpu_last_error",
    "sdfgpu_build", "sdfgpu_build_cells", "sdfgpu_build_device", "sdfgpu_build_cells_device",
    "sdfgpu_get_extrema", "sdfgpu_sweep_zy_device", "sdfgpu_sweep_x_device", "sdfgpu_extrema_from_dsq",
    "sdfgpu_gradient_device", "sdfgpu_debug_copy_zsweep", "sdfgpu_debug_copy_yzsweep", "sdfgpu_debug_flat_habit", "sdfgpu_set_tuning",
    "sdfgpu_set_profiling", "sdfgpu_get_stage_times", "sdfgpu_set_option", "sdfgpu_last_build_info", "sdfgpu_last_dense_certified",
    "sdfgpu_pack_bits_device", "sdfgpu_dense_ball_device", "sdfgpu_voxelize_points_device", "sdfgpu_build_tagged_cells", "sdfgpu_query_points_device", "sdfgpu_fold_extrema_device", "sdfgpu_slab_dense_phase",
    "sdfgpu_gradient", "sdfgpu_sweep_zy_tiered_device", "sdfgpu_sweep_x_lines_device", "sdfgpu_classify_cells_device",
    "sdfgpu_copy_to_host", "sdfgpu_copy_from_host", "sdfgpu_query_points", "sdfgpu_device_malloc", "sdfgpu_device_free",
    "sdfgpu_build_to_device", "sdfgpu_build_cells_to_device", "sdfgpu_upload_classified",
    "sdfgpu_build_bits_device", "sdfgpu_build_bits", "sdfgpu_voxelize_points_bits_device", "sdfgpu_debug_finish_table", "sdfgpu_redzone_check",
    "sdfgpu_components_bits_device", "sdfgpu_components", "sdfgpu_components_cells", "sdfgpu_component_stats_device",
    "sdfgpu_component_topology_device", "sdfgpu_component_topology", "sdfgpu_component_topology_cells",
    "sdfgpu_component_surfaces_device", "sdfgpu_component_surfaces", "sdfgpu_component_surfaces_cells",
    "sdfgpu_local_extrema_device", "sdfgpu_local_extrema", "sdfgpu_convex_segments_cells", "sdfgpu_convex_last_info",
    "sdfgpu_project_step_limit", "sdfgpu_project_points_device", "sdfgpu_project_points",
    "sdfgpu_query_gradients_device", "sdfgpu_query_gradients",
    "sdfgpu_build_batch_device", "sdfgpu_get_extrema_batch", "sdfgpu_build_batch", "sdfgpu_build_tagged_objects",
    "sdfgpu_gradient_batch_device", "sdfgpu_last_batch_info",
    "sdfgpu_resample_cells_device", "sdfgpu_resample_cells", "sdfgpu_debug_resample_times",
    "sdfgpu_display_select_cells_device", "sdfgpu_display_select_cells", "sdfgpu_display_select_sdf_device", "sdfgpu_display_select_sdf",
    "sdfgpu_display_expand_device", "sdfgpu_display_sdf_colors_device", "sdfgpu_display_sdf_colors",
    "sdfgpu_display_contour_reach", "sdfgpu_display_select_contour_device", "sdfgpu_display_select_contour",
    "sdfgpu_rasterize_shapes_device", "sdfgpu_rasterize_shapes",
    "sdfgpu_rasterize_meshes_device", "sdfgpu_rasterize_meshes",
    "sdfgpu_rasterize_solid_meshes_device", "sdfgpu_rasterize_solid_meshes", "sdfgpu_check_closed_meshes",
    "sdfgpu_dsh_create", "sdfgpu_dsh_destroy", "sdfgpu_dsh_info",
    "sdfgpu_dsh_set_cells_device", "sdfgpu_dsh_set_cells", "sdfgpu_dsh_set_chunks_device", "sdfgpu_dsh_set_chunks",
    "sdfgpu_dsh_insert_points_device", "sdfgpu_dsh_insert_rays_device", "sdfgpu_dsh_insert_rays", "sdfgpu_dsh_fuse_rays_device", "sdfgpu_dsh_fuse_rays",
    "sdfgpu_dsh_remove_chunks_device", "sdfgpu_dsh_remove_chunks", "sdfgpu_dsh_retain_box", "sdfgpu_dsh_shrink",
    "sdfgpu_dsh_cast_rays_device", "sdfgpu_dsh_cast_rays", "sdfgpu_dsh_cast_segments_device", "sdfgpu_dsh_cast_segments",
    "sdfgpu_dsh_get_device", "sdfgpu_dsh_get",
    "sdfgpu_dsh_extract_window_device", "sdfgpu_dsh_extract_window", "sdfgpu_dsh_export_device", "sdfgpu_dsh_export",
    "sdfgpu_dsh_frontier_window_device", "sdfgpu_dsh_frontier_window", "sdfgpu_dsh_frontier_cells_device", "sdfgpu_dsh_frontier_cells",
    "sdfgpu_dsh_update_components", "sdfgpu_dsh_components_info",
]

# include/sdfgpu.h "Projection": modes and per-point statuses
PROJECT_OUT_OF_COLLISION, PROJECT_INTO_VALID_VOLUME = 0, 1
PROJECT_CONVERGED, PROJECT_FLAT_GRADIENT, PROJECT_NO_GRADIENT, PROJECT_LEFT_GRID, PROJECT_STEP_LIMIT, PROJECT_NON_FINITE = range(6)
PROJECT_MAX_STEPS_CEILING = 1048576

# include/sdfgpu.h "Interpolated gradients": kinds and per-point statuses
QUERY_SMOOTH_GRADIENT, QUERY_AUTODIFF_GRADIENT, QUERY_DISTANCE_TO_BOUNDARY = 0, 1, 2
QUERY_OK, QUERY_OUTSIDE, QUERY_WINDOW_TOO_LARGE, QUERY_NON_FINITE = range(4)

# include/sdfgpu.h "Display export": rules and class bits
DISPLAY_OCCUPANCY, DISPLAY_KEY_FIELD = 0, 1
DISPLAY_FILLED, DISPLAY_EMPTY, DISPLAY_UNKNOWN = 1, 2, 4

# include/sdfgpu.h "Shape rasteriser": the types, the limit and struct sdfgpu_shape as a numpy record (160 bytes)
SHAPE_BOX, SHAPE_SPHERE, SHAPE_CYLINDER = 1, 2, 3
SHAPE_PLANE = 5
MAX_SHAPES = 65536
MAX_MESHES = 65536
MAX_TRIANGLES = 1 << 24
SHAPE_DTYPE = np.dtype([("type", np.uint32), ("object_id", np.uint32), ("dims", np.float64, (3,)), ("pose", np.float64, (16,))], align=True)
MESH_DTYPE = np.dtype([("object_id", np.uint32), ("reserved", np.uint32), ("first_triangle", np.int64), ("n_triangles", np.int64),
                       ("first_vertex", np.int64), ("n_vertices", np.int64), ("pose", np.float64, (16,))], align=True)


class SdfGpuError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("sdfgpu %s (%d): %s" % (_STATUS.get(code, "?"), code, message))
        self.code = code


_lib = None


def load_library():
    """dlopen sdf_tools_amd/libsdfgpu.so (must have been built: see build.py)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SDFGPU_LIB") or _build.LIB        # (SDFGPU_LIB: another build of the same library, for an A/B against this one)
    if not os.path.exists(path):
        raise ImportError("libsdfgpu.so is not built (run `python -m sdf_tools_amd.build`); "
                          "there is no CPU fallback for the SDF build path")
    # torch bundles its own libamdhip64.so (same SONAME as /opt/rocm's).  Import it first so the
    # dynamic loader binds libsdfgpu.so to the HIP runtime torch uses: streams and device pointers
    # are then shared by both.  Without torch the system ROCm runtime is used.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional plumbing
        pass
    L = ctypes.CDLL(path)
    i64, dbl, ci, vp, sz = ctypes.c_int64, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    u32 = ctypes.c_uint32
    L.sdfgpu_version.restype = ctypes.c_char_p
    L.sdfgpu_device_count.restype = ci
    L.sdfgpu_create.argtypes = [ci, ctypes.POINTER(vp)]
    L.sdfgpu_destroy.argtypes = [vp]
    L.sdfgpu_last_error.argtypes = [vp]
    L.sdfgpu_last_error.restype = ctypes.c_char_p
    L.sdfgpu_build.argtypes = [vp, vp, i64, i64, i64, dbl, ci, vp, vp, vp]
    L.sdfgpu_build_cells.argtypes = [vp, vp, sz, sz, ci, i64, i64, i64, dbl, ci, vp, vp, vp]
    L.sdfgpu_build_tagged_cells.argtypes = [vp, vp, sz, sz, sz, ci, vp, i64, ci, i64, i64, i64, dbl, ci, vp, vp, vp]
    L.sdfgpu_query_points_device.argtypes = [vp, vp, i64, i64, i64, dbl, vp, vp, ctypes.c_float, vp, i64, ci, vp, vp, vp, vp]
    L.sdfgpu_fold_extrema_device.argtypes = [vp, vp, vp]
    L.sdfgpu_query_points.argtypes = [vp, vp, i64, i64, i64, dbl, vp, vp, ctypes.c_float, vp, i64, ci, vp, vp, vp]
    L.sdfgpu_device_malloc.argtypes = [vp, sz, ctypes.POINTER(vp)]
    L.sdfgpu_device_free.argtypes = [vp, vp]
    L.sdfgpu_build_to_device.argtypes = [vp, vp, i64, i64, i64, dbl, ci, vp, vp, vp]
    L.sdfgpu_build_cells_to_device.argtypes = [vp, vp, sz, sz, ci, i64, i64, i64, dbl, ci, vp, vp, vp]
    L.sdfgpu_slab_dense_phase.argtypes = [vp, ci, vp, i64, i64, i64, vp, i64, i64, dbl, vp, vp, vp]
    L.sdfgpu_build_device.argtypes = [vp, vp, i64, i64, i64, dbl, ci, vp, vp]
    L.sdfgpu_build_cells_device.argtypes = [vp, vp, sz, sz, ci, i64, i64, i64, dbl, ci, vp, vp]
    L.sdfgpu_get_extrema.argtypes = [vp, vp, vp]
    L.sdfgpu_build_bits_device.argtypes = [vp, vp, i64, i64, i64, dbl, ci, vp, vp]
    L.sdfgpu_build_bits.argtypes = [vp, vp, i64, i64, i64, dbl, ci, vp, vp, vp]
    L.sdfgpu_voxelize_points_bits_device.argtypes = [vp, vp, i64, vp, dbl, i64, i64, i64, vp, ci, vp]
    L.sdfgpu_sweep_zy_device.argtypes = [vp, vp, i64, i64, i64, vp, vp]
    L.sdfgpu_classify_cells_device.argtypes = [vp, vp, sz, sz, ci, i64, vp, vp]
    L.sdfgpu_sweep_zy_tiered_device.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp]
    L.sdfgpu_sweep_x_lines_device.argtypes = [vp, vp, i64, i64, i64, i64, i64, dbl, ci, vp, vp, vp]
    L.sdfgpu_sweep_x_device.argtypes = [vp, vp, i64, i64, i64, i64, i64, ci, ci, i64, i64, dbl, ci, vp, vp, vp, vp]
    L.sdfgpu_pack_bits_device.argtypes = [vp, vp, i64, i64, vp, vp]
    L.sdfgpu_dense_ball_device.argtypes = [vp, vp, i64, i64, i64, i64, i64, dbl, vp, vp, vp, vp]
    L.sdfgpu_voxelize_points_device.argtypes = [vp, vp, i64, vp, dbl, i64, i64, i64, vp, ci, vp]
    L.sdfgpu_extrema_from_dsq.argtypes = [u32, u32, dbl, vp, vp]
    L.sdfgpu_gradient_device.argtypes = [vp, vp, i64, i64, i64, dbl, ci, vp, ci, vp]
    L.sdfgpu_gradient.argtypes = [vp, vp, i64, i64, i64, dbl, ci, vp, ci]
    L.sdfgpu_debug_finish_table.argtypes = [vp, vp, i64, dbl, ci, vp]
    L.sdfgpu_redzone_check.argtypes = [vp, vp]
    L.sdfgpu_debug_copy_zsweep.argtypes = [vp, vp, i64]
    L.sdfgpu_debug_copy_yzsweep.argtypes = [vp, vp, i64]
    L.sdfgpu_debug_flat_habit.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.sdfgpu_set_tuning.argtypes = [vp, ci, ci]
    L.sdfgpu_set_option.argtypes = [vp, ctypes.c_char_p, ci]
    L.sdfgpu_last_build_info.argtypes = [vp, vp]
    L.sdfgpu_last_dense_certified.argtypes = [vp, vp]
    L.sdfgpu_set_profiling.argtypes = [vp, ci]
    L.sdfgpu_copy_to_host.argtypes = [vp, vp, vp, ctypes.c_size_t, vp]
    L.sdfgpu_copy_from_host.argtypes = [vp, vp, vp, ctypes.c_size_t, vp]
    L.sdfgpu_upload_classified.argtypes = [vp, vp, vp, sz, sz, ci, i64, vp, vp]
    L.sdfgpu_get_stage_times.argtypes = [vp, vp, vp]
    L.sdfgpu_components_bits_device.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp]
    L.sdfgpu_components.argtypes = [vp, vp, i64, i64, i64, vp, vp]
    L.sdfgpu_components_cells.argtypes = [vp, vp, sz, sz, sz, i64, i64, i64, vp]
    L.sdfgpu_component_stats_device.argtypes = [vp, vp, vp, i64, i64, i64, u32, vp, i64, vp, vp]
    L.sdfgpu_component_topology_device.argtypes = [vp, vp, vp, i64, i64, i64, u32, vp, vp]
    L.sdfgpu_component_topology.argtypes = [vp, vp, vp, i64, i64, i64, u32, vp]
    L.sdfgpu_component_topology_cells.argtypes = [vp, vp, sz, sz, sz, i64, i64, i64, ci, u32, vp]
    L.sdfgpu_component_surfaces_device.argtypes = [vp, vp, vp, i64, i64, i64, u32, vp, vp, i64, vp, vp, vp]
    L.sdfgpu_component_surfaces.argtypes = [vp, vp, vp, i64, i64, i64, u32, vp, vp, i64, vp]
    L.sdfgpu_component_surfaces_cells.argtypes = [vp, vp, sz, sz, sz, i64, i64, i64, ci, u32, vp, vp, i64, vp]
    L.sdfgpu_local_extrema_device.argtypes = [vp, vp, i64, i64, i64, dbl, vp, vp, vp]
    L.sdfgpu_local_extrema.argtypes = [vp, vp, i64, i64, i64, dbl, vp, vp]
    L.sdfgpu_convex_segments_cells.argtypes = [vp, vp, sz, sz, sz, sz, i64, i64, i64, dbl, vp, dbl, ci, vp]
    L.sdfgpu_convex_last_info.argtypes = [vp, vp, vp, vp, vp]
    L.sdfgpu_project_step_limit.argtypes = [i64, i64, i64, dbl, ci, vp]
    L.sdfgpu_project_points_device.argtypes = [vp, vp, i64, i64, i64, dbl, vp, vp, dbl, dbl, ci, ci, vp, i64, vp, vp, vp, vp]
    L.sdfgpu_project_points.argtypes = [vp, vp, i64, i64, i64, dbl, vp, vp, dbl, dbl, ci, ci, vp, i64, vp, vp, vp]
    L.sdfgpu_query_gradients_device.argtypes = [vp, vp, i64, i64, i64, dbl, vp, ctypes.c_float, ci, dbl, vp, i64, vp, vp, vp, vp]
    L.sdfgpu_query_gradients.argtypes = [vp, vp, i64, i64, i64, dbl, vp, ctypes.c_float, ci, dbl, vp, i64, vp, vp, vp]
    L.sdfgpu_resample_cells_device.argtypes = [vp, vp, sz, i64, i64, i64, vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, vp]
    L.sdfgpu_resample_cells.argtypes = [vp, vp, sz, i64, i64, i64, vp, vp, vp, vp, vp, i64, i64, i64, vp, vp]
    L.sdfgpu_debug_resample_times.argtypes = [vp, vp, vp]
    L.sdfgpu_display_select_cells_device.argtypes = [vp, vp, sz, sz, sz, i64, i64, i64, ci, ci, ci, vp, i64, ci, ci, vp, vp, i64, vp, vp, vp, i64, vp, vp]
    L.sdfgpu_display_select_cells.argtypes = [vp, vp, sz, sz, sz, i64, i64, i64, ci, ci, ci, vp, i64, ci, ci, vp, vp, i64, vp, vp, vp, i64, vp]
    L.sdfgpu_display_select_sdf_device.argtypes = [vp, vp, i64, i64, i64, vp, i64, vp, vp]
    L.sdfgpu_display_select_sdf.argtypes = [vp, vp, i64, i64, i64, vp, i64, vp]
    L.sdfgpu_display_expand_device.argtypes = [vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, vp, i64, vp, vp]
    L.sdfgpu_display_sdf_colors_device.argtypes = [vp, vp, i64, i64, i64, ctypes.c_float, vp, vp]
    L.sdfgpu_display_sdf_colors.argtypes = [vp, vp, i64, i64, i64, ctypes.c_float, vp]
    L.sdfgpu_display_contour_reach.argtypes = [dbl, vp]
    L.sdfgpu_display_select_contour_device.argtypes = [vp, vp, sz, sz, sz, i64, i64, i64, ci, ci, vp, i64, ci, ci, vp, vp, i64, vp, vp, vp, i64, vp, vp]
    L.sdfgpu_display_select_contour.argtypes = [vp, vp, sz, sz, sz, i64, i64, i64, ci, ci, vp, i64, ci, ci, vp, vp, i64, vp, vp, vp, i64, vp]
    L.sdfgpu_rasterize_shapes_device.argtypes = [vp, vp, i64, vp, dbl, i64, i64, i64, vp, vp, vp, vp, vp]
    L.sdfgpu_rasterize_shapes.argtypes = [vp, vp, i64, vp, dbl, i64, i64, i64, vp, vp, vp]
    L.sdfgpu_rasterize_meshes_device.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, dbl, i64, i64, i64, vp, vp, vp, ctypes.c_int, vp, vp]
    L.sdfgpu_rasterize_meshes.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, dbl, i64, i64, i64, vp, vp, vp]
    L.sdfgpu_rasterize_solid_meshes_device.argtypes = L.sdfgpu_rasterize_meshes_device.argtypes
    L.sdfgpu_rasterize_solid_meshes.argtypes = L.sdfgpu_rasterize_meshes.argtypes
    L.sdfgpu_check_closed_meshes.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp]
    L.sdfgpu_build_batch_device.argtypes = [vp, vp, i64, i64, i64, i64, dbl, vp, ci, vp, vp]
    L.sdfgpu_get_extrema_batch.argtypes = [vp, i64, vp, vp]
    L.sdfgpu_build_batch.argtypes = [vp, vp, i64, i64, i64, i64, dbl, vp, ci, vp, vp, vp]
    L.sdfgpu_build_tagged_objects.argtypes = [vp, vp, sz, sz, sz, vp, i64, ci, i64, i64, i64, dbl, ci, vp, vp, vp]
    L.sdfgpu_gradient_batch_device.argtypes = [vp, vp, i64, i64, i64, i64, dbl, vp, ci, ci, vp, vp]
    L.sdfgpu_last_batch_info.argtypes = [vp, vp, vp]
    L.sdfgpu_dsh_create.argtypes = [vp, vp, dbl, i64, i64, i64, vp, i64, ctypes.c_uint64, ctypes.POINTER(vp)]
    L.sdfgpu_dsh_destroy.argtypes = [vp]
    L.sdfgpu_dsh_info.argtypes = [vp, vp]
    L.sdfgpu_dsh_set_cells_device.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    L.sdfgpu_dsh_set_cells.argtypes = [vp, vp, i64, vp, vp, vp]
    L.sdfgpu_dsh_set_chunks_device.argtypes = L.sdfgpu_dsh_set_cells_device.argtypes
    L.sdfgpu_dsh_set_chunks.argtypes = L.sdfgpu_dsh_set_cells.argtypes
    L.sdfgpu_dsh_insert_points_device.argtypes = [vp, vp, i64, vp, vp, vp]
    L.sdfgpu_dsh_insert_rays_device.argtypes = [vp, vp, vp, i64, dbl, vp, vp, vp, vp, vp]
    L.sdfgpu_dsh_insert_rays.argtypes = [vp, vp, vp, i64, dbl, vp, vp, vp, vp]
    L.sdfgpu_dsh_fuse_rays_device.argtypes = [vp, vp, vp, i64, dbl, vp, vp, vp, vp]
    L.sdfgpu_dsh_fuse_rays.argtypes = [vp, vp, vp, i64, dbl, vp, vp, vp]
    L.sdfgpu_dsh_remove_chunks_device.argtypes = [vp, vp, i64, vp, vp, vp]
    L.sdfgpu_dsh_remove_chunks.argtypes = [vp, vp, i64, vp, vp]
    L.sdfgpu_dsh_retain_box.argtypes = [vp, vp, vp, ci, vp, vp]
    L.sdfgpu_dsh_shrink.argtypes = [vp, i64, vp]
    L.sdfgpu_dsh_cast_rays_device.argtypes = [vp, vp, vp, i64, dbl, ctypes.c_uint32, vp, vp, vp]
    L.sdfgpu_dsh_cast_rays.argtypes = [vp, vp, vp, i64, dbl, ctypes.c_uint32, vp, vp]
    L.sdfgpu_dsh_cast_segments_device.argtypes = [vp, vp, vp, i64, dbl, ctypes.c_uint32, vp, vp, vp]
    L.sdfgpu_dsh_cast_segments.argtypes = [vp, vp, vp, i64, dbl, ctypes.c_uint32, vp, vp]
    L.sdfgpu_dsh_get_device.argtypes = [vp, vp, i64, vp, vp, vp]
    L.sdfgpu_dsh_get.argtypes = [vp, vp, i64, vp, vp]
    L.sdfgpu_dsh_extract_window_device.argtypes = [vp, vp, i64, i64, i64, ci, vp, vp, vp]
    L.sdfgpu_dsh_extract_window.argtypes = [vp, vp, i64, i64, i64, ci, vp, vp]
    L.sdfgpu_dsh_export_device.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp]
    L.sdfgpu_dsh_export.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    L.sdfgpu_dsh_frontier_window_device.argtypes = [vp, vp, i64, i64, i64, u32, vp, vp]
    L.sdfgpu_dsh_frontier_window.argtypes = [vp, vp, i64, i64, i64, u32, vp]
    L.sdfgpu_dsh_frontier_cells_device.argtypes = [vp, vp, vp, u32, vp, i64, vp, vp]
    L.sdfgpu_dsh_frontier_cells.argtypes = [vp, vp, vp, u32, vp, i64, vp]
    L.sdfgpu_dsh_update_components.argtypes = [vp, u32, vp, vp]
    L.sdfgpu_dsh_components_info.argtypes = [vp, vp, vp, vp]
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is ctypes.c_int or name not in ("sdfgpu_version", "sdfgpu_last_error"):
            fn.restype = ci
    _lib = L
    return L


def pack_bits_host(filled):
    """uint8 / bool occupancy (any shape) -> the linear bit field of sdfgpu_build_bits*: uint32[ceil(n / 32)], bit (v & 31) of
    word (v >> 5) = voxel v in C order."""
    m = np.ascontiguousarray(filled).reshape(-1) != 0
    b = np.packbits(m, bitorder="little")
    b = np.concatenate([b, np.zeros((-b.size) % 4, np.uint8)])
    return b.view("<u4").astype(np.uint32, copy=False)


TOPOLOGY_FILLED, TOPOLOGY_EMPTY, TOPOLOGY_UNKNOWN = 1, 2, 4       # class_mask of SdfGpu.component_topology_cells


def topology_holes_voids(counts):
    """component_topology* counters int64 [L, 5] (surface vertices, M3, M5, M6, surfaces) -> {component: (holes, voids)} for every
    component with a surface vertex, in the reference's int32 arithmetic: raw = 1 + (M5 + 2 M6 - M3) / 8 with C truncation
    (math.trunc, not //), voids = surfaces - 1, holes = raw + voids."""
    out = {}
    counts = np.asarray(counts)
    for c in np.nonzero(counts[:, 0])[0]:
        _, m3, m5, m6, surfaces = (int(v) for v in counts[c])
        num = m5 + 2 * m6 - m3
        raw = 1 + (abs(num) // 8) * (1 if num >= 0 else -1)
        out[int(c)] = (raw + surfaces - 1, surfaces - 1)
    return out


EXTREMUM_OFF = 0xFFFFFFFF          # local_extrema*: the voxel's gradient walk leaves the grid


def quaternion_and_inverse(q=(1.0, 0.0, 0.0, 0.0)):
    """(w, x, y, z) -> the 8 doubles of sdfgpu_local_extrema*'s q_and_qinv: q, then q.inverse() with eigen_lite's arithmetic
    (n = w w + x x + y y + z z, left to right; (w / n, -x / n, -y / n, -z / n))."""
    w, x, y, z = (float(v) for v in q)
    n = w * w + x * x + y * y + z * z
    return (w, x, y, z, w / n, -x / n, -y / n, -z / n)


def quaternion_from_matrix(R):
    """3x3 rotation -> (w, x, y, z) by eigen_lite's Quaterniond(Matrix3d) (Shepperd's method, same branches and operations): the
    quaternion the C++ classes derive from their origin transform."""
    R = [[float(R[i][j]) for j in range(3)] for i in range(3)]
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        return (0.25 * s, (R[2][1] - R[1][2]) / s, (R[0][2] - R[2][0]) / s, (R[1][0] - R[0][1]) / s)
    if R[0][0] > R[1][1] and R[0][0] > R[2][2]:
        s = math.sqrt(1.0 + R[0][0] - R[1][1] - R[2][2]) * 2
        return ((R[2][1] - R[1][2]) / s, 0.25 * s, (R[0][1] + R[1][0]) / s, (R[0][2] + R[2][0]) / s)
    if R[1][1] > R[2][2]:
        s = math.sqrt(1.0 + R[1][1] - R[0][0] - R[2][2]) * 2
        return ((R[0][2] - R[2][0]) / s, (R[0][1] + R[1][0]) / s, 0.25 * s, (R[1][2] + R[2][1]) / s)
    s = math.sqrt(1.0 + R[2][2] - R[0][0] - R[1][1]) * 2
    return ((R[1][0] - R[0][1]) / s, (R[0][2] + R[2][0]) / s, (R[1][2] + R[2][1]) / s, 0.25 * s)


def extremum_locations(indices, shape, resolution):
    """uint32 extremum indices [nx, ny, nz] -> the reference's local extrema map, float64 [nx, ny, nz, 3]: grid-frame cell centres
    res * (i + 0.5), (+inf, +inf, +inf) for EXTREMUM_OFF."""
    nx, ny, nz = (int(s) for s in shape)
    idx = np.asarray(indices, np.uint32).reshape(-1).astype(np.int64)
    off = idx == EXTREMUM_OFF
    idx = np.where(off, 0, idx)
    res = float(resolution)
    out = np.empty((idx.size, 3), np.float64)
    out[:, 0] = res * ((idx // (ny * nz)).astype(np.float64) + 0.5)
    out[:, 1] = res * (((idx // nz) % ny).astype(np.float64) + 0.5)
    out[:, 2] = res * ((idx % nz).astype(np.float64) + 0.5)
    out[off] = np.inf
    return out.reshape(nx, ny, nz, 3)


def _transform12(t):
    """3x4 or 4x4 transform -> the 12 row-major doubles of the C ABI (None stays None)"""
    if t is None:
        return None
    a = np.asarray(t, np.float64)
    return (ctypes.c_double * 12)(*a.reshape(-1, 4)[:3].reshape(-1))


def _doubles(v, n):
    """scalar or sequence -> n C doubles (a scalar is repeated; a matrix is taken row-major)"""
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, n)
    if a.size != n:
        raise ValueError("expected %d values, got %d" % (n, a.size))
    return (ctypes.c_double * n)(*a)


def make_shapes(items):
    """[(type, object_id, dims, pose 4 x 4 or 3 x 4)] -> SHAPE_DTYPE records (missing dims are 0, the pose's fourth row 0 0 0 1)"""
    out = np.zeros(len(items), SHAPE_DTYPE)
    for rec, (kind, object_id, dims, pose) in zip(out, items):
        rec["type"], rec["object_id"] = kind, object_id
        d = np.asarray(dims, np.float64).reshape(-1)
        rec["dims"][:d.size] = d
        m = np.eye(4)
        m[:3] = np.asarray(pose, np.float64).reshape(-1, 4)[:3]
        rec["pose"] = m.reshape(-1)
    return out


MAX_SOLID_MESHES = 256                # SDFGPU_MAX_SOLID_MESHES


def make_meshes(items):
    """[(object_id, vertices [n, 3], triangles [m, 3] of indices into those vertices, pose 4 x 4 or 3 x 4)] ->
    (MESH_DTYPE records, vertices float64 [sum n, 3], triangles uint32 [sum m, 3]): the arrays of sdfgpu_rasterize_meshes, every
    mesh's runs one behind the other"""
    out = np.zeros(len(items), MESH_DTYPE)
    vs, ts = [np.zeros((0, 3), np.float64)], [np.zeros((0, 3), np.uint32)]
    nv = nt = 0
    for rec, (object_id, vertices, triangles, pose) in zip(out, items):
        v = np.asarray(vertices, np.float64).reshape(-1, 3)
        t = np.asarray(triangles, np.uint32).reshape(-1, 3)
        rec["object_id"] = object_id
        rec["first_triangle"], rec["n_triangles"], rec["first_vertex"], rec["n_vertices"] = nt, len(t), nv, len(v)
        m = np.eye(4)
        m[:3] = np.asarray(pose, np.float64).reshape(-1, 4)[:3]
        rec["pose"] = m.reshape(-1)
        vs.append(v)
        ts.append(t)
        nv, nt = nv + len(v), nt + len(t)
    return out, np.ascontiguousarray(np.concatenate(vs)), np.ascontiguousarray(np.concatenate(ts))


def check_closed_meshes(meshes, vertices, triangles):
    """sdfgpu_check_closed_meshes (no GPU needed): None when every mesh is closed -- each undirected edge, its endpoints keyed by
    world position, is used by an even number of the mesh's triangles -- else (mesh index, triangle index within the mesh); the
    triangle is -1 for a refused mesh record.  Refused arrays raise."""
    L = load_library()
    ms = np.ascontiguousarray(meshes, dtype=MESH_DTYPE).reshape(-1)
    vs = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    ts = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
    bad_mesh, bad_triangle = ctypes.c_int64(-2), ctypes.c_int64(-2)
    rc = L.sdfgpu_check_closed_meshes(ms.ctypes.data if ms.size else None, int(ms.size), vs.ctypes.data if vs.size else None, len(vs),
                                      ts.ctypes.data if ts.size else None, len(ts), ctypes.byref(bad_mesh), ctypes.byref(bad_triangle))
    if rc == 0:
        return None
    if bad_mesh.value < 0:
        raise ValueError("sdfgpu_check_closed_meshes: refused arguments")
    return int(bad_mesh.value), int(bad_triangle.value)


def project_step_limit(shape, stepsize_multiplier=1.0 / 8.0, max_steps=0):
    """The step limit a projection with these arguments uses (sdfgpu_project_step_limit; no GPU needed)."""
    L = load_library()
    out = ctypes.c_int()
    nx, ny, nz = (int(v) for v in shape)
    rc = L.sdfgpu_project_step_limit(nx, ny, nz, float(stepsize_multiplier), int(max_steps), ctypes.byref(out))
    if rc != 0:
        raise SdfGpuError(rc, "stepsize_multiplier must be positive and finite, max_steps >= 0, dims positive")
    return out.value


def display_contour_reach(cell_size):
    """include/sdfgpu.h "Display export: contours": the largest squared distance D in 0 .. 3 that ExportContourOnlyForDisplay draws
    at this cell size (the reference's literal float comparisons; NaN and sizes <= 0 give 0).  Host only."""
    reach = ctypes.c_int(-1)
    rc = load_library().sdfgpu_display_contour_reach(float(cell_size), ctypes.byref(reach))
    if rc != 0:
        raise SdfGpuError(rc, "sdfgpu_display_contour_reach")
    return int(reach.value)


def device_count():
    return int(load_library().sdfgpu_device_count())


def extrema_from_dsq(max_dsq_free, max_dsq_filled, resolution):
    """Host helper (no GPU needed): (max, min) from the integer maxima, as sdf_generation.hpp:246-269."""
    out = (ctypes.c_double * 2)()
    rc = load_library().sdfgpu_extrema_from_dsq(int(max_dsq_free), int(max_dsq_filled), float(resolution),
                                                ctypes.byref(out, 0), ctypes.byref(out, 8))
    if rc != 0:
        raise SdfGpuError(rc, "resolution must be positive and finite")
    return float(out[0]), float(out[1])


class SdfGpu:
    """One context on one GPU (wraps sdfgpu_create / sdfgpu_destroy)."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = ctypes.c_void_p()
        rc = self._lib.sdfgpu_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise SdfGpuError(rc, self._lib.sdfgpu_last_error(None).decode())
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sdfgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise SdfGpuError(rc, self._lib.sdfgpu_last_error(self._h).decode())

    # ---- host-buffer API -------------------------------------------------
    def build(self, filled, resolution=1.0, add_virtual_border=False):
        """filled: uint8/bool [nx,ny,nz].  Returns (sdf float32 [nx,ny,nz], (max, min))."""
        m = np.ascontiguousarray(filled, dtype=np.uint8)
        if m.ndim != 3:
            raise ValueError("mask must be [nx, ny, nz]")
        out = np.empty(m.shape, dtype=np.float32)
        ext = (ctypes.c_double * 2)()
        self._check(self._lib.sdfgpu_build(self._h, m.ctypes.data, *m.shape, float(resolution),
                                           int(bool(add_virtual_border)), out.ctypes.data,
                                           ctypes.byref(ext, 0), ctypes.byref(ext, 8)))
        return out, (float(ext[0]), float(ext[1]))

    def build_cells(self, cells, shape, cell_stride=8, occupancy_offset=0, unknown_is_filled=False,
                    resolution=1.0, add_virtual_border=False):
        """cells: raw COLLISION_CELL records (any contiguous array of nx*ny*nz*cell_stride bytes)."""
        c = np.ascontiguousarray(cells)
        nx, ny, nz = (int(s) for s in shape)
        if c.nbytes != nx * ny * nz * cell_stride:
            raise ValueError("cells buffer size does not match shape * cell_stride")
        out = np.empty((nx, ny, nz), dtype=np.float32)
        ext = (ctypes.c_double * 2)()
        self._check(self._lib.sdfgpu_build_cells(self._h, c.ctypes.data, cell_stride, occupancy_offset,
                                                 int(bool(unknown_is_filled)), nx, ny, nz, float(resolution),
                                                 int(bool(add_virtual_border)), out.ctypes.data,
                                                 ctypes.byref(ext, 0), ctypes.byref(ext, 8)))
        return out, (float(ext[0]), float(ext[1]))

    def build_tagged_cells(self, cells, shape, object_mode=0, object_ids=(), unknown_is_filled=False, resolution=1.0,
                           add_virtual_border=False, cell_stride=16, occupancy_offset=0, object_id_offset=8):
        """cells: raw TAGGED_OBJECT_COLLISION_CELL records; object_mode 0 any / 1 named (id > 0) / 2 id list.
        cells=None re-uses the records the previous call on this context uploaded (one field per object: upload once)."""
        nx, ny, nz = (int(s) for s in shape)
        c = None
        if cells is not None:
            c = np.ascontiguousarray(cells)
            if c.nbytes != nx * ny * nz * cell_stride:
                raise ValueError("cells buffer size does not match shape * cell_stride")
        ids = np.ascontiguousarray(np.asarray(object_ids, dtype=np.uint32))
        out = np.empty((nx, ny, nz), dtype=np.float32)
        ext = (ctypes.c_double * 2)()
        self._check(self._lib.sdfgpu_build_tagged_cells(
            self._h, c.ctypes.data if c is not None else None, cell_stride, occupancy_offset, object_id_offset, int(object_mode),
            ids.ctypes.data if ids.size else None, int(ids.size), int(bool(unknown_is_filled)), nx, ny, nz,
            float(resolution), int(bool(add_virtual_border)), out.ctypes.data, ctypes.byref(ext, 0), ctypes.byref(ext, 8)))
        return out, (float(ext[0]), float(ext[1]))

    def query_points_device(self, d_sdf, shape, resolution, d_points, n_points, d_distance=0, d_gradient=0, d_flags=0,
                            world_to_grid=None, rotation=None, oob_value=float("inf"), enable_edge_gradients=False,
                            stream=0):
        """Batched EstimateDistance / GetGradient at n world-frame points (device pointers as ints)."""
        nx, ny, nz = (int(s) for s in shape)
        w = None if world_to_grid is None else (ctypes.c_double * 12)(*np.asarray(world_to_grid, np.float64).reshape(-1)[:12])
        r = None if rotation is None else (ctypes.c_double * 9)(*np.asarray(rotation, np.float64).reshape(-1)[:9])
        self._check(self._lib.sdfgpu_query_points_device(
            self._h, d_sdf, nx, ny, nz, float(resolution), w, r, float(oob_value), d_points, int(n_points),
            int(bool(enable_edge_gradients)), d_distance or None, d_gradient or None, d_flags or None, stream or None))

    # ---- host input -> device-resident field; host points -> host answers (what the C++ mirror's DeviceSignedDistanceField uses)
    def device_malloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(self._lib.sdfgpu_device_malloc(self._h, int(nbytes), ctypes.byref(p)))
        return int(p.value)

    def device_free(self, ptr):
        self._check(self._lib.sdfgpu_device_free(self._h, ctypes.c_void_p(int(ptr))))

    def build_to_device(self, filled, d_out, resolution=1.0, add_virtual_border=False):
        """Host mask [nx, ny, nz] -> fp32 field at device address d_out (no download).  Returns (max, min)."""
        m = np.ascontiguousarray(filled, dtype=np.uint8)
        ext = (ctypes.c_double * 2)()
        self._check(self._lib.sdfgpu_build_to_device(self._h, m.ctypes.data, *m.shape, float(resolution),
                                                     int(bool(add_virtual_border)), ctypes.c_void_p(int(d_out)),
                                                     ctypes.byref(ext, 0), ctypes.byref(ext, 8)))
        return float(ext[0]), float(ext[1])

    def query_points(self, d_sdf, shape, resolution, points, world_to_grid=None, rotation=None, oob_value=float("inf"),
                     enable_edge_gradients=False):
        """Batched EstimateDistance + GetGradient at host points [n, 3] float64 against a field in HBM.
        Returns (distance [n], gradient [n, 3], flags [n]) as numpy arrays."""
        nx, ny, nz = (int(v) for v in shape)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        dist, grad, flags = np.empty(n, np.float64), np.empty((n, 3), np.float64), np.empty(n, np.uint8)
        w = None if world_to_grid is None else (ctypes.c_double * 12)(*np.asarray(world_to_grid, np.float64).reshape(-1)[:12])
        r = None if rotation is None else (ctypes.c_double * 9)(*np.asarray(rotation, np.float64).reshape(-1)[:9])
        self._check(self._lib.sdfgpu_query_points(self._h, ctypes.c_void_p(int(d_sdf)), nx, ny, nz, float(resolution), w, r,
                                                  float(oob_value), pts.ctypes.data, n, int(bool(enable_edge_gradients)),
                                                  dist.ctypes.data, grad.ctypes.data, flags.ctypes.data))
        return dist, grad, flags

    def slab_dense_phase(self, phase, d_mask_slab, nxs, ny, nz, d_bits_ext, halo_lo, halo_hi, resolution, d_out, d_small,
                         stream=0):
        self._check(self._lib.sdfgpu_slab_dense_phase(self._h, int(phase), d_mask_slab, int(nxs), int(ny), int(nz), d_bits_ext,
                                                      int(halo_lo), int(halo_hi), float(resolution), d_out, d_small,
                                                      stream or None))

    def fold_extrema_device(self, d_maxdsq, stream=0):
        self._check(self._lib.sdfgpu_fold_extrema_device(self._h, d_maxdsq, stream or None))

    # ---- device-pointer API (raw integers: tensor.data_ptr(), stream.cuda_stream) -------------
    def build_device(self, d_filled, shape, d_out, resolution=1.0, add_virtual_border=False, stream=0):
        nx, ny, nz = (int(s) for s in shape)
        self._check(self._lib.sdfgpu_build_device(self._h, d_filled, nx, ny, nz, float(resolution),
                                                  int(bool(add_virtual_border)), d_out, stream or None))

    def build_bits_device(self, d_bits, shape, d_out, resolution=1.0, add_virtual_border=False, stream=0):
        """d_bits: device pointer of the linear bit field (bit v & 31 of word v >> 5 = voxel v), ceil(n / 32) uint32 words."""
        nx, ny, nz = (int(s) for s in shape)
        self._check(self._lib.sdfgpu_build_bits_device(self._h, d_bits, nx, ny, nz, float(resolution),
                                                       int(bool(add_virtual_border)), d_out, stream or None))

    def build_bits(self, bits, shape, resolution=1.0, add_virtual_border=False):
        """bits: host uint32 array of ceil(n / 32) words (see pack_bits_host).  Returns (sdf float32 [nx,ny,nz], (max, min))."""
        nx, ny, nz = (int(s) for s in shape)
        b = np.ascontiguousarray(bits, dtype=np.uint32)
        if b.size != (nx * ny * nz + 31) // 32:
            raise ValueError("bit field must hold ceil(nx*ny*nz / 32) words")
        out = np.empty((nx, ny, nz), dtype=np.float32)
        ext = (ctypes.c_double * 2)()
        self._check(self._lib.sdfgpu_build_bits(self._h, b.ctypes.data, nx, ny, nz, float(resolution),
                                                int(bool(add_virtual_border)), out.ctypes.data,
                                                ctypes.byref(ext, 0), ctypes.byref(ext, 8)))
        return out, (float(ext[0]), float(ext[1]))

    # ---- connected components (CollisionMapGrid::UpdateConnectedComponents, include/sdfgpu.h) -------------
    def components(self, filled):
        """filled: uint8/bool [nx,ny,nz].  Returns (labels uint32 [nx,ny,nz], K): 6-connected components of the filled and the
        free voxels, numbered 1..K in x -> y -> z scan order."""
        m = np.ascontiguousarray(filled, dtype=np.uint8)
        if m.ndim != 3:
            raise ValueError("mask must be [nx, ny, nz]")
        out = np.empty(m.shape, dtype=np.uint32)
        k = ctypes.c_uint32(0)
        self._check(self._lib.sdfgpu_components(self._h, m.ctypes.data, *m.shape, out.ctypes.data, ctypes.byref(k)))
        return out, int(k.value)

    def components_bits_device(self, d_bits, shape, d_labels, stream=0):
        """d_bits: device bit field (ceil(n / 32) words), d_labels: device uint32 [n].  Returns K (synchronises `stream`)."""
        nx, ny, nz = (int(s) for s in shape)
        k = ctypes.c_uint32(0)
        self._check(self._lib.sdfgpu_components_bits_device(self._h, d_bits, nx, ny, nz, d_labels, ctypes.byref(k), stream or None))
        return int(k.value)

    def component_stats_device(self, d_bits, d_labels, shape, label_count, d_stats=0, capacity=0, stream=0):
        """sdfgpu_component_stats_device: bit field + the labels made from it (device) -> COMPONENT_STATS_DTYPE records of the labels
        in 1 .. label_count with a set voxel, in label order, at d_stats iff `capacity` (in records) suffices; returns their number"""
        total = ctypes.c_int64()
        self._check(self._lib.sdfgpu_component_stats_device(self._h, d_bits or None, d_labels or None, *(int(s) for s in shape), int(label_count),
                                                            d_stats or None, int(capacity), ctypes.byref(total), stream or None))
        return total.value

    def components_cells(self, cells, shape, cell_stride=8, occupancy_offset=0, component_offset=4):
        """cells: writable contiguous records (COLLISION_CELL: 8, 0, 4; TAGGED_OBJECT_COLLISION_CELL: 16, 0, 4); the labels are
        written into them in place.  Returns K."""
        nx, ny, nz = (int(s) for s in shape)
        if not (isinstance(cells, np.ndarray) and cells.flags.c_contiguous and cells.flags.writeable):
            raise ValueError("cells must be a writable C-contiguous numpy array")
        if cells.nbytes != nx * ny * nz * cell_stride:
            raise ValueError("cells buffer size does not match shape * cell_stride")
        k = ctypes.c_uint32(0)
        self._check(self._lib.sdfgpu_components_cells(self._h, cells.ctypes.data, cell_stride, occupancy_offset, component_offset,
                                                      nx, ny, nz, ctypes.byref(k)))
        return int(k.value)

    # ---- component topology (CollisionMapGrid::ComputeComponentTopology, include/sdfgpu.h) -----------------
    def component_topology(self, labels, select=None, max_label=None):
        """labels: uint32 [nx, ny, nz]; select: bool/uint8 [nx, ny, nz] or None (every voxel).  Returns int64 [max_label + 1, 5]:
        surface vertices, M3, M5, M6, surfaces per label (topology_holes_voids turns it into {c: (holes, voids)}).  max_label
        defaults to the largest label."""
        lab = np.ascontiguousarray(labels, dtype=np.uint32)
        if lab.ndim != 3:
            raise ValueError("labels must be [nx, ny, nz]")
        if max_label is None:
            max_label = int(lab.max()) if lab.size else 0
        sel = None
        if select is not None:
            sel = np.ascontiguousarray(np.asarray(select) != 0, dtype=np.uint8)
            if sel.shape != lab.shape:
                raise ValueError("select must have the labels' shape")
        out = np.zeros((int(max_label) + 1, 5), np.int64)
        self._check(self._lib.sdfgpu_component_topology(self._h, lab.ctypes.data, None if sel is None else sel.ctypes.data, *lab.shape,
                                                         int(max_label), out.ctypes.data))
        return out

    def component_topology_device(self, d_labels, shape, max_label, d_select_bits=None, stream=0):
        """d_labels: device uint32 [n]; d_select_bits: device bit field (ceil(n / 32) words) or None.  Returns int64
        [max_label + 1, 5] (synchronises `stream`)."""
        nx, ny, nz = (int(s) for s in shape)
        out = np.zeros((int(max_label) + 1, 5), np.int64)
        self._check(self._lib.sdfgpu_component_topology_device(self._h, d_labels, d_select_bits or None, nx, ny, nz, int(max_label),
                                                                out.ctypes.data, stream or None))
        return out

    def component_topology_cells(self, cells, shape, class_mask, max_label, cell_stride=8, occupancy_offset=0, component_offset=4):
        """cells: contiguous records (COLLISION_CELL: 8, 0, 4; TAGGED_OBJECT_COLLISION_CELL: 16, 0, 4) holding labels;
        class_mask: TOPOLOGY_FILLED | TOPOLOGY_EMPTY | TOPOLOGY_UNKNOWN (7 = every voxel).  Returns int64 [max_label + 1, 5]."""
        nx, ny, nz = (int(s) for s in shape)
        if not (isinstance(cells, np.ndarray) and cells.flags.c_contiguous):
            raise ValueError("cells must be a C-contiguous numpy array")
        if cells.nbytes != nx * ny * nz * cell_stride:
            raise ValueError("cells buffer size does not match shape * cell_stride")
        out = np.zeros((int(max_label) + 1, 5), np.int64)
        self._check(self._lib.sdfgpu_component_topology_cells(self._h, cells.ctypes.data, cell_stride, occupancy_offset, component_offset,
                                                               nx, ny, nz, int(class_mask), int(max_label), out.ctypes.data))
        return out

    # ---- component surfaces (CollisionMapGrid::ExtractComponentSurfaces, include/sdfgpu.h) -----------------
    def component_surfaces(self, labels, select=None, max_label=None):
        """labels: uint32 [nx, ny, nz]; select: bool/uint8 [nx, ny, nz] or None (every voxel).  Returns (counts int64
        [max_label + 1], indices uint32 [total]): the selected surface voxels grouped by ascending label, ascending inside each
        group (group c starts at counts[:c].sum()).  max_label defaults to the largest label."""
        lab = np.ascontiguousarray(labels, dtype=np.uint32)
        if lab.ndim != 3:
            raise ValueError("labels must be [nx, ny, nz]")
        if max_label is None:
            max_label = int(lab.max()) if lab.size else 0
        sel = None
        if select is not None:
            sel = np.ascontiguousarray(np.asarray(select) != 0, dtype=np.uint8)
            if sel.shape != lab.shape:
                raise ValueError("select must have the labels' shape")
        counts = np.zeros(int(max_label) + 1, np.int64)
        idx = np.empty(max(lab.size, 1), np.uint32)           # (every voxel can be a surface voxel)
        total = ctypes.c_int64(0)
        self._check(self._lib.sdfgpu_component_surfaces(self._h, lab.ctypes.data, None if sel is None else sel.ctypes.data, *lab.shape,
                                                         int(max_label), counts.ctypes.data, idx.ctypes.data, lab.size, ctypes.byref(total)))
        return counts, idx[:total.value].copy()

    def component_surfaces_device(self, d_labels, shape, max_label, d_select_bits=None, d_indices=None, capacity=0, d_surface_bits=None,
                                  stream=0, counts_only=False):
        """d_labels: device uint32 [n]; d_select_bits: device bit field (ceil(n / 32) words) or None; d_surface_bits: device bit
        field to receive the reported voxels, or None.  With d_indices (device uint32 [capacity]) the indices stay on the device
        and the call returns (counts, total); a capacity below the total raises SdfGpuError, whose `total` attribute then holds
        the number needed.  With counts_only it returns (counts, total) and sorts nothing.  Otherwise the indices are fetched:
        (counts int64 [max_label + 1], indices uint32 [total]).  Synchronises `stream`."""
        nx, ny, nz = (int(s) for s in shape)
        counts = np.zeros(int(max_label) + 1, np.int64)
        total = ctypes.c_int64(-1)

        def call(d_idx, cap):
            try:
                self._check(self._lib.sdfgpu_component_surfaces_device(self._h, d_labels, d_select_bits or None, nx, ny, nz, int(max_label),
                                                                        counts.ctypes.data, d_idx or None, int(cap), ctypes.byref(total),
                                                                        d_surface_bits or None, stream or None))
            except SdfGpuError as e:
                e.total = int(total.value)
                raise
        if d_indices or counts_only:
            call(d_indices, capacity)
            return counts, int(total.value)
        call(None, 0)
        n_idx = int(total.value)
        idx = np.empty(n_idx, np.uint32)
        if n_idx:
            d_idx = self.device_malloc(n_idx * 4)
            try:
                call(d_idx, n_idx)
                self.copy_to_host(idx, d_idx, stream)
            finally:
                self.device_free(d_idx)
        return counts, idx

    def component_surfaces_cells(self, cells, shape, class_mask, max_label, cell_stride=8, occupancy_offset=0, component_offset=4):
        """cells: contiguous records (COLLISION_CELL: 8, 0, 4; TAGGED_OBJECT_COLLISION_CELL: 16, 0, 4) holding labels;
        class_mask: TOPOLOGY_FILLED | TOPOLOGY_EMPTY | TOPOLOGY_UNKNOWN (7 = every voxel).  Returns (counts int64 [max_label + 1],
        indices uint32 [total])."""
        nx, ny, nz = (int(s) for s in shape)
        if not (isinstance(cells, np.ndarray) and cells.flags.c_contiguous):
            raise ValueError("cells must be a C-contiguous numpy array")
        if cells.nbytes != nx * ny * nz * cell_stride:
            raise ValueError("cells buffer size does not match shape * cell_stride")
        counts = np.zeros(int(max_label) + 1, np.int64)
        idx = np.empty(max(nx * ny * nz, 1), np.uint32)
        total = ctypes.c_int64(0)
        self._check(self._lib.sdfgpu_component_surfaces_cells(self._h, cells.ctypes.data, cell_stride, occupancy_offset, component_offset,
                                                               nx, ny, nz, int(class_mask), int(max_label), counts.ctypes.data,
                                                               idx.ctypes.data, nx * ny * nz, ctypes.byref(total)))
        return counts, idx[:total.value].copy()

    # ---- local extrema and convex segments (ComputeLocalExtremaMap / UpdateConvexSegments, include/sdfgpu.h) -----------------
    def local_extrema(self, sdf, resolution, q=(1.0, 0.0, 0.0, 0.0)):
        """sdf: float32 [nx, ny, nz]; q: (w, x, y, z) of the origin rotation.  Returns the extremum indices, uint32 [nx, ny, nz]
        (EXTREMUM_OFF where the walk leaves the grid; extremum_locations() gives the reference's map)."""
        f = np.ascontiguousarray(sdf, dtype=np.float32)
        if f.ndim != 3:
            raise ValueError("sdf must be [nx, ny, nz]")
        out = np.empty(f.shape, np.uint32)
        qq = (ctypes.c_double * 8)(*quaternion_and_inverse(q))
        self._check(self._lib.sdfgpu_local_extrema(self._h, f.ctypes.data, *f.shape, float(resolution), qq, out.ctypes.data))
        return out

    def local_extrema_device(self, d_sdf, shape, resolution, d_extremum, q=(1.0, 0.0, 0.0, 0.0), stream=0):
        nx, ny, nz = (int(s) for s in shape)
        qq = (ctypes.c_double * 8)(*quaternion_and_inverse(q))
        self._check(self._lib.sdfgpu_local_extrema_device(self._h, d_sdf, nx, ny, nz, float(resolution), qq, d_extremum, stream or None))

    def convex_segments_cells(self, cells, shape, resolution, connected_threshold, add_virtual_border, q=(1.0, 0.0, 0.0, 0.0),
                              cell_stride=16, occupancy_offset=0, object_id_offset=8, segment_offset=12):
        """cells: writable contiguous records (TAGGED_OBJECT_COLLISION_CELL: 16 bytes, occupancy 0, object id 8, segment 12); the
        segment labels are written into them in place.  Returns K."""
        nx, ny, nz = (int(s) for s in shape)
        if not (isinstance(cells, np.ndarray) and cells.flags.c_contiguous and cells.flags.writeable):
            raise ValueError("cells must be a writable C-contiguous numpy array")
        if cells.nbytes != nx * ny * nz * cell_stride:
            raise ValueError("cells buffer size does not match shape * cell_stride")
        k = ctypes.c_uint32(0)
        qq = (ctypes.c_double * 8)(*quaternion_and_inverse(q))
        self._check(self._lib.sdfgpu_convex_segments_cells(self._h, cells.ctypes.data, cell_stride, occupancy_offset, object_id_offset,
                                                           segment_offset, nx, ny, nz, float(resolution), qq, float(connected_threshold),
                                                           int(bool(add_virtual_border)), ctypes.byref(k)))
        return int(k.value)

    def project_points(self, d_sdf, shape, resolution, points, world_to_grid, grid_to_world, minimum_distance=0.0,
                       stepsize_multiplier=1.0 / 8.0, max_steps=0, into_valid_volume_only=False):
        """Projection out of collision (or into the valid volume) of host points [n, 3] float64 against a field in HBM (d_sdf:
        device address).  world_to_grid / grid_to_world: 3x4 (or 4x4) transforms.  Returns (points [n, 3], status uint8 [n],
        steps int32 [n])."""
        nx, ny, nz = (int(v) for v in shape)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        out, status, steps = np.empty((n, 3), np.float64), np.empty(n, np.uint8), np.empty(n, np.int32)
        w, g = _transform12(world_to_grid), _transform12(grid_to_world)
        mode = PROJECT_INTO_VALID_VOLUME if into_valid_volume_only else PROJECT_OUT_OF_COLLISION
        self._check(self._lib.sdfgpu_project_points(self._h, ctypes.c_void_p(int(d_sdf)), nx, ny, nz, float(resolution), w, g,
                                                    float(minimum_distance), float(stepsize_multiplier), int(max_steps), mode,
                                                    pts.ctypes.data, n, out.ctypes.data, status.ctypes.data, steps.ctypes.data))
        return out, status, steps

    def project_points_device(self, d_sdf, shape, resolution, d_points, n_points, d_out_points, world_to_grid, grid_to_world,
                              minimum_distance=0.0, stepsize_multiplier=1.0 / 8.0, max_steps=0, into_valid_volume_only=False,
                              d_status=0, d_steps=0, stream=0, mode=None):
        """Device form of project_points (device addresses as ints; d_status / d_steps may be 0), enqueued on `stream`."""
        nx, ny, nz = (int(v) for v in shape)
        w, g = _transform12(world_to_grid), _transform12(grid_to_world)
        if mode is None:
            mode = PROJECT_INTO_VALID_VOLUME if into_valid_volume_only else PROJECT_OUT_OF_COLLISION
        self._check(self._lib.sdfgpu_project_points_device(
            self._h, d_sdf or None, nx, ny, nz, float(resolution), w, g, float(minimum_distance), float(stepsize_multiplier),
            int(max_steps), int(mode), d_points or None, int(n_points), d_out_points or None, d_status or None, d_steps or None,
            stream or None))

    def query_gradients(self, d_sdf, shape, resolution, points, world_to_grid, kind, window=0.0, oob_value=math.inf, outputs=True):
        """Smooth / autodiff gradients or distances to the boundary (kind QUERY_*) of host points [n, 3] float64 against a field in
        HBM (d_sdf: device address).  world_to_grid: 3x4 (or 4x4).  Returns (value [n], gradient [n, 3], status uint8 [n]);
        outputs=False passes NULL for all three (and returns None)."""
        nx, ny, nz = (int(v) for v in shape)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        value, grad, status = np.empty(n, np.float64), np.empty((n, 3), np.float64), np.empty(n, np.uint8)
        self._check(self._lib.sdfgpu_query_gradients(self._h, ctypes.c_void_p(int(d_sdf)), nx, ny, nz, float(resolution),
                                                     _transform12(world_to_grid), float(oob_value), int(kind), float(window),
                                                     pts.ctypes.data if n else None, n, value.ctypes.data if outputs else None,
                                                     grad.ctypes.data if outputs else None, status.ctypes.data if outputs else None))
        return (value, grad, status) if outputs else None

    def query_gradients_device(self, d_sdf, shape, resolution, d_points, n_points, world_to_grid, kind, window=0.0,
                               oob_value=math.inf, d_value=0, d_gradient=0, d_status=0, stream=0):
        """Device form of query_gradients (device addresses as ints; any output may be 0), enqueued on `stream`."""
        nx, ny, nz = (int(v) for v in shape)
        self._check(self._lib.sdfgpu_query_gradients_device(
            self._h, d_sdf or None, nx, ny, nz, float(resolution), _transform12(world_to_grid), float(oob_value), int(kind),
            float(window), d_points or None, int(n_points), d_value or None, d_gradient or None, d_status or None, stream or None))

    # ---- Resample (CollisionMapGrid / TaggedObjectCollisionMapGrid::Resample, include/sdfgpu.h) -----------------
    def _resample_geometry(self, shape, src_cell, origin, dst_inverse_origin, dst_inv_cell, dst_shape, fill_cell, cell_bytes):
        fill = np.ascontiguousarray(fill_cell).view(np.uint8).reshape(-1)
        if fill.size != cell_bytes:
            raise ValueError("fill_cell must hold cell_bytes bytes")
        return ([int(v) for v in shape], _doubles(src_cell, 3), _doubles(origin, 16), _doubles(dst_inverse_origin, 16),
                _doubles(dst_inv_cell, 3), [int(v) for v in dst_shape], fill)

    def resample_cells(self, cells, shape, src_cell, origin, dst_inverse_origin, dst_inv_cell, dst_shape, fill_cell, cell_bytes=8):
        """cells: contiguous records (COLLISION_CELL 8 bytes, TAGGED_OBJECT_COLLISION_CELL 16, or 4) of a grid `shape` with cell
        sizes src_cell and the 4 x 4 origin transform; the result grid has dst_shape cells, the 4 x 4 inverse origin transform
        dst_inverse_origin and cell sizes 1 / dst_inv_cell.  Returns (records uint8 [mx, my, mz, cell_bytes], result cells
        written): each result cell holds the source cell of the largest linear index that lands in it, or fill_cell."""
        if not (isinstance(cells, np.ndarray) and cells.flags.c_contiguous):
            raise ValueError("cells must be a C-contiguous numpy array")
        (nx, ny, nz), c, o, inv, ic, (mx, my, mz), fill = self._resample_geometry(shape, src_cell, origin, dst_inverse_origin,
                                                                                dst_inv_cell, dst_shape, fill_cell, cell_bytes)
        if cells.nbytes != nx * ny * nz * cell_bytes:
            raise ValueError("cells buffer size does not match shape * cell_bytes")
        out = np.empty((mx, my, mz, cell_bytes), np.uint8)
        written = ctypes.c_uint64(0)
        self._check(self._lib.sdfgpu_resample_cells(self._h, cells.ctypes.data, cell_bytes, nx, ny, nz, c, o, inv, ic, out.ctypes.data,
                                                    mx, my, mz, fill.ctypes.data, ctypes.byref(written)))
        return out, int(written.value)

    def resample_cells_device(self, d_src, shape, src_cell, origin, dst_inverse_origin, dst_inv_cell, d_dst, dst_shape, fill_cell,
                              cell_bytes=8, count=False, stream=0):
        """Device form of resample_cells (device addresses as ints), enqueued on `stream`.  count: return the number of result
        cells written (synchronises `stream`); otherwise the call returns None with its work pending."""
        (nx, ny, nz), c, o, inv, ic, (mx, my, mz), fill = self._resample_geometry(shape, src_cell, origin, dst_inverse_origin,
                                                                                dst_inv_cell, dst_shape, fill_cell, cell_bytes)
        written = ctypes.c_uint64(0)
        self._check(self._lib.sdfgpu_resample_cells_device(self._h, d_src or None, cell_bytes, nx, ny, nz, c, o, inv, ic, d_dst or None,
                                                           mx, my, mz, fill.ctypes.data, ctypes.byref(written) if count else None,
                                                           stream or None))
        return int(written.value) if count else None

    # ---- display export (the ExportForDisplay family, include/sdfgpu.h "Display export") -----------------
    @staticmethod
    def _draw_keys(draw_keys):
        if draw_keys is None:
            return None, 0, None
        k = np.ascontiguousarray(draw_keys, dtype=np.uint32).reshape(-1)
        n = int(k.size)
        if n == 0:
            k = np.zeros(1, np.uint32)                          # (an empty list is still a list: a non-null pointer)
        return k, n, k.ctypes.data

    def display_select_cells(self, cells, shape, rule, cell_stride=8, occupancy_offset=0, key_offset=4, class_mask=7, surface_only=False,
                             draw_keys=None, draw_zero=True, grouped=False, capacity=None, group_capacity=None):
        """cells: contiguous records; rule: DISPLAY_OCCUPANCY or DISPLAY_KEY_FIELD.  Returns (indices uint32 [total], keys uint32
        [total]) in scan order, or with grouped (indices, keys, group_keys uint32 [G], group_offsets uint32 [G + 1]) ordered by
        (key, index).  Without a capacity a count-only call sizes the arrays first; a short capacity / group_capacity raises
        SdfGpuError whose `total` and `groups` attributes hold the numbers needed."""
        nx, ny, nz = (int(v) for v in shape)
        if not (isinstance(cells, np.ndarray) and cells.flags.c_contiguous):
            raise ValueError("cells must be a C-contiguous numpy array")
        if cells.nbytes != nx * ny * nz * cell_stride:
            raise ValueError("cells buffer size does not match shape * cell_stride")
        total, groups = ctypes.c_int64(-1), ctypes.c_int64(-1)
        dk, n_dk, p_dk = self._draw_keys(draw_keys)
        if capacity is None:                                    # a count-only call sizes the arrays (4 words per VOXEL otherwise)
            self._check(self._lib.sdfgpu_display_select_cells(
                self._h, cells.ctypes.data, cell_stride, occupancy_offset, key_offset, nx, ny, nz, int(rule), int(class_mask),
                int(bool(surface_only)), p_dk, n_dk, int(bool(draw_zero)), 0, None, None, 0, ctypes.byref(total), None, None, 0, None))
        cap = int(total.value) if capacity is None else int(capacity)
        # (at most one group per drawn voxel; the occupancy rule has three keys)
        gcap = (min(cap, 3) if int(rule) == DISPLAY_OCCUPANCY else cap) if group_capacity is None else int(group_capacity)
        idx, keys = np.empty(max(cap, 1), np.uint32), np.empty(max(cap, 1), np.uint32)
        gkeys, goffs = np.empty(max(gcap, 1), np.uint32), np.empty(gcap + 1, np.uint32)
        try:
            self._check(self._lib.sdfgpu_display_select_cells(
                self._h, cells.ctypes.data, cell_stride, occupancy_offset, key_offset, nx, ny, nz, int(rule), int(class_mask),
                int(bool(surface_only)), p_dk, n_dk, int(bool(draw_zero)), int(bool(grouped)), idx.ctypes.data, keys.ctypes.data, cap,
                ctypes.byref(total), gkeys.ctypes.data if grouped else None, goffs.ctypes.data if grouped else None, gcap,
                ctypes.byref(groups) if grouped else None))
        except SdfGpuError as e:
            e.total, e.groups = int(total.value), int(groups.value)
            raise
        t, g = int(total.value), int(groups.value)
        if grouped:
            return idx[:t].copy(), keys[:t].copy(), gkeys[:g].copy(), goffs[:g + 1].copy()
        return idx[:t].copy(), keys[:t].copy()

    def display_select_cells_device(self, d_cells, shape, rule, cell_stride=8, occupancy_offset=0, key_offset=4, class_mask=7,
                                    surface_only=False, draw_keys=None, draw_zero=True, grouped=False, d_indices=None, d_keys=None,
                                    capacity=0, d_group_keys=None, d_group_offsets=None, group_capacity=0, stream=0):
        """Device records and device result arrays (uint32 [capacity]; d_group_offsets [group_capacity + 1]); draw_keys is a host
        list.  Without d_indices only the total is computed.  Returns (total, groups); synchronises `stream`."""
        nx, ny, nz = (int(v) for v in shape)
        total, groups = ctypes.c_int64(-1), ctypes.c_int64(-1)
        dk, n_dk, p_dk = self._draw_keys(draw_keys)
        try:
            self._check(self._lib.sdfgpu_display_select_cells_device(
                self._h, d_cells, cell_stride, occupancy_offset, key_offset, nx, ny, nz, int(rule), int(class_mask), int(bool(surface_only)),
                p_dk, n_dk, int(bool(draw_zero)), int(bool(grouped)), d_indices or None, d_keys or None, int(capacity), ctypes.byref(total),
                d_group_keys or None, d_group_offsets or None, int(group_capacity), ctypes.byref(groups) if grouped else None,
                stream or None))
        except SdfGpuError as e:
            e.total, e.groups = int(total.value), int(groups.value)
            raise
        return int(total.value), int(groups.value) if grouped else 0

    def display_select_contour(self, cells, shape, reach, cell_stride=16, occupancy_offset=0, key_offset=8, unknown_is_filled=True,
                               draw_keys=None, draw_zero=False, grouped=False, capacity=None, group_capacity=None):
        """The object contours (include/sdfgpu.h "Display export: contours"): cells filled for their own key with a cell that is not
        within squared offset `reach` (0 .. 3, display_contour_reach).  Arguments and results as display_select_cells."""
        nx, ny, nz = (int(v) for v in shape)
        if not (isinstance(cells, np.ndarray) and cells.flags.c_contiguous):
            raise ValueError("cells must be a C-contiguous numpy array")
        if cells.nbytes != nx * ny * nz * cell_stride:
            raise ValueError("cells buffer size does not match shape * cell_stride")
        total, groups = ctypes.c_int64(-1), ctypes.c_int64(-1)
        dk, n_dk, p_dk = self._draw_keys(draw_keys)
        head = (self._h, cells.ctypes.data, cell_stride, occupancy_offset, key_offset, nx, ny, nz, int(reach), int(bool(unknown_is_filled)),
                p_dk, n_dk, int(bool(draw_zero)))
        if capacity is None:                                    # a count-only call sizes the arrays
            self._check(self._lib.sdfgpu_display_select_contour(*head, 0, None, None, 0, ctypes.byref(total), None, None, 0, None))
        cap = int(total.value) if capacity is None else int(capacity)
        gcap = cap if group_capacity is None else int(group_capacity)
        idx, keys = np.empty(max(cap, 1), np.uint32), np.empty(max(cap, 1), np.uint32)
        gkeys, goffs = np.empty(max(gcap, 1), np.uint32), np.empty(gcap + 1, np.uint32)
        try:
            self._check(self._lib.sdfgpu_display_select_contour(
                *head, int(bool(grouped)), idx.ctypes.data, keys.ctypes.data, cap, ctypes.byref(total), gkeys.ctypes.data if grouped else None,
                goffs.ctypes.data if grouped else None, gcap, ctypes.byref(groups) if grouped else None))
        except SdfGpuError as e:
            e.total, e.groups = int(total.value), int(groups.value)
            raise
        t, g = int(total.value), int(groups.value)
        if grouped:
            return idx[:t].copy(), keys[:t].copy(), gkeys[:g].copy(), goffs[:g + 1].copy()
        return idx[:t].copy(), keys[:t].copy()

    def display_select_contour_device(self, d_cells, shape, reach, cell_stride=16, occupancy_offset=0, key_offset=8, unknown_is_filled=True,
                                      draw_keys=None, draw_zero=False, grouped=False, d_indices=None, d_keys=None, capacity=0,
                                      d_group_keys=None, d_group_offsets=None, group_capacity=0, stream=0):
        """Device form of display_select_contour (device addresses as ints; draw_keys is a host list).  Without d_indices only the
        total is computed.  Returns (total, groups); synchronises `stream`."""
        nx, ny, nz = (int(v) for v in shape)
        total, groups = ctypes.c_int64(-1), ctypes.c_int64(-1)
        dk, n_dk, p_dk = self._draw_keys(draw_keys)
        try:
            self._check(self._lib.sdfgpu_display_select_contour_device(
                self._h, d_cells, cell_stride, occupancy_offset, key_offset, nx, ny, nz, int(reach), int(bool(unknown_is_filled)), p_dk, n_dk,
                int(bool(draw_zero)), int(bool(grouped)), d_indices or None, d_keys or None, int(capacity), ctypes.byref(total),
                d_group_keys or None, d_group_offsets or None, int(group_capacity), ctypes.byref(groups) if grouped else None, stream or None))
        except SdfGpuError as e:
            e.total, e.groups = int(total.value), int(groups.value)
            raise
        return int(total.value), int(groups.value) if grouped else 0

    def display_select_sdf(self, sdf, capacity=None):
        """sdf: float32 [nx, ny, nz].  Returns the indices of the voxels with d <= 0, ascending (uint32)."""
        f = np.ascontiguousarray(sdf, dtype=np.float32)
        if f.ndim != 3:
            raise ValueError("sdf must be [nx, ny, nz]")
        total = ctypes.c_int64(-1)
        if capacity is None:                                    # a count-only call sizes the array
            self._check(self._lib.sdfgpu_display_select_sdf(self._h, f.ctypes.data, *f.shape, None, 0, ctypes.byref(total)))
        cap = int(total.value) if capacity is None else int(capacity)
        idx = np.empty(max(cap, 1), np.uint32)
        try:
            self._check(self._lib.sdfgpu_display_select_sdf(self._h, f.ctypes.data, *f.shape, idx.ctypes.data, cap, ctypes.byref(total)))
        except SdfGpuError as e:
            e.total = int(total.value)
            raise
        return idx[:total.value].copy()

    def display_select_sdf_device(self, d_sdf, shape, d_indices=None, capacity=0, stream=0):
        """Device field; d_indices: device uint32 [capacity] or None (the total only).  Returns the total; synchronises `stream`."""
        nx, ny, nz = (int(v) for v in shape)
        total = ctypes.c_int64(-1)
        try:
            self._check(self._lib.sdfgpu_display_select_sdf_device(self._h, d_sdf, nx, ny, nz, d_indices or None, int(capacity),
                                                                    ctypes.byref(total), stream or None))
        except SdfGpuError as e:
            e.total = int(total.value)
            raise
        return int(total.value)

    def display_expand_device(self, d_indices, count, shape, cell_sizes, d_points=None, d_colors=None, d_keys=None, d_color_table=None,
                              table_entries=0, default_color=(0.0, 0.0, 0.0, 0.0), stream=0):
        """indices (+ keys) -> d_points (float64 [count, 3], grid frame) and / or d_colors (float32 [count, 4]) from the device table
        (float32 [table_entries, 4]; keys at or past its end get default_color).  Returns with the kernel pending on `stream`."""
        nx, ny, nz = (int(v) for v in shape)
        cs = _doubles(cell_sizes, 3)
        dc = np.ascontiguousarray(default_color, dtype=np.float32).reshape(4)
        self._check(self._lib.sdfgpu_display_expand_device(self._h, d_indices, d_keys or None, int(count), nx, ny, nz, cs,
                                                            d_points or None, d_colors or None, d_color_table or None, int(table_entries),
                                                            dc.ctypes.data, stream or None))

    def display_sdf_colors(self, sdf, alpha):
        """sdf: float32 [nx, ny, nz].  Returns the colour map of SignedDistanceField::ExportForDisplay, float32 [nx, ny, nz, 4]."""
        f = np.ascontiguousarray(sdf, dtype=np.float32)
        if f.ndim != 3:
            raise ValueError("sdf must be [nx, ny, nz]")
        out = np.empty(f.shape + (4,), np.float32)
        self._check(self._lib.sdfgpu_display_sdf_colors(self._h, f.ctypes.data, *f.shape, float(alpha), out.ctypes.data))
        return out

    def display_sdf_colors_device(self, d_sdf, shape, alpha, d_colors, stream=0):
        """Device field -> d_colors (float32 [n, 4]).  Synchronises `stream`."""
        nx, ny, nz = (int(v) for v in shape)
        self._check(self._lib.sdfgpu_display_sdf_colors_device(self._h, d_sdf, nx, ny, nz, float(alpha), d_colors, stream or None))

    # ---- shape rasteriser (include/sdfgpu.h "Shape rasteriser") -------------
    def rasterize_shapes(self, shapes, origin, resolution, shape, bits=True, mask=False, object_ids=False):
        """shapes: a numpy array of SHAPE_DTYPE records (see make_shapes); origin: 4 x 4, grid frame -> world.  Returns a dict of the
        outputs asked for: "bits" uint32 [ceil(n / 32)], "mask" uint8 [nx, ny, nz], "object_ids" uint32 [nx, ny, nz]."""
        nx, ny, nz = (int(v) for v in shape)
        sh = np.ascontiguousarray(shapes, dtype=SHAPE_DTYPE).reshape(-1)
        n = nx * ny * nz
        out = {}
        if bits:
            out["bits"] = np.empty((max(n, 0) + 31) // 32, np.uint32)
        if mask:
            out["mask"] = np.empty((nx, ny, nz), np.uint8)
        if object_ids:
            out["object_ids"] = np.empty((nx, ny, nz), np.uint32)
        ptr = [out[k].ctypes.data if k in out else None for k in ("bits", "mask", "object_ids")]
        self._check(self._lib.sdfgpu_rasterize_shapes(self._h, sh.ctypes.data if sh.size else None, int(sh.size), _doubles(origin, 16),
                                                      float(resolution), nx, ny, nz, *ptr))
        return out

    def rasterize_shapes_device(self, d_shapes, n_shapes, origin, resolution, shape, d_bits=0, d_mask=0, d_object_ids=0, check=False,
                                stream=0):
        """Device form (device addresses as ints), enqueued on `stream`.  check: synchronise the stream and return the index of the
        first refused shape (-1: none; a refused shape also raises); without it the call does not wait and returns None."""
        nx, ny, nz = (int(v) for v in shape)
        bad = ctypes.c_int64(-2)
        self._check(self._lib.sdfgpu_rasterize_shapes_device(self._h, d_shapes or None, int(n_shapes), _doubles(origin, 16), float(resolution),
                                                             nx, ny, nz, d_bits or None, d_mask or None, d_object_ids or None,
                                                             ctypes.byref(bad) if check else None, stream or None))
        return int(bad.value) if check else None

    # ---- mesh rasteriser (include/sdfgpu.h "Planes and triangle meshes") and solid meshes ("Solid meshes") ----
    def _meshes_host(self, call, meshes, vertices, triangles, origin, resolution, shape, bits, mask, object_ids):
        """the host form of either mesh call: the arrays in, a dict of the outputs asked for back"""
        nx, ny, nz = (int(v) for v in shape)
        ms = np.ascontiguousarray(meshes, dtype=MESH_DTYPE).reshape(-1)
        vs = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        ts = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        n = nx * ny * nz
        out = {}
        if bits:
            out["bits"] = np.empty((max(n, 0) + 31) // 32, np.uint32)
        if mask:
            out["mask"] = np.empty((nx, ny, nz), np.uint8)
        if object_ids:
            out["object_ids"] = np.empty((nx, ny, nz), np.uint32)
        ptr = [out[k].ctypes.data if k in out else None for k in ("bits", "mask", "object_ids")]
        self._check(call(self._h, ms.ctypes.data if ms.size else None, int(ms.size),
                         vs.ctypes.data if vs.size else None, len(vs), ts.ctypes.data if ts.size else None, len(ts),
                         _doubles(origin, 16), float(resolution), nx, ny, nz, *ptr))
        return out

    def _meshes_device(self, call, d_meshes, n_meshes, d_vertices, n_vertices, d_triangles, n_triangles, origin, resolution, shape,
                       d_bits, d_mask, d_object_ids, accumulate, check, stream):
        """the device form of either mesh call"""
        nx, ny, nz = (int(v) for v in shape)
        bad = ctypes.c_int64(-2)
        self._check(call(self._h, d_meshes or None, int(n_meshes), d_vertices or None, int(n_vertices),
                         d_triangles or None, int(n_triangles), _doubles(origin, 16), float(resolution),
                         nx, ny, nz, d_bits or None, d_mask or None, d_object_ids or None,
                         int(accumulate), ctypes.byref(bad) if check else None, stream or None))
        return int(bad.value) if check else None

    def rasterize_meshes(self, meshes, vertices, triangles, origin, resolution, shape, bits=True, mask=False, object_ids=False):
        """meshes: MESH_DTYPE records, vertices: float64 [n, 3], triangles: uint32 [m, 3] (see make_meshes).  Returns a dict of the
        outputs asked for, as rasterize_shapes does."""
        return self._meshes_host(self._lib.sdfgpu_rasterize_meshes, meshes, vertices, triangles, origin, resolution, shape, bits, mask, object_ids)

    def rasterize_meshes_device(self, d_meshes, n_meshes, d_vertices, n_vertices, d_triangles, n_triangles, origin, resolution, shape,
                                d_bits=0, d_mask=0, d_object_ids=0, accumulate=False, check=False, stream=0):
        """Device form (device addresses as ints), enqueued on `stream`.  accumulate: OR onto the bits and the mask that are there,
        ids to the smallest non-zero.  check: synchronise the stream and return the index of the first refused mesh (-1: none; a
        refused mesh also raises); without it the call does not wait and returns None."""
        return self._meshes_device(self._lib.sdfgpu_rasterize_meshes_device, d_meshes, n_meshes, d_vertices, n_vertices, d_triangles, n_triangles,
                                   origin, resolution, shape, d_bits, d_mask, d_object_ids, accumulate, check, stream)

    def rasterize_solid_meshes(self, meshes, vertices, triangles, origin, resolution, shape, bits=True, mask=False, object_ids=False):
        """rasterize_meshes with every mesh filled inside (even-odd, per mesh); an open mesh is refused"""
        return self._meshes_host(self._lib.sdfgpu_rasterize_solid_meshes, meshes, vertices, triangles, origin, resolution, shape, bits, mask, object_ids)

    def rasterize_solid_meshes_device(self, d_meshes, n_meshes, d_vertices, n_vertices, d_triangles, n_triangles, origin, resolution, shape,
                                      d_bits=0, d_mask=0, d_object_ids=0, accumulate=False, check=False, stream=0):
        """rasterize_meshes_device with every mesh filled inside; at most MAX_SOLID_MESHES meshes, closedness is not checked"""
        return self._meshes_device(self._lib.sdfgpu_rasterize_solid_meshes_device, d_meshes, n_meshes, d_vertices, n_vertices, d_triangles, n_triangles,
                                   origin, resolution, shape, d_bits, d_mask, d_object_ids, accumulate, check, stream)

    def debug_resample_times(self):
        """(memset + winner kernel, gather kernel) of the last resample call in ms, after set_option("resample_timing", 1)"""
        a, b = ctypes.c_double(), ctypes.c_double()
        self._check(self._lib.sdfgpu_debug_resample_times(self._h, ctypes.byref(a), ctypes.byref(b)))
        return float(a.value), float(b.value)

    def convex_last_info(self):
        """The last extrema computation on this handle: {rounds, cycles, longest_cycle, longest_entry}."""
        r, c, lc, le = ctypes.c_int(0), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(self._lib.sdfgpu_convex_last_info(self._h, ctypes.byref(r), ctypes.byref(c), ctypes.byref(lc), ctypes.byref(le)))
        return {"rounds": r.value, "cycles": c.value, "longest_cycle": lc.value, "longest_entry": le.value}

    def voxelize_points_bits_device(self, d_points, n_points, origin, resolution, shape, d_bits, clear_first=True, stream=0):
        nx, ny, nz = (int(s) for s in shape)
        o = (ctypes.c_double * 3)(*[float(v) for v in origin])
        self._check(self._lib.sdfgpu_voxelize_points_bits_device(self._h, d_points, int(n_points), o, float(resolution),
                                                                 nx, ny, nz, d_bits, int(bool(clear_first)), stream or None))

    def build_cells_device(self, d_cells, shape, d_out, cell_stride=8, occupancy_offset=0,
                           unknown_is_filled=False, resolution=1.0, add_virtual_border=False, stream=0):
        nx, ny, nz = (int(s) for s in shape)
        self._check(self._lib.sdfgpu_build_cells_device(self._h, d_cells, cell_stride, occupancy_offset,
                                                        int(bool(unknown_is_filled)), nx, ny, nz,
                                                        float(resolution), int(bool(add_virtual_border)),
                                                        d_out, stream or None))

    def classify_cells_device(self, d_cells, n_cells, d_mask, cell_stride=8, occupancy_offset=0, unknown_is_filled=False, stream=0):
        """The CollisionMapGrid predicate on n_cells raw device records -> device byte mask (1 = filled)."""
        self._check(self._lib.sdfgpu_classify_cells_device(self._h, d_cells, cell_stride, occupancy_offset,
                                                           int(bool(unknown_is_filled)), int(n_cells), d_mask, stream or None))

    # ---- batches of same-shape grids (include/sdfgpu.h "Batches of same-shape grids") ----
    @staticmethod
    def _batch_resolutions(resolution, batch):
        """(scalar, array or None): one resolution for every grid, or one per grid."""
        if np.ndim(resolution) == 0:
            return float(resolution), None
        r = np.ascontiguousarray(resolution, dtype=np.float64)
        if r.shape != (batch,):
            raise ValueError("resolutions must hold one entry per grid")
        return float(r[0]), r

    def build_batch(self, filled, resolution=1.0, add_virtual_border=False):
        """filled: uint8/bool [B,nx,ny,nz]; resolution: a scalar or B values.  Returns (sdf float32 [B,nx,ny,nz], [(max, min)] * B)."""
        m = np.ascontiguousarray(filled, dtype=np.uint8)
        if m.ndim != 4:
            raise ValueError("masks must be [B, nx, ny, nz]")
        res, arr = self._batch_resolutions(resolution, m.shape[0])
        out = np.empty(m.shape, dtype=np.float32)
        mx = np.empty(m.shape[0], np.float64)
        mn = np.empty(m.shape[0], np.float64)
        self._check(self._lib.sdfgpu_build_batch(self._h, m.ctypes.data, *m.shape, res, arr.ctypes.data if arr is not None else None,
                                                 int(bool(add_virtual_border)), out.ctypes.data, mx.ctypes.data, mn.ctypes.data))
        return out, [(float(a), float(b)) for a, b in zip(mx, mn)]

    def build_batch_device(self, d_filled, batch, shape, d_out, resolution=1.0, add_virtual_border=False, stream=0):
        nx, ny, nz = (int(s) for s in shape)
        res, arr = self._batch_resolutions(resolution, int(batch))
        self._check(self._lib.sdfgpu_build_batch_device(self._h, d_filled, int(batch), nx, ny, nz, res,
                                                        arr.ctypes.data if arr is not None else None,
                                                        int(bool(add_virtual_border)), d_out, stream or None))

    def get_extrema_batch(self, batch):
        mx = np.empty(int(batch), np.float64)
        mn = np.empty(int(batch), np.float64)
        self._check(self._lib.sdfgpu_get_extrema_batch(self._h, int(batch), mx.ctypes.data, mn.ctypes.data))
        return [(float(a), float(b)) for a, b in zip(mx, mn)]

    def build_tagged_objects(self, cells, shape, object_ids, unknown_is_filled=False, resolution=1.0, add_virtual_border=False,
                             cell_stride=16, occupancy_offset=0, object_id_offset=8):
        """One field per object id from one grid of raw TAGGED_OBJECT_COLLISION_CELL records (cells=None: the records of the
        previous tagged call).  Returns (sdf float32 [len(object_ids),nx,ny,nz], [(max, min)] per id)."""
        nx, ny, nz = (int(s) for s in shape)
        c = None
        if cells is not None:
            c = np.ascontiguousarray(cells)
            if c.nbytes != nx * ny * nz * cell_stride:
                raise ValueError("cells buffer size does not match shape * cell_stride")
        ids = np.ascontiguousarray(np.asarray(object_ids, dtype=np.uint32))
        out = np.empty((ids.size, nx, ny, nz), dtype=np.float32)
        mx = np.empty(ids.size, np.float64)
        mn = np.empty(ids.size, np.float64)
        self._check(self._lib.sdfgpu_build_tagged_objects(
            self._h, c.ctypes.data if c is not None else None, cell_stride, occupancy_offset, object_id_offset,
            ids.ctypes.data if ids.size else None, int(ids.size), int(bool(unknown_is_filled)), nx, ny, nz, float(resolution),
            int(bool(add_virtual_border)), out.ctypes.data, mx.ctypes.data, mn.ctypes.data))
        return out, [(float(a), float(b)) for a, b in zip(mx, mn)]

    def gradient_batch_device(self, d_sdf, batch, shape, d_out, resolution=1.0, enable_edge_gradients=True, f64=True, stream=0):
        nx, ny, nz = (int(s) for s in shape)
        res, arr = self._batch_resolutions(resolution, int(batch))
        self._check(self._lib.sdfgpu_gradient_batch_device(self._h, d_sdf, int(batch), nx, ny, nz, res,
                                                           arr.ctypes.data if arr is not None else None,
                                                           int(bool(enable_edge_gradients)), int(bool(f64)), d_out, stream or None))

    def last_batch_info(self):
        """(fast_path, launches) of the last batch build: launches is 2 on the fast path, -1 (not counted) otherwise."""
        f = ctypes.c_int(0)
        n = ctypes.c_int(0)
        self._check(self._lib.sdfgpu_last_batch_info(self._h, ctypes.byref(f), ctypes.byref(n)))
        return bool(f.value), int(n.value)

    def get_extrema(self):
        ext = (ctypes.c_double * 2)()
        self._check(self._lib.sdfgpu_get_extrema(self._h, ctypes.byref(ext, 0), ctypes.byref(ext, 8)))
        return float(ext[0]), float(ext[1])

    def sweep_zy_device(self, d_filled, slab_shape, d_plane_dsq, stream=0):
        nxs, ny, nz = (int(s) for s in slab_shape)
        self._check(self._lib.sdfgpu_sweep_zy_device(self._h, d_filled, nxs, ny, nz, d_plane_dsq, stream or None))

    def sweep_zy_tiered_device(self, d_filled, slab_shape, d_plane_dsq, d_far=0, stream=0):
        nxs, ny, nz = (int(s) for s in slab_shape)
        self._check(self._lib.sdfgpu_sweep_zy_tiered_device(self._h, d_filled, nxs, ny, nz, d_plane_dsq, d_far or None,
                                                            stream or None))

    def sweep_x_lines_device(self, d_plane_dsq, nx, nys, nz, y_global, ny_global, resolution, add_virtual_border, d_out,
                             d_maxdsq, stream=0):
        self._check(self._lib.sdfgpu_sweep_x_lines_device(self._h, d_plane_dsq, int(nx), int(nys), int(nz), int(y_global),
                                                          int(ny_global), float(resolution), int(bool(add_virtual_border)),
                                                          d_out, d_maxdsq, stream or None))

    def sweep_x_device(self, d_plane_dsq, halo_lo, nxs, halo_hi, ny, nz, lo_truncated, hi_truncated,
                       x_global, nx_global, resolution, add_virtual_border, d_out, d_maxdsq, d_status, stream=0):
        self._check(self._lib.sdfgpu_sweep_x_device(self._h, d_plane_dsq, int(halo_lo), int(nxs), int(halo_hi),
                                                    int(ny), int(nz), int(bool(lo_truncated)),
                                                    int(bool(hi_truncated)), int(x_global), int(nx_global),
                                                    float(resolution), int(bool(add_virtual_border)),
                                                    d_out, d_maxdsq, d_status or None, stream or None))

    def pack_bits_device(self, d_filled, n_rows, nz, d_bits, stream=0):
        self._check(self._lib.sdfgpu_pack_bits_device(self._h, d_filled, int(n_rows), int(nz), d_bits, stream or None))

    def dense_ball_device(self, d_bits, rows_x, out_lo, out_hi, ny, nz, resolution, d_out, d_maxdsq, d_uncertified,
                          stream=0):
        self._check(self._lib.sdfgpu_dense_ball_device(self._h, d_bits, int(rows_x), int(out_lo), int(out_hi), int(ny),
                                                       int(nz), float(resolution), d_out, d_maxdsq, d_uncertified,
                                                       stream or None))

    def voxelize_points_device(self, d_points, n_points, origin, resolution, shape, d_mask, clear_first=True, stream=0):
        nx, ny, nz = (int(s) for s in shape)
        o = (ctypes.c_double * 3)(*[float(v) for v in origin])
        self._check(self._lib.sdfgpu_voxelize_points_device(self._h, d_points, int(n_points), o, float(resolution),
                                                            nx, ny, nz, d_mask, int(bool(clear_first)), stream or None))

    def gradient_device(self, d_sdf, shape, d_out, resolution=1.0, enable_edge_gradients=True, f64=True, stream=0):
        nx, ny, nz = (int(s) for s in shape)
        self._check(self._lib.sdfgpu_gradient_device(self._h, d_sdf, nx, ny, nz, float(resolution),
                                                     int(bool(enable_edge_gradients)), d_out, int(bool(f64)),
                                                     stream or None))

    def copy_to_host(self, dst, d_src, stream=0):
        """device pointer -> numpy array (may be untouched memory) at link rate; returns dst."""
        self._check(self._lib.sdfgpu_copy_to_host(self._h, dst.ctypes.data, int(d_src), dst.nbytes, int(stream)))
        return dst

    def copy_from_host(self, d_dst, src, stream=0):
        """numpy array -> device pointer at link rate."""
        a = np.ascontiguousarray(src)
        self._check(self._lib.sdfgpu_copy_from_host(self._h, int(d_dst), a.ctypes.data, a.nbytes, int(stream)))

    def upload_classified(self, d_mask, filled=None, cells=None, cell_stride=8, occupancy_offset=0, unknown_is_filled=False,
                          stream=0):
        """Host mask (uint8 array) or raw cell records -> device byte mask (0 / 1), classified on the host, 1 bit per voxel
        over PCIe (sdfgpu_upload_classified)."""
        if (filled is None) == (cells is None):
            raise ValueError("exactly one of filled / cells")
        if filled is not None:
            a = np.ascontiguousarray(filled, dtype=np.uint8)
            n = a.size
            self._check(self._lib.sdfgpu_upload_classified(self._h, a.ctypes.data, None, 0, 0, 0, n, int(d_mask), int(stream) or None))
        else:
            a = np.ascontiguousarray(cells)
            n = a.nbytes // cell_stride
            self._check(self._lib.sdfgpu_upload_classified(self._h, None, a.ctypes.data, cell_stride, occupancy_offset,
                                                           int(bool(unknown_is_filled)), n, int(d_mask), int(stream) or None))
        return n

    def gradient(self, sdf, resolution=1.0, enable_edge_gradients=True, f64=True):
        """Host-buffer full-grid gradient: sdf float32 [nx,ny,nz] -> [nx,ny,nz,3] (NaN where the reference has none)."""
        f = np.ascontiguousarray(sdf, dtype=np.float32)
        out = np.empty(f.shape + (3,), dtype=np.float64 if f64 else np.float32)
        self._check(self._lib.sdfgpu_gradient(self._h, f.ctypes.data, *f.shape, float(resolution),
                                              int(bool(enable_edge_gradients)), out.ctypes.data, int(bool(f64))))
        return out

    def redzone_check(self, stream=0):
        """Red-zone mode (SDFGPU_REDZONE=1 / option "redzone"): check every canary now; raises SdfGpuError(REDZONE) naming the buffer."""
        self._check(self._lib.sdfgpu_redzone_check(self._h, stream or None))

    def debug_finish_table(self, d_out, n, resolution, fast=True):
        """float(sqrt(double(D)) * resolution) for D = 0 .. n - 1 into the device buffer d_out: the fp32 form of sdfgpu_finish.hpp
        (fast) or the x sweep's fp64 sequence; returns the number of lanes of the fp32 form that took the fp64 sequence."""
        c = ctypes.c_uint32()
        self._check(self._lib.sdfgpu_debug_finish_table(self._h, d_out, int(n), float(resolution), int(bool(fast)), ctypes.byref(c)))
        return int(c.value)

    def debug_zsweep(self, shape):
        out = np.empty(shape, dtype=np.int16)
        self._check(self._lib.sdfgpu_debug_copy_zsweep(self._h, out.ctypes.data, out.size))
        return out

    def debug_yzsweep(self, shape):
        out = np.empty(shape, dtype=np.int32)
        self._check(self._lib.sdfgpu_debug_copy_yzsweep(self._h, out.ctypes.data, out.size))
        return out

    def debug_flat_habit(self):
        """(score, gate) of the two-valued tiles' device-side habit (include/sdfgpu.h); synchronises."""
        sc, g = ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.sdfgpu_debug_flat_habit(self._h, ctypes.byref(sc), ctypes.byref(g)))
        return sc.value, g.value

    def set_option(self, name, value):
        self._check(self._lib.sdfgpu_set_option(self._h, name.encode(), int(value)))

    def last_build_info(self):
        v = ctypes.c_int()
        self._check(self._lib.sdfgpu_last_build_info(self._h, ctypes.byref(v)))
        return {"fused_zy": bool(v.value & 1), "plane16": bool(v.value & 2), "dense": bool(v.value & 4),
                "standby_far": bool(v.value & 8), "dense3": bool(v.value & 16), "dense3_staged": bool(v.value & 32),
                "far_predicted": bool(v.value & 64), "lines_tiered": bool(v.value & 128),
                "far_x_instance": ((v.value >> 8) & 31) - 1, "standby_single": bool(v.value & (1 << 13))}

    def last_path(self):
        """{'dense_certified', 'far_y', 'far_x'} of the last build (synchronises)."""
        v = ctypes.c_int()
        self._check(self._lib.sdfgpu_last_dense_certified(self._h, ctypes.byref(v)))
        why = (v.value >> 8) & 0xff
        names = ("one_class_tile", "wave_all_undecided", "wave_too_many_undecided", "tile_over_fixup_cap", "beyond_fixup_reach", "beyond_ball", "too_sparse_for_the_shell_pass")
        out = {"dense_certified": bool(v.value & 1), "far_y": bool(v.value & 2), "far_x": bool(v.value & 4)}
        if why:
            out["dense_gave_up"] = [n for k, n in enumerate(names) if why & (1 << k)]
        return out

    def last_dense_certified(self):
        return self.last_path()["dense_certified"]

    def last_build_fused_zy(self):
        return self.last_build_info()["fused_zy"]

    def set_profiling(self, enable=True):
        """False/0 off, True/1 every stage, 2 only the dense ball kernel (two events per build), 3 = 2 on every
        4th build."""
        self._check(self._lib.sdfgpu_set_profiling(self._h, int(enable)))

    def get_stage_times(self):
        """(ms_sum[7] for pack / dense ball / z / y-or-zy / envelope y / x / envelope x, builds) since the
        last call; synchronises."""
        ms = (ctypes.c_double * 7)()
        n = ctypes.c_int64()
        self._check(self._lib.sdfgpu_get_stage_times(self._h, ms, ctypes.byref(n)))
        return [float(v) for v in ms], int(n.value)

    def set_tuning(self, rows_per_chunk_y=0, rows_per_chunk_x=0):
        self._check(self._lib.sdfgpu_set_tuning(self._h, int(rows_per_chunk_y), int(rows_per_chunk_x)))

    def dsh_create(self, inverse_origin=None, cell_size=1.0, chunk_dims=(16, 16, 16), default_cell=0, initial_chunks=0, byte_limit=0):
        """A DshMap on this context (close it before the context)."""
        return DshMap(self, inverse_origin, cell_size, chunk_dims, default_cell, initial_chunks, byte_limit)


# ---- include/sdfgpu.h "Dynamic spatial hashed map" ------------------------------------------------------------------
DSH_NOT_FOUND, DSH_FOUND_IN_CHUNK, DSH_FOUND_IN_CELL = 0, 1, 2
DSH_NOT_SET, DSH_SET_CHUNK, DSH_SET_CELL = 0, 1, 2
DSH_RAY_SKIPPED, DSH_RAY_HIT, DSH_RAY_TRUNCATED = 0, 1, 2
DSH_CHUNK_NOT_REMOVED, DSH_CHUNK_REMOVED = 0, 1
DSH_CAST_SKIPPED, DSH_CAST_CLEAR, DSH_CAST_CLEAR_IN_RANGE, DSH_CAST_BLOCKED = 0, 1, 2, 3
DSH_CAST_SKIP_FIRST, DSH_CAST_SKIP_LAST, DSH_CAST_UNKNOWN_IS_FILLED = 1, 2, 4
DSH_FRONTIER_26 = 1
DSH_COMPONENTS_UNKNOWN_APART = 1
DSH_MAX_CHUNK_CELLS = 32768
DSH_COUNTS_DTYPE = np.dtype([(n, np.uint64) for n in ("chunk_filled", "cell_filled", "capacity_chunks", "table_capacity", "bytes_held",
                                                      "scratch_bytes", "byte_limit")])
DSH_RAY_COUNTS_DTYPE = np.dtype([(n, np.uint64) for n in ("rays_hit", "rays_truncated", "rays_skipped", "cells_carved", "new_chunks")])
DSH_SENSOR_MODEL_DTYPE = np.dtype([(n, np.float32) for n in ("prob_hit", "prob_miss", "clamp_min", "clamp_max")])
DSH_CAST_HIT_DTYPE = np.dtype([("cell", np.int64, (3,)), ("record", np.uint64), ("t", np.float64), ("step", np.uint32), ("found", np.uint32)])
DSH_SENSOR_MODEL_DEFAULT = (0.7, 0.4, 0.12, 0.97)                             # octomap's numbers
DSH_CHUNK_DTYPE = np.dtype([("c", np.int64, (3,)), ("state", np.uint32), ("reserved", np.uint32), ("record", np.uint64),
                            ("first_cell", np.int64)])
# include/sdfgpu.h "Component statistics": struct sdfgpu_component_stats (64 bytes)
COMPONENT_STATS_DTYPE = np.dtype([("label", np.uint32), ("reserved", np.uint32), ("count", np.int64), ("sum", np.uint64, (3,)),
                                  ("lo", np.int32, (3,)), ("hi", np.int32, (3,))])


def dsh_record(occupancy, component=0):
    """A COLLISION_CELL {float occupancy; uint32 component} as the uint64 the map moves (little endian: occupancy in the low word)."""
    return int(np.array([occupancy], np.float32).view(np.uint32)[0]) | (int(component) & 0xFFFFFFFF) << 32


class DshMap:
    """One sparse map on a context's GPU (wraps sdfgpu_dsh_create / sdfgpu_dsh_destroy).  Records are uint64 (dsh_record);
    locations are [n, 3] float64; device pointers are integers."""

    def __init__(self, ctx, inverse_origin=None, cell_size=1.0, chunk_dims=(16, 16, 16), default_cell=0, initial_chunks=0, byte_limit=0):
        self._ctx, self._lib = ctx, ctx._lib
        inv = np.eye(4) if inverse_origin is None else np.ascontiguousarray(inverse_origin, dtype=np.float64).reshape(4, 4)
        m = ctypes.c_void_p()
        default = np.array([default_cell], np.uint64)
        ctx._check(self._lib.sdfgpu_dsh_create(ctx._h, inv.ctypes.data, float(cell_size), *(int(d) for d in chunk_dims), default.ctypes.data,
                                               int(initial_chunks), int(byte_limit), ctypes.byref(m)))
        self._m = m
        self.chunk_dims = tuple(int(d) for d in chunk_dims)
        self.cells_per_chunk = int(np.prod(self.chunk_dims))

    def close(self):
        if getattr(self, "_m", None) and getattr(self._ctx, "_h", None):
            self._lib.sdfgpu_dsh_destroy(self._m)
        self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        self._ctx._check(rc)

    def info(self):
        out = np.zeros(1, DSH_COUNTS_DTYPE)
        self._check(self._lib.sdfgpu_dsh_info(self._m, out.ctypes.data))
        return {k: int(out[0][k]) for k in DSH_COUNTS_DTYPE.names}

    @staticmethod
    def _values(value, n):
        """(values array or None, one-value array or None): a scalar is the batch's one record"""
        if np.ndim(value) == 0:
            return None, np.array([value], np.uint64)
        v = np.ascontiguousarray(value, dtype=np.uint64).reshape(-1)
        if v.size != n:
            raise ValueError("one value per operation (or a scalar)")
        return v, None

    def _set(self, call, locations, value, statuses):
        loc = np.ascontiguousarray(locations, dtype=np.float64).reshape(-1, 3)
        values, one = self._values(value, len(loc))
        st = np.zeros(len(loc), np.uint8) if statuses else None
        self._check(call(self._m, loc.ctypes.data, len(loc), None if values is None else values.ctypes.data, None if one is None else one.ctypes.data,
                         None if st is None else st.ctypes.data))
        return st

    def set_cells(self, locations, value, statuses=True):
        return self._set(self._lib.sdfgpu_dsh_set_cells, locations, value, statuses)

    def set_chunks(self, locations, value, statuses=True):
        return self._set(self._lib.sdfgpu_dsh_set_chunks, locations, value, statuses)

    def _set_device(self, call, d_locations, n, d_values, one_value, d_statuses, stream):
        one = None if one_value is None else np.array([one_value], np.uint64)
        self._check(call(self._m, d_locations, int(n), d_values or None, None if one is None else one.ctypes.data, d_statuses or None, stream or None))

    def set_cells_device(self, d_locations, n, d_values=0, one_value=None, d_statuses=0, stream=0):
        self._set_device(self._lib.sdfgpu_dsh_set_cells_device, d_locations, n, d_values, one_value, d_statuses, stream)

    def set_chunks_device(self, d_locations, n, d_values=0, one_value=None, d_statuses=0, stream=0):
        self._set_device(self._lib.sdfgpu_dsh_set_chunks_device, d_locations, n, d_values, one_value, d_statuses, stream)

    def insert_points_device(self, d_points, n, one_value, d_statuses=0, stream=0):
        one = np.array([one_value], np.uint64)
        self._check(self._lib.sdfgpu_dsh_insert_points_device(self._m, d_points, int(n), one.ctypes.data, d_statuses or None, stream or None))

    def insert_rays(self, sensor, points, max_range, free_value, hit_value):
        """One frame of sensor rays (sdfgpu_dsh_insert_rays): points float32 [n, 3] -> (statuses uint8 [n], counts dict)"""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        s = np.ascontiguousarray(sensor, dtype=np.float64).reshape(3)
        free, hit = np.array([free_value], np.uint64), np.array([hit_value], np.uint64)
        st, counts = np.zeros(len(pts), np.uint8), np.zeros(1, DSH_RAY_COUNTS_DTYPE)
        self._check(self._lib.sdfgpu_dsh_insert_rays(self._m, s.ctypes.data, pts.ctypes.data, len(pts), float(max_range), free.ctypes.data, hit.ctypes.data,
                                                     st.ctypes.data, counts.ctypes.data))
        return st, {k: int(counts[0][k]) for k in DSH_RAY_COUNTS_DTYPE.names}

    def insert_rays_device(self, sensor, d_points, n, max_range, free_value, hit_value, d_statuses=0, stream=0):
        """The device form on `stream` (points float32 [n, 3] in device memory); returns the counts dict"""
        s = np.ascontiguousarray(sensor, dtype=np.float64).reshape(3)
        free, hit = np.array([free_value], np.uint64), np.array([hit_value], np.uint64)
        counts = np.zeros(1, DSH_RAY_COUNTS_DTYPE)
        self._check(self._lib.sdfgpu_dsh_insert_rays_device(self._m, s.ctypes.data, d_points or None, int(n), float(max_range), free.ctypes.data,
                                                            hit.ctypes.data, d_statuses or None, counts.ctypes.data, stream or None))
        return {k: int(counts[0][k]) for k in DSH_RAY_COUNTS_DTYPE.names}

    @staticmethod
    def _model(model):
        """(prob_hit, prob_miss, clamp_min, clamp_max), or None for the defaults -> one DSH_SENSOR_MODEL_DTYPE record"""
        out = np.zeros(1, DSH_SENSOR_MODEL_DTYPE)
        out[0] = tuple(DSH_SENSOR_MODEL_DEFAULT if model is None else model)
        return out

    def fuse_rays(self, sensor, points, max_range, model=None):
        """One frame of sensor rays fused into the occupancies (sdfgpu_dsh_fuse_rays): points float32 [n, 3], model a tuple
        (prob_hit, prob_miss, clamp_min, clamp_max) or None for DSH_SENSOR_MODEL_DEFAULT -> (statuses uint8 [n], counts dict)"""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        s = np.ascontiguousarray(sensor, dtype=np.float64).reshape(3)
        mdl = self._model(model)
        st, counts = np.zeros(len(pts), np.uint8), np.zeros(1, DSH_RAY_COUNTS_DTYPE)
        self._check(self._lib.sdfgpu_dsh_fuse_rays(self._m, s.ctypes.data, pts.ctypes.data, len(pts), float(max_range), mdl.ctypes.data, st.ctypes.data,
                                                   counts.ctypes.data))
        return st, {k: int(counts[0][k]) for k in DSH_RAY_COUNTS_DTYPE.names}

    def fuse_rays_device(self, sensor, d_points, n, max_range, model=None, d_statuses=0, stream=0):
        """The device form on `stream` (points float32 [n, 3] in device memory); returns the counts dict"""
        s = np.ascontiguousarray(sensor, dtype=np.float64).reshape(3)
        mdl = self._model(model)
        counts = np.zeros(1, DSH_RAY_COUNTS_DTYPE)
        self._check(self._lib.sdfgpu_dsh_fuse_rays_device(self._m, s.ctypes.data, d_points or None, int(n), float(max_range), mdl.ctypes.data,
                                                          d_statuses or None, counts.ctypes.data, stream or None))
        return {k: int(counts[0][k]) for k in DSH_RAY_COUNTS_DTYPE.names}

    def remove_chunks(self, locations, statuses=True):
        """Remove the chunks of the locations, in list order (sdfgpu_dsh_remove_chunks) -> (statuses uint8 [n] or None, removed)"""
        loc = np.ascontiguousarray(locations, dtype=np.float64).reshape(-1, 3)
        st = np.zeros(len(loc), np.uint8) if statuses else None
        removed = ctypes.c_int64()
        self._check(self._lib.sdfgpu_dsh_remove_chunks(self._m, loc.ctypes.data, len(loc), None if st is None else st.ctypes.data, ctypes.byref(removed)))
        return st, removed.value

    def remove_chunks_device(self, d_locations, n, d_statuses=0, stream=0):
        """The device form on `stream` (locations float64 [n, 3] in device memory); returns the number of chunks removed"""
        removed = ctypes.c_int64()
        self._check(self._lib.sdfgpu_dsh_remove_chunks_device(self._m, d_locations or None, int(n), d_statuses or None, ctypes.byref(removed), stream or None))
        return removed.value

    def retain_box(self, lower, extent, invert=False, stream=0):
        """Remove every chunk that holds no cell of the box of global cells lower .. lower + extent - 1 (invert: every chunk that
        holds at least one); returns the number of chunks removed"""
        lo = np.array([int(v) for v in lower], np.int64).reshape(3)
        ext = np.array([int(v) for v in extent], np.int64).reshape(3)
        removed = ctypes.c_int64()
        self._check(self._lib.sdfgpu_dsh_retain_box(self._m, lo.ctypes.data, ext.ctypes.data, int(bool(invert)), ctypes.byref(removed), stream or None))
        return removed.value

    def remove_box(self, lower, extent, stream=0):
        return self.retain_box(lower, extent, True, stream)

    def clear(self, stream=0):
        """Remove every chunk (the empty box retains nothing); returns the number of chunks removed"""
        return self.retain_box((0, 0, 0), (0, 0, 0), False, stream)

    def shrink(self, spare_chunks=0, stream=0):
        """Hand memory back: the pool to max(live + spare_chunks, 1) chunks, the table to match, the mark plane freed"""
        self._check(self._lib.sdfgpu_dsh_shrink(self._m, int(spare_chunks), stream or None))

    def cast_rays(self, sensor, points, max_range, flags=0, statuses=True, hits=True):
        """The first blocking cell of each ray sensor -> point (sdfgpu_dsh_cast_rays): points float32 [n, 3], flags of DSH_CAST_* ->
        (statuses uint8 [n] or None, hits DSH_CAST_HIT_DTYPE [n] or None)"""
        s = np.ascontiguousarray(sensor, np.float64).reshape(3)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        st = np.zeros(len(pts), np.uint8) if statuses else None
        ht = np.zeros(len(pts), DSH_CAST_HIT_DTYPE) if hits else None
        self._check(self._lib.sdfgpu_dsh_cast_rays(self._m, s.ctypes.data, pts.ctypes.data, len(pts), float(max_range), int(flags),
                                                   None if st is None else st.ctypes.data, None if ht is None else ht.ctypes.data))
        return st, ht

    def cast_rays_device(self, sensor, d_points, n, max_range, flags=0, d_statuses=0, d_hits=0, stream=0):
        """sdfgpu_dsh_cast_rays_device: one kernel on `stream`, pending on return; d_hits takes n records of DSH_CAST_HIT_DTYPE"""
        s = np.ascontiguousarray(sensor, np.float64).reshape(3)
        self._check(self._lib.sdfgpu_dsh_cast_rays_device(self._m, s.ctypes.data, d_points or None, int(n), float(max_range), int(flags), d_statuses or None,
                                                          d_hits or None, stream or None))

    def cast_segments(self, starts, ends, max_range, flags=0, statuses=True, hits=True):
        """The first blocking cell of each segment start -> end (sdfgpu_dsh_cast_segments): float64 [n, 3] each -> as cast_rays"""
        a = np.ascontiguousarray(starts, np.float64).reshape(-1, 3)
        b = np.ascontiguousarray(ends, np.float64).reshape(-1, 3)
        if len(a) != len(b):
            raise ValueError("cast_segments: %d starts and %d ends" % (len(a), len(b)))
        st = np.zeros(len(a), np.uint8) if statuses else None
        ht = np.zeros(len(a), DSH_CAST_HIT_DTYPE) if hits else None
        self._check(self._lib.sdfgpu_dsh_cast_segments(self._m, a.ctypes.data, b.ctypes.data, len(a), float(max_range), int(flags),
                                                       None if st is None else st.ctypes.data, None if ht is None else ht.ctypes.data))
        return st, ht

    def cast_segments_device(self, d_starts, d_ends, n, max_range, flags=0, d_statuses=0, d_hits=0, stream=0):
        self._check(self._lib.sdfgpu_dsh_cast_segments_device(self._m, d_starts or None, d_ends or None, int(n), float(max_range), int(flags),
                                                              d_statuses or None, d_hits or None, stream or None))

    def get(self, locations):
        """(records uint64 [n], statuses uint8 [n])"""
        loc = np.ascontiguousarray(locations, dtype=np.float64).reshape(-1, 3)
        rec, st = np.zeros(len(loc), np.uint64), np.zeros(len(loc), np.uint8)
        self._check(self._lib.sdfgpu_dsh_get(self._m, loc.ctypes.data, len(loc), rec.ctypes.data, st.ctypes.data))
        return rec, st

    def get_device(self, d_locations, n, d_records=0, d_statuses=0, stream=0):
        self._check(self._lib.sdfgpu_dsh_get_device(self._m, d_locations, int(n), d_records or None, d_statuses or None, stream or None))

    def extract_window(self, lower, shape, unknown_is_filled=False, records=True, bits=True):
        """(records uint64 [nx, ny, nz] or None, bits uint32 [ceil(n / 32)] or None)"""
        lo = np.ascontiguousarray(lower, dtype=np.int64).reshape(3)
        nx, ny, nz = (int(s) for s in shape)
        n = nx * ny * nz
        rec = np.zeros(max(n, 0), np.uint64) if records else None
        bit = np.zeros(max((n + 31) // 32, 0), np.uint32) if bits else None
        self._check(self._lib.sdfgpu_dsh_extract_window(self._m, lo.ctypes.data, nx, ny, nz, int(bool(unknown_is_filled)),
                                                        None if rec is None else rec.ctypes.data, None if bit is None else bit.ctypes.data))
        return (None if rec is None else rec.reshape(nx, ny, nz)), bit

    def extract_window_device(self, lower, shape, unknown_is_filled=False, d_records=0, d_bits=0, stream=0):
        lo = np.ascontiguousarray(lower, dtype=np.int64).reshape(3)
        nx, ny, nz = (int(s) for s in shape)
        self._check(self._lib.sdfgpu_dsh_extract_window_device(self._m, lo.ctypes.data, nx, ny, nz, int(bool(unknown_is_filled)), d_records or None,
                                                               d_bits or None, stream or None))

    def frontier_window(self, lower, shape, flags=0):
        """The frontier bits of a window (sdfgpu_dsh_frontier_window): a cell is a frontier cell iff its chunk is live, it is free
        (occupancy < 0.5) and one of its 6 face neighbours (all 26 under DSH_FRONTIER_26) is unknown (== 0.5) -> bits uint32 [ceil(n / 32)]"""
        lo = np.ascontiguousarray(lower, dtype=np.int64).reshape(3)
        nx, ny, nz = (int(s) for s in shape)
        bit = np.zeros(max((nx * ny * nz + 31) // 32, 0), np.uint32)
        self._check(self._lib.sdfgpu_dsh_frontier_window(self._m, lo.ctypes.data, nx, ny, nz, int(flags), bit.ctypes.data))
        return bit

    def frontier_window_device(self, lower, shape, flags=0, d_bits=0, stream=0):
        """sdfgpu_dsh_frontier_window_device: one kernel on `stream`, pending on return; d_bits takes ceil(n / 32) words"""
        lo = np.ascontiguousarray(lower, dtype=np.int64).reshape(3)
        nx, ny, nz = (int(s) for s in shape)
        self._check(self._lib.sdfgpu_dsh_frontier_window_device(self._m, lo.ctypes.data, nx, ny, nz, int(flags), d_bits or None, stream or None))

    @staticmethod
    def _box(lower, extent):
        """(lower, extent) as two int64 [3] arrays, or (None, None) for the whole map"""
        if lower is None and extent is None:
            return None, None
        if lower is None or extent is None:
            raise ValueError("a box is lower and extent, or neither")
        return np.array([int(v) for v in lower], np.int64).reshape(3), np.array([int(v) for v in extent], np.int64).reshape(3)

    def frontier_cells(self, lower=None, extent=None, flags=0):
        """The frontier cells among the cells of live chunks in the box lower .. lower + extent - 1 (the whole map without a box), in
        ascending chunk and cell slot order (sdfgpu_dsh_frontier_cells) -> global cells int64 [total, 3]"""
        lo, ext = self._box(lower, extent)
        args = (None if lo is None else lo.ctypes.data, None if ext is None else ext.ctypes.data, int(flags))
        total = ctypes.c_int64()
        self._check(self._lib.sdfgpu_dsh_frontier_cells(self._m, *args, None, 0, ctypes.byref(total)))
        cells = np.zeros((total.value, 3), np.int64)
        if total.value:
            self._check(self._lib.sdfgpu_dsh_frontier_cells(self._m, *args, cells.ctypes.data, total.value, ctypes.byref(total)))
            assert total.value == len(cells)
        return cells

    def frontier_cells_device(self, lower=None, extent=None, flags=0, d_cells=0, capacity=0, stream=0):
        """sdfgpu_dsh_frontier_cells_device: the list (int64 [3] per cell) goes to d_cells iff `capacity` (in cells) suffices;
        returns the total"""
        lo, ext = self._box(lower, extent)
        total = ctypes.c_int64()
        self._check(self._lib.sdfgpu_dsh_frontier_cells_device(self._m, None if lo is None else lo.ctypes.data, None if ext is None else ext.ctypes.data,
                                                               int(flags), d_cells or None, int(capacity), ctypes.byref(total), stream or None))
        return total.value

    def update_components(self, flags=0, stream=0):
        """Label the connected components of the whole map in place (sdfgpu_dsh_update_components): the component word of every
        cell record, and of every chunk-filled chunk's record, becomes its node's label in 1..K; flags 0 (filled / everything
        else) or DSH_COMPONENTS_UNKNOWN_APART (filled / free / unknown and NaN).  Always recomputes.  Returns K."""
        count = ctypes.c_uint32()
        self._check(self._lib.sdfgpu_dsh_update_components(self._m, int(flags), ctypes.byref(count), stream or None))
        return count.value

    def components_info(self):
        """(K of the last update, the flags it ran under, whether nothing has changed the map's content since): host-only"""
        count, flags, valid = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
        self._check(self._lib.sdfgpu_dsh_components_info(self._m, ctypes.byref(count), ctypes.byref(flags), ctypes.byref(valid)))
        return count.value, flags.value, bool(valid.value)

    def export(self):
        """(chunks DSH_CHUNK_DTYPE [n] in ascending (c_x, c_y, c_z) order, cells uint64 [cell-filled chunks, n_x, n_y, n_z])"""
        nc, ncell = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.sdfgpu_dsh_export(self._m, None, 0, None, 0, ctypes.byref(nc), ctypes.byref(ncell)))
        chunks, cells = np.zeros(nc.value, DSH_CHUNK_DTYPE), np.zeros(ncell.value, np.uint64)
        if nc.value:
            self._check(self._lib.sdfgpu_dsh_export(self._m, chunks.ctypes.data, nc.value, cells.ctypes.data, ncell.value, ctypes.byref(nc), ctypes.byref(ncell)))
            assert nc.value == len(chunks) and ncell.value == len(cells)
        return chunks, cells.reshape((-1,) + self.chunk_dims)

    def export_device(self, d_chunks, chunk_capacity, d_cells, cell_capacity, stream=0):
        """(chunks, cell records) the map holds; the lists are written iff both capacities suffice"""
        nc, ncell = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.sdfgpu_dsh_export_device(self._m, d_chunks or None, int(chunk_capacity), d_cells or None, int(cell_capacity), ctypes.byref(nc),
                                                       ctypes.byref(ncell), stream or None))
        return nc.value, ncell.value


# ---- multi-GPU C ABI (include/sdfgpu_multi.h, libsdfgpu_multi.so) -------------------------------------------------
MULTI_EXPORTS = [
    "sdfgpu_multi_create", "sdfgpu_multi_destroy", "sdfgpu_multi_last_error", "sdfgpu_multi_ranks",
    "sdfgpu_multi_slab_range", "sdfgpu_multi_build", "sdfgpu_multi_build_cells", "sdfgpu_multi_build_device",
    "sdfgpu_multi_last_path", "sdfgpu_multi_set_option", "sdfgpu_multi_last_stats", "sdfgpu_multi_last_host_us",
]
_multi_lib = None


def load_multi_library():
    """dlopen sdf_tools_amd/libsdfgpu_multi.so (x-slab multi-GPU build over RCCL; no CPU fallback)."""
    global _multi_lib
    if _multi_lib is not None:
        return _multi_lib
    load_library()                               # libsdfgpu.so (and torch's HIP / RCCL runtimes) first
    path = _build.LIB_MULTI
    if not os.path.exists(path):
        raise ImportError("libsdfgpu_multi.so is not built (run `python -m sdf_tools_amd.build`)")
    L = ctypes.CDLL(path)
    i64, dbl, ci, vp, sz = ctypes.c_int64, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    L.sdfgpu_multi_create.argtypes = [ci, vp, ctypes.POINTER(vp)]
    L.sdfgpu_multi_destroy.argtypes = [vp]
    L.sdfgpu_multi_last_error.argtypes = [vp]
    L.sdfgpu_multi_last_error.restype = ctypes.c_char_p
    L.sdfgpu_multi_ranks.argtypes = [vp]
    L.sdfgpu_multi_slab_range.argtypes = [vp, i64, ci, vp, vp]
    L.sdfgpu_multi_build.argtypes = [vp, vp, i64, i64, i64, dbl, ci, vp, vp, vp]
    L.sdfgpu_multi_build_cells.argtypes = [vp, vp, sz, sz, ci, i64, i64, i64, dbl, ci, vp, vp, vp]
    L.sdfgpu_multi_build_device.argtypes = [vp, vp, i64, i64, i64, dbl, ci, vp, vp, vp]
    L.sdfgpu_multi_last_path.argtypes = [vp, vp]
    L.sdfgpu_multi_last_stats.argtypes = [vp, vp, vp]
    L.sdfgpu_multi_last_host_us.argtypes = [vp, vp, vp]
    L.sdfgpu_multi_set_option.argtypes = [vp, ctypes.c_char_p, ci]
    for name in MULTI_EXPORTS:
        if name != "sdfgpu_multi_last_error":
            getattr(L, name).restype = ci
    _multi_lib = L
    return L


class MultiSdfGpu:
    """n ranks (one per GPU; the same GPU may be named several times for single-GPU testing) behind sdfgpu_multi_*."""

    def __init__(self, n_ranks, devices=None):
        self._lib = load_multi_library()
        h = ctypes.c_void_p()
        devs = None
        if devices is not None:
            devs = (ctypes.c_int * n_ranks)(*[int(d) for d in devices])
        rc = self._lib.sdfgpu_multi_create(int(n_ranks), devs, ctypes.byref(h))
        if rc != 0:
            raise SdfGpuError(rc, self._lib.sdfgpu_multi_last_error(None).decode())
        self._h = h
        self.n_ranks = int(n_ranks)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sdfgpu_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise SdfGpuError(rc, self._lib.sdfgpu_multi_last_error(self._h).decode())

    def slab_range(self, nx, rank):
        a, b = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.sdfgpu_multi_slab_range(self._h, int(nx), int(rank), ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def set_option(self, name, value):
        self._check(self._lib.sdfgpu_multi_set_option(self._h, name.encode(), int(value)))

    def last_path(self):
        v = ctypes.c_int()
        self._check(self._lib.sdfgpu_multi_last_path(self._h, ctypes.byref(v)))
        return {"dense_certified": bool(v.value & 1), "whole_lines": bool(v.value & 2), "rccl": bool(v.value & 4)}

    def last_stats(self):
        """{'host_reads': status-block round trips of the last build, 'mispredictions': general builds since creation
        whose predicted x sweep had to be redone, 'host_us_max_rank' / 'host_us_sum': host time of the last build inside API
        calls -- the slowest rank thread / the sum over the rank threads (sdfgpu_multi_last_host_us)}."""
        a, b = ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.sdfgpu_multi_last_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        mx, sm = ctypes.c_double(), ctypes.c_double()
        self._check(self._lib.sdfgpu_multi_last_host_us(self._h, ctypes.byref(mx), ctypes.byref(sm)))
        return {"host_reads": int(a.value), "mispredictions": int(b.value),
                "host_us_max_rank": float(mx.value), "host_us_sum": float(sm.value)}

    def build(self, filled, resolution=1.0, add_virtual_border=False):
        m = np.ascontiguousarray(filled, dtype=np.uint8)
        out = np.empty(m.shape, dtype=np.float32)
        ext = (ctypes.c_double * 2)()
        self._check(self._lib.sdfgpu_multi_build(self._h, m.ctypes.data, *m.shape, float(resolution),
                                                 int(bool(add_virtual_border)), out.ctypes.data,
                                                 ctypes.byref(ext, 0), ctypes.byref(ext, 8)))
        return out, (float(ext[0]), float(ext[1]))

    def build_cells(self, cells, shape, cell_stride=8, occupancy_offset=0, unknown_is_filled=False, resolution=1.0,
                    add_virtual_border=False):
        c = np.ascontiguousarray(cells)
        nx, ny, nz = (int(s) for s in shape)
        out = np.empty((nx, ny, nz), dtype=np.float32)
        ext = (ctypes.c_double * 2)()
        self._check(self._lib.sdfgpu_multi_build_cells(self._h, c.ctypes.data, cell_stride, occupancy_offset,
                                                       int(bool(unknown_is_filled)), nx, ny, nz, float(resolution),
                                                       int(bool(add_virtual_border)), out.ctypes.data,
                                                       ctypes.byref(ext, 0), ctypes.byref(ext, 8)))
        return out, (float(ext[0]), float(ext[1]))

    def build_device(self, d_mask_slabs, shape, d_out_slabs, resolution=1.0, add_virtual_border=False):
        """d_mask_slabs / d_out_slabs: per-rank device pointers (ints) of the x slabs."""
        nx, ny, nz = (int(s) for s in shape)
        pm = (ctypes.c_void_p * self.n_ranks)(*[int(p) for p in d_mask_slabs])
        po = (ctypes.c_void_p * self.n_ranks)(*[int(p) for p in d_out_slabs])
        ext = (ctypes.c_double * 2)()
        self._check(self._lib.sdfgpu_multi_build_device(self._h, pm, nx, ny, nz, float(resolution),
                                                        int(bool(add_virtual_border)), po, ctypes.byref(ext, 0),
                                                        ctypes.byref(ext, 8)))
        return float(ext[0]), float(ext[1])
