"""numpy helpers with the conventions of the reference's src/sdf_tools/utils_3d.py:5-108.

Input ``env`` is indexed ``[y, x, z]`` (utils_3d.py:57-60), a voxel is filled where ``env == 1``
(:65), out-of-bounds cell is COLLISION_CELL(-10000) (:21), no virtual border, unknown is free (:68).
Outputs are ``[y, x, z]`` float32 (:74-75) and, for the gradient, ``[y, x, z, 3]`` from
GetGradient(..., enable_edge_gradients=True) (:77-90).  Unlike the reference, no Python loop runs
per voxel: occupancy goes in as one array and the field comes back as one array.
"""
import numpy as np

from ._bindings import load_pysdf_tools


def _origin(origin_point):
    return [[1.0, 0.0, 0.0, origin_point[0]], [0.0, 1.0, 0.0, origin_point[1]],
            [0.0, 0.0, 1.0, origin_point[2]], [0.0, 0.0, 0.0, 1.0]]


def _grid_from_env(env, res, origin_point, frame="world"):
    m = load_pysdf_tools()
    env = np.asarray(env)
    y_shape, x_shape, z_shape = env.shape
    oob_value = m.COLLISION_CELL(-10000)
    grid = m.CollisionMapGrid(m.Isometry3d(_origin(origin_point)), frame, res, x_shape, y_shape, z_shape, oob_value)
    # cells default to the OOB cell (-10000, free); filled cells become occupancy 1 (utils_3d.py:62-67)
    occ = np.where(np.transpose(env, [1, 0, 2]) == 1, np.float32(1.0), np.float32(-10000.0))
    grid.SetOccupancyFromNumpy(np.ascontiguousarray(occ, dtype=np.float32))
    return grid, oob_value


def compute_sdf(env, res, origin_point):
    """:return: pysdf_tools.SignedDistanceField (utils_3d.py:5-36)"""
    grid, oob_value = _grid_from_env(env, res, origin_point)
    return grid.ExtractSignedDistanceField(oob_value.occupancy, False, False)[0]


def compute_sdf_and_gradient(env, res, origin_point):
    """:return: (sdf [y,x,z] float32, gradient [y,x,z,3] float32) (utils_3d.py:39-97)"""
    sdf = compute_sdf(env, res, origin_point)
    np_sdf = np.transpose(sdf.GetRawDataNumpy(), [1, 0, 2]).astype(np.float32)
    np_gradient = np.transpose(sdf.GetFullGradientNumpy(True), [1, 0, 2, 3]).astype(np.float32)
    return np_sdf, np_gradient


def compute_sdf_and_gradient_batch(env, res, origin_point, batch_size):
    """A batch of environments of one shape, each with its own resolution and origin (reference
    src/sdf_tools/utils_3d_tensorflow.py:6-15): env [B, y, x, z], res [B], origin_point [B, 3].
    :return: (sdf [B,y,x,z] float32, gradient [B,y,x,z,3] float32), each entry what compute_sdf_and_gradient returns for it.
    One batched build and one batched gradient on the GPU (sdfgpu_build_batch_device, sdfgpu_gradient_batch_device).  The
    values are in the grid frame, so the origins (pure translations) do not enter them."""
    import torch

    from . import capi

    env = np.asarray(env)
    batch_size = int(batch_size)
    res = np.asarray(res, dtype=np.float64).reshape(-1)
    origin_point = np.asarray(origin_point, dtype=np.float64)
    if env.ndim != 4 or env.shape[0] != batch_size or res.shape != (batch_size,) or origin_point.shape != (batch_size, 3):
        raise ValueError("env must be [batch_size, y, x, z] with one res and one origin_point per environment")
    mask = torch.from_numpy(np.ascontiguousarray(np.transpose(env, [0, 2, 1, 3]) == 1).astype(np.uint8)).cuda()
    shape = tuple(mask.shape[1:])
    sdf = torch.empty(mask.shape, dtype=torch.float32, device="cuda")
    grad = torch.empty(tuple(mask.shape) + (3,), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx = capi.SdfGpu(torch.cuda.current_device())
    try:
        ctx.build_batch_device(mask.data_ptr(), batch_size, shape, sdf.data_ptr(), res, False, stream)
        ctx.gradient_batch_device(sdf.data_ptr(), batch_size, shape, grad.data_ptr(), res, True, True, stream)
        torch.cuda.current_stream().synchronize()
    finally:
        ctx.close()
    np_sdf = np.transpose(sdf.cpu().numpy(), [0, 2, 1, 3])
    np_gradient = np.transpose(grad.cpu().numpy(), [0, 2, 1, 3, 4]).astype(np.float32)
    return np.ascontiguousarray(np_sdf), np.ascontiguousarray(np_gradient)


def get_gradient(sdf, dtype=np.float64):
    """[x, y, z, 3] gradient of a SignedDistanceField (utils_3d.py:100-108)."""
    return sdf.GetFullGradientNumpy(True).astype(dtype)
