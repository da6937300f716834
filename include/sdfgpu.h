/*
 * sdfgpu.h -- C ABI of the MI355X-native signed-distance-field build path.
 *
 * This is the drop-in boundary for the one hot path of UM-ARM-Lab/sdf_tools:
 *
 *   sdf_generation::ExtractSignedDistanceField      include/sdf_tools/sdf_generation.hpp:209-271
 *     = classify (:219-240) + BuildDistanceField x2 (:95-207, called :242-243)
 *       + signed merge / extrema (:245-269)
 *   its virtual-border variant                      include/sdf_tools/sdf_generation.hpp:273-420
 *   the CollisionMapGrid predicate                  include/sdf_tools/collision_map.hpp:680-712
 *
 * A maintainer binds these entry points from the reference's C++ (see
 * INTEGRATION.md); the in-tree mirror of the reference's C++ API
 * (include/sdf_tools/ headers) and the pysdf_tools module call nothing else.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross this boundary
 *   - voxel layout: index = x*ny*nz + y*nz + z (z fastest), the reference's
 *     VoxelGrid layout (src/sdf_tools/sdf.cpp:241-245, utils_3d.py:71-73)
 *   - a device pointer needs the alignment of its element type only (uint8_t* none; float*, int32_t*, uint32_t* and cell
 *     records 4 bytes; a double gradient 8): 16-byte alignment only selects faster kernels, never another result, and a
 *     stage call (sdfgpu_dense_ball_device, sdfgpu_slab_dense_phase) whose bit planes or field are off 16 bytes goes
 *     through copies in the handle's scratch
 *   - every function returns SDFGPU_OK (0) or a negative sdfgpu_status;
 *     nothing throws; sdfgpu_last_error() gives the message for the handle
 *   - a handle is bound to one GPU; use one handle per host thread
 *   - builds on one handle share its scratch fields and status block.  Builds issued on the same stream are
 *     ordered by the stream; a build issued on a different stream than the previous one first waits (on the
 *     device, hipStreamWaitEvent) for the previous build's last kernel.  The tiered stage entry points
 *     (sdfgpu_sweep_zy_device / sdfgpu_sweep_zy_tiered_device, sdfgpu_sweep_x_lines_device) use the status block and
 *     scratch fields too and take part in the same ordering (they wait for the handle's previous work when that ran
 *     on another stream, and later work waits for them).  The remaining stage-level entry points
 *     (sdfgpu_sweep_x_device, sdfgpu_dense_ball_device, sdfgpu_slab_dense_phase ...) write only caller-owned
 *     buffers plus the handle's extrema slots: issue all stage calls of one build on one stream.
 *   - host-buffer entry points use the caller's output buffer as scratch while they run (its pages are
 *     faulted in while the input travels to the GPU): when such a call fails, the contents of out_sdf /
 *     out_grad are undefined
 *   - there is NO CPU fallback: without a usable HIP device sdfgpu_create fails
 */
#ifndef SDFGPU_H
#define SDFGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdfgpu_context* sdfgpu_handle;

typedef enum sdfgpu_status {
    SDFGPU_OK = 0,
    SDFGPU_ERR_INVALID_ARGUMENT = -1, /* null pointer, non-positive dims, bad stride ...          */
    SDFGPU_ERR_HIP = -2,              /* a HIP runtime call failed (maps to std::runtime_error)   */
    SDFGPU_ERR_UNSUPPORTED_SIZE = -3, /* a dim > 16384 or nx^2+ny^2+nz^2 >= 2^30                   */
    SDFGPU_ERR_NO_DEVICE = -4,        /* no HIP device / device index out of range                */
    SDFGPU_ERR_UNRESOLVED = -5,       /* slab x-sweep needed rows beyond the supplied halo        */
    SDFGPU_ERR_REDZONE = -6           /* red-zone mode: a kernel of this call stored outside a buffer of the library (the message names it) */
} sdfgpu_status;

/* Library version, e.g. "sdfgpu 0.1 (gfx950)". */
const char* sdfgpu_version(void);

/* Number of visible HIP devices (0 if none / runtime unusable). */
int sdfgpu_device_count(void);

/* Create / destroy a context on `device`.  The context owns the device scratch
 * (int16 z-sweep field, int32 yz-sweep field, staging buffers) and re-uses it
 * across calls, growing on demand -- needed for the 30 Hz streaming use. */
int sdfgpu_create(int device, sdfgpu_handle* out_handle);
int sdfgpu_destroy(sdfgpu_handle h);

/* Message for the last non-OK status returned on this handle (never NULL).
 * With h == NULL returns the message of the last failed sdfgpu_create. */
const char* sdfgpu_last_error(sdfgpu_handle h);

/* ---------------------------------------------------------------------------
 * Resolutions.  Every entry point that takes a `resolution` (or an array of them)
 * accepts exactly the positive finite doubles -- subnormal and huge finite values
 * included: the field then underflows to signed zeros or overflows to +/-inf as
 * float(sqrt((double)D) * resolution) does.  NaN, 0, negative and infinite values
 * are refused with SDFGPU_ERR_INVALID_ARGUMENT before anything is enqueued or
 * written; sdfgpu_last_error names the value.  (sdfgpu_extrema_from_dsq has no
 * handle: it returns the code and leaves its outputs untouched.)
 * ------------------------------------------------------------------------- */

/* ---------------------------------------------------------------------------
 * Whole-path entry points, host buffers.
 * Replaces sdf_generation::ExtractSignedDistanceField (sdf_generation.hpp:273-420)
 * once the caller has evaluated its predicate into `filled` (nonzero = filled),
 * in the reference's x->y->z order (:221-239).
 *   out_sdf : N floats, same layout.  sdf = filled ? -res*sqrt(D_free) : +res*sqrt(D_filled),
 *             computed as float(double) exactly like :254-265; +/-inf when a class is empty.
 *   out_max/out_min : extrema of the un-narrowed doubles (:246-269); with
 *             add_virtual_border the (free.max, filled.min) pair of :416-418.
 * ------------------------------------------------------------------------- */
int sdfgpu_build(sdfgpu_handle h, const uint8_t* filled,
                 int64_t nx, int64_t ny, int64_t nz,
                 double resolution, int add_virtual_border,
                 float* out_sdf, double* out_max, double* out_min);

/* Fast path for CollisionMapGrid::ExtractSignedDistanceField
 * (collision_map.hpp:680-712): `cells` is the grid's raw data
 * (GetImmutableRawData()), records of `cell_stride` bytes whose float occupancy
 * sits at `occupancy_offset`.  Classified on the device with exactly
 * occupancy > 0.5f || (unknown_is_filled && occupancy == 0.5f). */
int sdfgpu_build_cells(sdfgpu_handle h, const void* cells,
                       size_t cell_stride, size_t occupancy_offset, int unknown_is_filled,
                       int64_t nx, int64_t ny, int64_t nz,
                       double resolution, int add_virtual_border,
                       float* out_sdf, double* out_max, double* out_min);

/* Next-row N4: the predicates of TaggedObjectCollisionMapGrid (tagged_object_collision_map.hpp:730-856)
 * on raw TAGGED_OBJECT_COLLISION_CELL records {float occupancy; uint32 component; uint32 object_id;
 * uint32 convex_segment}.  A cell is filled iff its occupancy says so AND its object id passes:
 *   object_mode 0: any object                    (free_sdf_filled_fn :736-749)
 *   object_mode 1: object_id > 0                 (object_filled_fn :757-775, "named objects")
 *   object_mode 2: object_id in object_ids[0..n) (ExtractSignedDistanceField(objects_to_use) :817-827;
 *                                                 n == 0 means any object, like :826)
 * object_ids may hold any number of ids in any order (a sorted copy is searched on the device).
 * Classified on the device, then the same build as sdfgpu_build.
 * cells may be NULL: the records uploaded by the previous sdfgpu_build_tagged_cells call on this handle are used again
 * (same nx * ny * nz * cell_stride, no other host-buffer entry point on the handle in between; INVALID_ARGUMENT
 * otherwise).  A caller that builds one field per object (MakeObjectSDFs :875-891, one call per id) then sends the
 * 16 B/voxel records over PCIe once instead of once per object. */
int sdfgpu_build_tagged_cells(sdfgpu_handle h, const void* cells,
                              size_t cell_stride, size_t occupancy_offset, size_t object_id_offset,
                              int object_mode, const uint32_t* object_ids, int64_t n_object_ids,
                              int unknown_is_filled,
                              int64_t nx, int64_t ny, int64_t nz,
                              double resolution, int add_virtual_border,
                              float* out_sdf, double* out_max, double* out_min);

/* ---------------------------------------------------------------------------
 * Device-pointer variants (benchmark / streaming / multi-GPU callers).
 * All pointers are device pointers on the handle's GPU; `stream` is a
 * hipStream_t (NULL = default stream).  Asynchronous: kernels are enqueued on
 * `stream`, nothing is copied to the host.  Call sdfgpu_get_extrema afterwards
 * (it synchronises `stream`) to obtain (max, min) of the most recent build.
 * sdfgpu_get_extrema and sdfgpu_last_dense_certified fail with SDFGPU_ERR_HIP
 * (and a message) when the build's single stand-by launch gave up its bounded
 * in-launch wait (option "standby_single"): the field of that build is not valid.
 * ------------------------------------------------------------------------- */
int sdfgpu_build_device(sdfgpu_handle h, const uint8_t* d_filled,
                        int64_t nx, int64_t ny, int64_t nz,
                        double resolution, int add_virtual_border,
                        float* d_out_sdf, void* stream);

int sdfgpu_build_cells_device(sdfgpu_handle h, const void* d_cells,
                              size_t cell_stride, size_t occupancy_offset, int unknown_is_filled,
                              int64_t nx, int64_t ny, int64_t nz,
                              double resolution, int add_virtual_border,
                              float* d_out_sdf, void* stream);

int sdfgpu_get_extrema(sdfgpu_handle h, double* out_max, double* out_min);

/* Bits in (round 6): the occupancy as ONE BIT per voxel in linear voxel order -- bit (v & 31) of 32-bit word (v >> 5) is set
 * iff voxel v = x*ny*nz + y*nz + z is filled; ceil(nx*ny*nz / 32) words, bits beyond the last voxel ignored.  This is what the
 * predicate loop of sdf_generation.hpp:219-240 produces when a caller keeps its occupancy packed (an octree leaf mask, a
 * voxel hash), what the host-buffer entry points above upload after classifying on the host, and what
 * sdfgpu_voxelize_points_bits_device writes.  The dense tier reads the field in place (where nz = 32 * 2^k the linear field IS
 * its [x][y][nz/32] bit field: no pack kernel runs; 16-byte alignment avoids one device copy), the z sweep and the generic dense
 * kernels read it through bit loaders: no byte mask exists anywhere.  Same results, extrema and errors as sdfgpu_build_device /
 * sdfgpu_build.  d_bits / bits must be 4-byte aligned. */
int sdfgpu_build_bits_device(sdfgpu_handle h, const uint32_t* d_bits,
                             int64_t nx, int64_t ny, int64_t nz,
                             double resolution, int add_virtual_border,
                             float* d_out_sdf, void* stream);
int sdfgpu_build_bits(sdfgpu_handle h, const uint32_t* bits,
                      int64_t nx, int64_t ny, int64_t nz,
                      double resolution, int add_virtual_border,
                      float* out_sdf, double* out_max, double* out_min);

/* Pageable host memory <-> device memory at the rate of the link.  These are the copies the host-buffer entry points
 * above use; wrappers that keep their own device buffers (the multi-GPU library, a caller filling a std::vector such
 * as the reference's GetImmutableRawData() storage, sdf.hpp / voxel_grid.hpp:760) can use them too.
 *   to_host:   the destination may be memory nobody has touched yet (a fresh std::vector / numpy array): a plain
 *              hipMemcpy then takes one first-touch page fault after the other (512^3 floats: ~40 ms); here the DMA lands
 *              in pinned staging chunks of the handle and a team of host threads copies them out while the next chunk
 *              is in flight (512^3 floats: ~11 ms = the PCIe transfer).
 *   from_host: a synchronous hipMemcpy from pageable memory is staged by one host thread (~5 GB/s measured); here a
 *              team fills the pinned chunks (128 MiB: 3 ms instead of 24 - 30).
 * Both are enqueued on `stream` behind the work already there and return when the transfer is complete.  One transfer
 * at a time per handle (they share the handle's staging chunks). */
int sdfgpu_copy_to_host(sdfgpu_handle h, void* dst, const void* d_src, size_t bytes, void* stream);
int sdfgpu_copy_from_host(sdfgpu_handle h, void* d_dst, const void* src, size_t bytes, void* stream);

/* Host occupancy -> device byte mask, classified ON THE HOST while the pinned staging chunks are filled (round 5): the team
 * of host threads evaluates the predicate -- mask byte != 0 (filled != NULL), or the CollisionMapGrid predicate
 * occupancy > 0.5f || (unknown_is_filled && occupancy == 0.5f) on raw cell records (cells != NULL; reference
 * include/sdf_tools/collision_map.hpp:689-704) -- into ONE BIT per voxel, 1/8 byte per voxel crosses PCIe (16 MiB for 512^3
 * instead of 128 MiB of mask or 1 GiB of 8-byte cells), and a kernel on `stream` spreads the bits into d_mask[n] (0 / 1).
 * This is what sdfgpu_build / sdfgpu_build_cells / *_to_device do with their input (option "host_pack" = 0 restores the
 * upload-and-classify-on-device path); exported for wrappers with their own device buffers (libsdfgpu_multi's per-rank
 * slabs).  Exactly one of filled / cells is non-NULL.  Returns when the host buffer has been consumed. */
int sdfgpu_upload_classified(sdfgpu_handle h, const uint8_t* filled, const void* cells, size_t cell_stride, size_t occupancy_offset,
                             int unknown_is_filled, int64_t n_voxels, uint8_t* d_mask, void* stream);

/* ---------------------------------------------------------------------------
 * Stage-level entry points for the x-slab multi-GPU path.
 * The grid is partitioned along x (the slowest axis); a rank owns rows
 * [x0, x0+nxs).  The z and y sweeps are slab-local:
 *
 *   sdfgpu_sweep_zy_device : mask slab [nxs,ny,nz] -> signed squared in-plane
 *       distance, int32 [nxs,ny,nz]  (+D for free voxels, -D for filled,
 *       magnitude SDFGPU_DSQ_INF where the plane holds no opposite voxel).
 *
 * The caller exchanges `halo` boundary planes of that field with its x
 * neighbours (RCCL send/recv) into one contiguous buffer
 * [halo_lo + nxs + halo_hi, ny, nz] and runs
 *
 *   sdfgpu_sweep_x_device  : x sweep + signed merge over the extended buffer,
 *       writing the nxs owned rows.  `lo_truncated` / `hi_truncated` say that
 *       real grid rows exist beyond the buffer on that side.  A voxel whose
 *       search would have needed such a row raises bit 0 of *d_status (uint32,
 *       device, caller-zeroed); the caller all-reduces it and, if set, widens
 *       the halo (or gathers whole lines) and re-runs.  x_global is the grid x
 *       of the first owned row and nx_global the full grid extent (virtual
 *       border clamp needs both).  Extrema of the owned rows go to
 *       d_maxdsq[2] (uint32 device: max d^2 over free, over filled voxels;
 *       caller-zeroed; all-reduce MAX then sdfgpu_extrema_from_dsq).
 * ------------------------------------------------------------------------- */
#define SDFGPU_DSQ_INF (1 << 30)

int sdfgpu_sweep_zy_device(sdfgpu_handle h, const uint8_t* d_filled,
                           int64_t nxs, int64_t ny, int64_t nz,
                           int32_t* d_plane_dsq, void* stream);

/* Same as sdfgpu_sweep_zy_device, and reports which y sweep ran: *d_far (uint32 device word, may be NULL) is set to 1
 * when the device-side probe found the slab far-field and the envelope kernel did the y sweep (a hint that the x
 * sweep will need whole lines too), else to 0.  sdfgpu_sweep_zy_device is this call with d_far = NULL. */
int sdfgpu_sweep_zy_tiered_device(sdfgpu_handle h, const uint8_t* d_filled,
                                  int64_t nxs, int64_t ny, int64_t nz,
                                  int32_t* d_plane_dsq, uint32_t* d_far, void* stream);

/* Exact x sweep + signed merge on COMPLETE lines of a y slab: d_plane_dsq is [nx][nys][nz] (what an all-to-all
 * re-partition of the x-slab plane fields delivers), rows y_global .. y_global + nys of a grid
 * whose y extent is ny_global (the virtual border needs both).  Any distance: the marching sweep (bounded scan)
 * or the envelope kernel, chosen on the device.  d_out_sdf: [nx][nys][nz]; d_maxdsq[2] as in
 * sdfgpu_sweep_x_device. */
int sdfgpu_sweep_x_lines_device(sdfgpu_handle h, const int32_t* d_plane_dsq,
                                int64_t nx, int64_t nys, int64_t nz,
                                int64_t y_global, int64_t ny_global,
                                double resolution, int add_virtual_border,
                                float* d_out_sdf, uint32_t* d_maxdsq, void* stream);

int sdfgpu_sweep_x_device(sdfgpu_handle h, const int32_t* d_plane_dsq,
                          int64_t halo_lo, int64_t nxs, int64_t halo_hi,
                          int64_t ny, int64_t nz,
                          int lo_truncated, int hi_truncated,
                          int64_t x_global, int64_t nx_global,
                          double resolution, int add_virtual_border,
                          float* d_out_sdf, uint32_t* d_maxdsq, uint32_t* d_status,
                          void* stream);

/* Dense-scene stages (see sdf_tools_amd/csrc/sdfgpu_dense.hpp), also usable on x slabs:
 *   sdfgpu_pack_bits_device : n_rows z-rows of nz occupancy bytes -> n_rows * nz / 32 words (bit i of
 *       word w = voxel z = 32 w + i is filled); nz % 32 == 0.
 *   sdfgpu_dense_ball_device: bit planes [rows_x, ny, nz/32] -> fp32 SDF of planes [out_lo, out_hi),
 *       exact for every voxel whose nearest opposite-class voxel is within squared distance 8
 *       (needs 2 planes of context on each side, i.e. halo planes from the x neighbours in slab
 *       mode; at a true grid face the buffer simply ends).  Raises *d_uncertified (uint32, caller-
 *       zeroed) if some voxel is farther than that -- the caller must then run the general path.
 *       d_maxdsq[2] as in sdfgpu_sweep_x_device.  nz must be 32 * 2^k <= 2048. */
int sdfgpu_pack_bits_device(sdfgpu_handle h, const uint8_t* d_filled, int64_t n_rows, int64_t nz,
                            uint32_t* d_bits, void* stream);
int sdfgpu_dense_ball_device(sdfgpu_handle h, const uint32_t* d_bits, int64_t rows_x, int64_t out_lo,
                             int64_t out_hi, int64_t ny, int64_t nz, double resolution,
                             float* d_out_sdf, uint32_t* d_maxdsq, uint32_t* d_uncertified, void* stream);
/* The kernels behind sdfgpu_sweep_x_device / sdfgpu_dense_ball_device collect their maxima in a slot array
 * (see sdfgpu_kernels.hpp: slot_max2) and each call ends with a one-block fold into d_maxdsq[2].  A caller
 * that issues several such calls per build (interior + border planes of a slab) can set the option
 * "defer_fold" = 1 and fold once itself: */
int sdfgpu_fold_extrema_device(sdfgpu_handle h, uint32_t* d_maxdsq, void* stream);

/* One x slab of the dense path in three calls (the same kernels as the stage entry points above, fewer host
 * round trips per build).  d_bits_ext: [halo_lo + nxs + halo_hi][ny][nz/32] with halo_lo / halo_hi = 0 or 2 planes
 * the caller fills by exchanging boundary planes; d_small: 4 words {max d^2 free, max d^2 filled, -, uncertified}.
 *   phase 0   clear d_small, pack the boundary planes (everything if the slab has no neighbour or is too thin)
 *             -> the caller posts the halo exchange of the 2 + 2 boundary bit-planes
 *   phase 1   pack the interior, ball kernel on the planes that need no neighbour data (10 / 11: only the first /
 *             second of the two)
 *   phase 2   (after the exchange has completed) ball kernel on the border planes, fold of the maxima */
int sdfgpu_slab_dense_phase(sdfgpu_handle h, int phase, const uint8_t* d_mask_slab,
                            int64_t nxs, int64_t ny, int64_t nz,
                            uint32_t* d_bits_ext, int64_t halo_lo, int64_t halo_hi,
                            double resolution, float* d_out_sdf, uint32_t* d_small, void* stream);

/* (max, min) from the two integer maxima (0 = class absent, >= SDFGPU_DSQ_INF =
 * infinite), reproducing sdf_generation.hpp:246-269 / :416-418. */
int sdfgpu_extrema_from_dsq(uint32_t max_dsq_free, uint32_t max_dsq_filled,
                            double resolution, double* out_max, double* out_min);

/* ---------------------------------------------------------------------------
 * Next-row N1: grid-aligned gradient of a device-resident field,
 * SignedDistanceField::GetGridAlignedGradient (include/sdf_tools/sdf.hpp:432-526)
 * for every voxel at once.  d_out_grad: [nx,ny,nz,3] float64 when
 * out_is_f64 != 0 (bit-identical to the reference's doubles) else float32.
 * Interior voxels use central differences; edge voxels use the clamped
 * one-sided form when enable_edge_gradients != 0, else are written as NaN
 * (the reference returns an empty vector there).
 * ------------------------------------------------------------------------- */
int sdfgpu_gradient_device(sdfgpu_handle h, const float* d_sdf,
                           int64_t nx, int64_t ny, int64_t nz,
                           double resolution, int enable_edge_gradients,
                           void* d_out_grad, int out_is_f64, void* stream);

/* Host-buffer form (what SignedDistanceField::GetFullGradient's fast path and pysdf_tools call instead of
 * nx*ny*nz host GetGradient calls, reference sdf.hpp:341-358 / utils_3d.py:77-90): sdf = N floats,
 * out_grad = N x 3 doubles (out_is_f64) or floats; NaN where the reference returns an empty vector. */
int sdfgpu_gradient(sdfgpu_handle h, const float* sdf,
                    int64_t nx, int64_t ny, int64_t nz,
                    double resolution, int enable_edge_gradients,
                    void* out_grad, int out_is_f64);

/* Next-row N1, query side: batched SignedDistanceField::EstimateDistance4d (sdf.hpp:947-961: trilinear
 * inter/extrapolation :836-902 of the 8 surrounding cell centres, each shrunk by half a cell toward the
 * surface :773-796, neighbour pairs per axis :798-833) and GetGradient4d (:383-430) at n world-frame
 * points (d_points: n x 3 doubles).  world_to_grid: 12 host doubles, row-major 3x4 = inverse origin
 * transform (NULL = identity); grid_to_world_rotation: 9 host doubles, row-major (NULL = identity).
 * Outputs (device, any may be NULL):
 *   d_distance[n]  the estimate, or oob_value where the point is outside the grid; every product and sum is rounded on its own
 *                  (no fused multiply-add).  With world_to_grid = NULL (the identity) or a pure translation (rotation part the
 *                  identity: 1 x + 0 y + 0 z + t is x + t, one rounding) it is bit-equal to the host's EstimateDistance4d; the
 *                  tests pin these two cases.  With a rotation the grid coordinates are the four-term sums w0 x + w1 y + w2 z + w3,
 *                  which the host's transform need not round the same way.  What holds there, and is tested against exact
 *                  rational arithmetic in frames whose nine rotation entries are all nonzero (u = 2^-53, S_i = |w_i0 x| + |w_i1 y|
 *                  + |w_i2 z| + |w_i3|, S the largest of the three): the cell is the exact one, floor(W (p, 1) / resolution),
 *                  unless a coordinate is within 8 u S_i / resolution (in cells) of a cell face, where either neighbour may
 *                  answer (on an outer face: the estimate or oob_value); the distance is within 64 u (1 + S / resolution)
 *                  sum |D_c| of the exact estimate at the exact grid coordinates, D_c the 8 half-cell-corrected corner values
 *   d_gradient[3n] world-frame gradient of the cell holding the point, rounded product by product and sum by sum: each component
 *                  within 4 u sum_j |R_ij| |g_j| of the exactly rotated grid-frame gradient g of that cell; NaN where the reference returns
 *                  an empty vector (outside, or boundary shell without enable_edge_gradients)
 *   d_flags[n]     bit0 = point inside the grid, bit1 = gradient available */
int sdfgpu_query_points_device(sdfgpu_handle h, const float* d_sdf,
                               int64_t nx, int64_t ny, int64_t nz, double resolution,
                               const double* world_to_grid, const double* grid_to_world_rotation,
                               float oob_value, const double* d_points, int64_t n_points,
                               int enable_edge_gradients,
                               double* d_distance, double* d_gradient, uint8_t* d_flags, void* stream);

/* Host-buffer form of the query above against a field that LIVES IN HBM (round 4; what the C++ mirror's
 * sdf_tools::DeviceSignedDistanceField::EstimateDistanceBatch / GetGradientBatch call, i.e. N1 for callers of the
 * reference's host-side SignedDistanceField::EstimateDistance* / GetGradient*, sdf.hpp:922-961, :383-430): points
 * (n x 3 doubles) and the three outputs are HOST arrays (any output may be NULL); d_sdf is a device pointer, e.g.
 * one filled by sdfgpu_build_device into memory from sdfgpu_device_malloc.  A caller that only needs answers at its
 * points never downloads the field (512 MiB at 512^3, ~10 ms of PCIe).  Synchronous.  Runs on the device's null stream behind this
 * handle's last build; a d_sdf written by ANOTHER producer on a non-blocking stream (another handle's build on a PyTorch stream, a
 * caller's kernel) must be complete before the call: synchronise that stream first. */
int sdfgpu_query_points(sdfgpu_handle h, const float* d_sdf,
                        int64_t nx, int64_t ny, int64_t nz, double resolution,
                        const double* world_to_grid, const double* grid_to_world_rotation, float oob_value,
                        const double* points, int64_t n_points, int enable_edge_gradients,
                        double* out_distance, double* out_gradient, uint8_t* out_flags);

/* Host input -> DEVICE-RESIDENT result (round 4): sdfgpu_build / sdfgpu_build_cells without the download of the field.
 * d_out_sdf is device memory for nx*ny*nz floats (sdfgpu_device_malloc); the extrema come back as in sdfgpu_build.
 * What sdf_generation::ExtractSignedDistanceFieldDevice and CollisionMapGrid::ExtractSignedDistanceFieldDevice call. */
int sdfgpu_build_to_device(sdfgpu_handle h, const uint8_t* filled,
                           int64_t nx, int64_t ny, int64_t nz, double resolution, int add_virtual_border,
                           float* d_out_sdf, double* out_max, double* out_min);
int sdfgpu_build_cells_to_device(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset,
                                 int unknown_is_filled, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                 int add_virtual_border, float* d_out_sdf, double* out_max, double* out_min);

/* Device memory for callers without a HIP runtime of their own (the C++ mirror is plain host C++): memory on the
 * handle's device, usable with every *_device entry point and with sdfgpu_copy_to_host / sdfgpu_copy_from_host. */
int sdfgpu_device_malloc(sdfgpu_handle h, size_t bytes, void** out_ptr);
int sdfgpu_device_free(sdfgpu_handle h, void* ptr);

/* CollisionMapGrid predicate (collision_map.hpp:689-704) on raw cell records -> byte mask (1 = filled), for callers
 * of the slab stages, which take masks: occupancy > 0.5f || (unknown_is_filled && occupancy == 0.5f). */
int sdfgpu_classify_cells_device(sdfgpu_handle h, const void* d_cells, size_t cell_stride, size_t occupancy_offset,
                                 int unknown_is_filled, int64_t n_cells, uint8_t* d_mask, void* stream);

/* Next-row N2: point cloud -> occupancy grid, the convention of scripts/3d_sdf_demo_rviz.py:22-29:
 * index = trunc((p - origin) / resolution) per axis (fp64 arithmetic on fp32 points), mask[ix][iy][iz] = 1
 * with explicit x, y, z axis order; points outside the grid are dropped.  d_points: n_points x 3 floats
 * (x, y, z interleaved).  clear_first != 0 zeroes the mask before scattering.  Feeds
 * sdfgpu_build_device without leaving the GPU (the streaming configuration). */
int sdfgpu_voxelize_points_device(sdfgpu_handle h, const float* d_points, int64_t n_points,
                                  const double* origin, double resolution,
                                  int64_t nx, int64_t ny, int64_t nz,
                                  uint8_t* d_mask, int clear_first, void* stream);

/* The same scatter into the bit field of sdfgpu_build_bits_device (one atomic OR per point; clear_first zeroes
 * ceil(nx*ny*nz / 32) words): a streaming frame goes point cloud -> bits -> SDF without a byte mask in between. */
int sdfgpu_voxelize_points_bits_device(sdfgpu_handle h, const float* d_points, int64_t n_points,
                                       const double* origin, double resolution,
                                       int64_t nx, int64_t ny, int64_t nz,
                                       uint32_t* d_bits, int clear_first, void* stream);

/* ---------------------------------------------------------------------------
 * Connected components of a two-class grid: CollisionMapGrid::UpdateConnectedComponents
 * (reference src/sdf_tools/collision_map.cpp:564-618, topology_computation.hpp:25-150) on the GPU.
 *   - a voxel is filled iff its bit is set (the bit field of sdfgpu_build_bits_device), its mask byte is nonzero, or its
 *     cell's occupancy > 0.5f -- unknown (0.5) and NaN voxels are free; there is no unknown_is_filled here
 *   - two voxels are in one component iff a path of face neighbours (6-connectivity) of their class joins them
 *   - components are numbered 1 .. K in the order the reference's x -> y -> z scan meets them, i.e. by each component's
 *     minimum linear index; the labels are therefore fully determined (bit-equal to the reference's) and every voxel gets
 *     one >= 1.  K goes to *out_count.
 *   - a grid of more than 2^32 - 1 voxels is refused (SDFGPU_ERR_INVALID_ARGUMENT): labels are uint32
 * All three are synchronous: they return when the labels are written (the device form synchronises `stream` to read K).
 * They use scratch of their own: the handle's SDF scratch, status block and learnt policy are left as they were.
 *
 *   sdfgpu_components_bits_device: d_bits (ceil(n / 32) words, 4-byte aligned) -> d_labels (n uint32, [nx][ny][nz]); a streaming
 *       frame goes point cloud -> bits -> labels with sdfgpu_voxelize_points_bits_device in front.
 *   sdfgpu_components: host mask (n bytes) -> host labels (n uint32).
 *   sdfgpu_components_cells: raw cell records of `cell_stride` bytes (COLLISION_CELL: 8, 0, 4; TAGGED_OBJECT_COLLISION_CELL:
 *       16, 0, 4), classified on the host into 1 bit per voxel while the pinned staging chunks fill; the labels come back
 *       through the staging chunks and are written IN PLACE into each record's uint32 at component_offset.
 * ------------------------------------------------------------------------- */
int sdfgpu_components_bits_device(sdfgpu_handle h, const uint32_t* d_bits, int64_t nx, int64_t ny, int64_t nz,
                                  uint32_t* d_labels, uint32_t* out_count, void* stream);
int sdfgpu_components(sdfgpu_handle h, const uint8_t* filled, int64_t nx, int64_t ny, int64_t nz,
                      uint32_t* out_labels, uint32_t* out_count);
int sdfgpu_components_cells(sdfgpu_handle h, void* cells, size_t cell_stride, size_t occupancy_offset, size_t component_offset,
                            int64_t nx, int64_t ny, int64_t nz, uint32_t* out_count);

/* Component statistics: size, coordinate sums and bounding box of every component of the set class.
 * Takes any bit field and the labels sdfgpu_components_bits_device made from it, and summarises every label in 1 .. label_count
 * that has a voxel whose bit is set, over those voxels: one sdfgpu_component_stats record per such label, in ascending label
 * order.  sum holds the sums of the voxels' x, y and z, lo and hi the bounding box (inclusive).  Everything is integer
 * arithmetic: the atomics that gather it cannot make the result depend on their order.  A voxel whose label is 0 or above
 * label_count is left out.  capacity is in records; the total always goes to out_total (required), and a list whose capacity is
 * too small is not written, which is not an error.  The call synchronises `stream` once, to read the total.  Its scratch (one
 * record per label in 0 .. label_count) is the handle's own for this call: the SDF scratch, status block and learnt policy are
 * left as they were; an allocation that fails is an SDFGPU_ERR_* as elsewhere, with nothing written.  Refused with
 * SDFGPU_ERR_INVALID_ARGUMENT: null d_bits, d_labels or out_total, buffers off their alignment (bits and labels 4, records 8
 * bytes), a negative capacity or one without a buffer, a grid of more than 2^32 - 1 voxels or with an axis above 2^31 - 1 (lo and
 * hi are int32). */
typedef struct sdfgpu_component_stats {   /* 64 bytes */
    uint32_t label;
    uint32_t reserved;           /* 0 */
    int64_t count;               /* voxels of the label whose bit is set */
    uint64_t sum[3];             /* sums of their x, y and z */
    int32_t lo[3];               /* bounding box, inclusive */
    int32_t hi[3];
} sdfgpu_component_stats;

int sdfgpu_component_stats_device(sdfgpu_handle h, const uint32_t* d_bits, const uint32_t* d_labels, int64_t nx, int64_t ny, int64_t nz,
                                  uint32_t label_count, sdfgpu_component_stats* d_stats, int64_t capacity, int64_t* out_total,
                                  void* stream);

/* ---------------------------------------------------------------------------
 * Component topology: CollisionMapGrid / TaggedObjectCollisionMapGrid::ComputeComponentTopology (reference
 * src/sdf_tools/collision_map.cpp:620-671, tagged_object_collision_map.cpp:424-490, topology_computation.hpp:297-672) on the GPU.
 * Indices: voxel (x, y, z) is (x ny + y) nz + z.  Vertex (i, j, k), 0 <= i <= nx, 0 <= j <= ny, 0 <= k <= nz, is the corner of
 * the eight voxels (i-1..i, j-1..j, k-1..k), its cube.  An out-of-grid voxel is component -1.
 * Inputs: one uint32 label per voxel (normally sdfgpu_components' output) and optionally a selection, one bit per voxel in the
 * library's bit-field layout (ignore_empty_components = occupancy > 0.5; the tagged COMPONENT_TYPES mask).
 *   - (v, c) is a SURFACE VERTEX of c iff v's cube holds a selected voxel s of label c and a face neighbour of s inside the
 *     cube has another label.  With no selection (or each label wholly selected or wholly unselected) this is: the cube holds
 *     c and something else.
 *   - its edge mask has the reference's 6 bits (z-, z+, y-, y+, x-, x+); an edge is exposed iff the 4 voxels around it hold c
 *     and something else; e = number of exposed edges; M3 / M5 / M6 = surface vertices of c with e = 3 / 5 / 6
 *   - surfaces_c = connected components of c's surface vertices joined by exposed edges (each ends in a surface vertex of c)
 *   - per component (int32, C truncation): raw = 1 + (M5 + 2 M6 - M3) / 8, voids = surfaces - 1, holes = raw + voids; the
 *     map holds exactly the components with at least one surface vertex (with sdfgpu_components labels: every selected one)
 * out_counts: (max_label + 1) x 5 int64, row c = surface vertices, M3, M5, M6, surfaces of label c (rows of absent labels are 0).
 * Deviations from the literal reference:
 *   1. the "+z" face neighbour is read at z + 1 (topology_computation.hpp:383-386 reads z - 1, after which the reference throws
 *      std::out_of_range on almost every grid: the vertices of an upper-z face never enter the vertex set its search reaches);
 *   2. out-of-grid voxels are component -1 everywhere (the reference's surface-voxel test alone compares against the OOB cell's
 *      component, and misses z == nz - 1 as an edge voxel, collision_map.hpp:108); these differ only when the OOB cell carries
 *      a label in use.
 * Refused (SDFGPU_ERR_INVALID_ARGUMENT, with a message): a selection under which some label has both selected and unselected
 * voxels (e.g. stale labels; even the corrected reference can throw there); a label above max_label; max_label = 2^32 - 1;
 * more than 2^32 - 1 voxels; more than 2^32 - 1 surface-vertex nodes (the union-find's node ids are 32-bit: Bernoulli noise has
 * about 2.1 - 2.3 nodes per vertex, so noise grids beyond about 1250^3 exceed it; structured scenes have orders of magnitude fewer).
 * All three are synchronous and, like the components, use scratch of their own (the SDF scratch, status block and policy
 * are left as they were).  Counts are integers: results are bit-reproducible.
 *
 *   sdfgpu_component_topology_device: d_labels (n uint32), d_select_bits (ceil(n / 32) words, NULL = every voxel), 4-byte aligned.
 *   sdfgpu_component_topology: host labels (n uint32) and host select_mask (n bytes, nonzero = selected; NULL = every voxel).
 *   sdfgpu_component_topology_cells: labels from each record's uint32 at component_offset, selection from its occupancy float
 *       by class_mask = FILLED (1, > 0.5) | EMPTY (2, < 0.5) | UNKNOWN (4, the rest, NaN included); 7 = every voxel.
 * ------------------------------------------------------------------------- */
int sdfgpu_component_topology_device(sdfgpu_handle h, const uint32_t* d_labels, const uint32_t* d_select_bits, int64_t nx, int64_t ny,
                                     int64_t nz, uint32_t max_label, int64_t* out_counts, void* stream);
int sdfgpu_component_topology(sdfgpu_handle h, const uint32_t* labels, const uint8_t* select_mask, int64_t nx, int64_t ny, int64_t nz,
                              uint32_t max_label, int64_t* out_counts);
int sdfgpu_component_topology_cells(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t component_offset,
                                    int64_t nx, int64_t ny, int64_t nz, int class_mask, uint32_t max_label, int64_t* out_counts);

/* ---------------------------------------------------------------------------
 * Component surfaces: CollisionMapGrid / TaggedObjectCollisionMapGrid::ExtractComponentSurfaces and its Filled / Unknown / Empty
 * wrappers (reference src/sdf_tools/collision_map.cpp:697-754, tagged_object_collision_map.cpp:492-550,
 * topology_computation.hpp:297-330) on the GPU.  DESIGN.md section 19.
 * Indices: voxel (x, y, z) is (x ny + y) nz + z.  An out-of-grid voxel is component -1 (as in "Component topology", deviation 2).
 * Inputs: one uint32 label per voxel (normally sdfgpu_components' output) and optionally a selection, one bit per voxel in the
 * library's bit-field layout (for cell records: the class mask FILLED 1, occupancy > 0.5; EMPTY 2, < 0.5; UNKNOWN 4, the rest,
 * NaN included).
 *   - a voxel v of label c is a SURFACE VOXEL iff at least one of its six face neighbours has a label other than c; an
 *     out-of-grid neighbour counts as different, so every voxel on a grid face is a surface voxel;
 *   - v is REPORTED iff it is selected and a surface voxel.  The neighbour comparison does not look at the selection, and no
 *     label is refused for being partly selected: each voxel stands alone.
 * Results:
 *   out_counts: max_label + 1 int64, entry c = reported voxels of label c (0 for absent labels);
 *   indices: the linear indices of all reported voxels as uint32, grouped by label in ascending label order and ascending
 *     inside each group -- the order in which the reference's x -> y -> z loop inserts them.  Group c starts at the sum of
 *     out_counts[0 .. c - 1].  *out_total = their number.  Fully determined, so results are bit-reproducible.
 *   d_surface_bits (device form, optional): ceil(n / 32) words, bit v set iff voxel v is reported.
 * A NULL index buffer asks for the counts (and the total, and the bits) only.
 * Deviations from the literal reference:
 *   1. every occupancy class is tested at (x, y, z) (collision_map.cpp:723 tests filled voxels at (x, y, y) and :743 unknown
 *      ones at (x, z, z); tagged_object_collision_map.cpp:519 and :539 do the same);
 *   2. out-of-grid voxels are component -1 everywhere (collision_map.hpp:108 compares z_index == GetNumZCells(), so the
 *      z = nz - 1 face is missed, and interior comparisons against the edge read the OOB cell's component).
 * Refused (SDFGPU_ERR_INVALID_ARGUMENT, with a message): a label above max_label; max_label = 2^32 - 1; more than 2^32 - 1
 * voxels (by shape alone, before anything is allocated); an index buffer whose capacity is below the total -- out_counts and
 * *out_total are valid then, so the caller can size the buffer and call again, and nothing is written past the capacity.
 * All three are synchronous and use scratch of their own from the library's allocator (the SDF scratch, status block and
 * policy are left as they were).
 *
 *   sdfgpu_component_surfaces_device: d_labels (n uint32), d_select_bits (ceil(n / 32) words, NULL = every voxel), d_indices
 *       (capacity uint32, NULL = counts only), d_surface_bits (NULL = not wanted): device pointers, 4-byte aligned.
 *   sdfgpu_component_surfaces: host labels (n uint32), host select_mask (n bytes, nonzero = selected; NULL = every voxel), host
 *       out_indices (capacity uint32, NULL = counts only).
 *   sdfgpu_component_surfaces_cells: labels from each record's uint32 at component_offset, selection from its occupancy float
 *       by class_mask (7 = every voxel), packed on the host like sdfgpu_component_topology_cells' selection.
 * ------------------------------------------------------------------------- */
int sdfgpu_component_surfaces_device(sdfgpu_handle h, const uint32_t* d_labels, const uint32_t* d_select_bits, int64_t nx, int64_t ny,
                                     int64_t nz, uint32_t max_label, int64_t* out_counts, uint32_t* d_indices, int64_t capacity,
                                     int64_t* out_total, uint32_t* d_surface_bits, void* stream);
int sdfgpu_component_surfaces(sdfgpu_handle h, const uint32_t* labels, const uint8_t* select_mask, int64_t nx, int64_t ny, int64_t nz,
                              uint32_t max_label, int64_t* out_counts, uint32_t* out_indices, int64_t capacity, int64_t* out_total);
int sdfgpu_component_surfaces_cells(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t component_offset,
                                    int64_t nx, int64_t ny, int64_t nz, int class_mask, uint32_t max_label, int64_t* out_counts,
                                    uint32_t* out_indices, int64_t capacity, int64_t* out_total);

/* -------------------------------------------------------------------------
 * Local extrema and convex segments: SignedDistanceField::ComputeLocalExtremaMap (reference src/sdf_tools/sdf.cpp:23-207) and
 * TaggedObjectCollisionMapGrid::UpdateConvexSegments (tagged_object_collision_map.cpp:552-654) on the GPU.  DESIGN.md section 15.
 * Indices: voxel (x, y, z) is (x ny + y) nz + z; loc(i) = (res (x + 0.5), res (y + 0.5), res (z + 0.5)) in the grid frame.
 * Local extrema of an SDF f (float [nx][ny][nz]) with cell size res and origin rotation q:
 *   - g(v) = GetGradient(v, enable_edge_gradients = true): central differences inside the grid, clamped one-sided differences on
 *     the boundary shell, rotated as q * ((0, g) * q^-1) with eigen_lite's Quaterniond arithmetic (no fused multiply-add).
 *   - next(v): w = f(v) < 0 ? -g : g; per axis +1 if w > s, -1 if w < -s, else 0, s = res * 0.06125.  next(v) == v exactly when
 *     the reference's GradientIsEffectiveFlat holds or no axis steps because of a NaN; the reference stops at v in both cases.
 *     A step out of the grid goes to the sink OFF.
 *   - the extremum e(v) of v's forward orbit: a fixed point t -> loc(t); OFF -> (+inf, +inf, +inf); a cycle C (length >= 2) ->
 *     loc(entry), entry = the first node of C on the orbit of the minimum-index voxel of C's basin (the voxels whose orbit ends
 *     in C).  That voxel's walk is the first of the basin in the reference's x -> y -> z scan and fixes the value for the whole
 *     basin: two voxels either side of a ridge whose maximum lies between them point at each other, and the one the scan
 *     enters first is the extremum of both.
 *   As indices: out_extremum[v] = t, entry, or 0xFFFFFFFF for OFF (4 B per voxel; the reference's map holds 24).
 *   q_and_qinv: (w, x, y, z) of q, then of q.inverse() as eigen_lite computes it (identity: 1 0 0 0 1 -0 -0 -0).
 * Convex segments of tagged cell records (float occupancy, uint32 object id, uint32 segment):
 *   - the SDF is ExtractSignedDistanceField(+inf, {}, unknown_is_filled = true, true) with add_virtual_border, otherwise
 *     ExtractFreeAndNamedObjectsSignedDistanceField(+inf, true) (free-space SDF outside, named-object SDF inside, 0 else);
 *   - a cell takes part iff (occupancy < 0.5f || object_id > 0) (NaN occupancy with object 0 does not) and e(cell) is not OFF;
 *   - two face neighbours that take part are joined iff their object ids are equal and
 *     sqrt(((0 + dx dx) + dy dy) + dz dz) < connected_threshold in double, d = loc(e(a)) - loc(e(b)) (correctly rounded sqrt);
 *   - segments are numbered 1..K by minimum index; every other cell gets 0.  Every record's segment word is overwritten; the
 *     other fields are not touched.  *out_count = K.
 * Refused (SDFGPU_ERR_INVALID_ARGUMENT): 2^32 - 2 voxels or more (indices share the uint32 space with the OFF sentinel 2^32 - 1
 * and the doubling markers 2^32 - 1, 2^32 - 2, 2^32 - 3: at most 2^32 - 3 voxels); res <= 0 or not finite.
 * The SDF of sdfgpu_convex_segments_cells is an ordinary tagged build on the handle; the extrema and segment stages use scratch
 * of their own (the SDF scratch, status block and policy are left as they were).  All results are bit-reproducible.
 *
 *   sdfgpu_local_extrema_device: d_sdf (n floats) -> d_extremum (n uint32), enqueued on `stream`; synchronises it once per
 *       doubling round (the host reads the count of unresolved voxels) and returns with its last three kernels pending there:
 *       read d_extremum on `stream` or after synchronising it.  Calls on one handle from different streams are ordered by the
 *       library (a call first waits, on the device, for the previous call's last kernel), as builds are.
 *   sdfgpu_local_extrema: host field in, host indices out.
 *   sdfgpu_convex_segments_cells: synchronous, in place; the records are uploaded once and the SDF, extrema and labels stay on
 *       the device until the labels are scattered into each record's uint32 at segment_offset.
 *   sdfgpu_convex_last_info: the last extrema computation on this handle: doubling rounds used, cycles (length >= 2), the
 *       longest cycle and the longest basin-minimum -> cycle walk (diagnostics, the benchmarks report them).
 * ------------------------------------------------------------------------- */
int sdfgpu_local_extrema_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                const double q_and_qinv[8], uint32_t* d_extremum, void* stream);
int sdfgpu_local_extrema(sdfgpu_handle h, const float* sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                         const double q_and_qinv[8], uint32_t* out_extremum);
int sdfgpu_convex_segments_cells(sdfgpu_handle h, void* cells, size_t cell_stride, size_t occupancy_offset, size_t object_id_offset,
                                 size_t segment_offset, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                 const double q_and_qinv[8], double connected_threshold, int add_virtual_border, uint32_t* out_count);
int sdfgpu_convex_last_info(sdfgpu_handle h, int* out_rounds, uint32_t* out_cycles, uint32_t* out_longest_cycle,
                            uint32_t* out_longest_entry);

/* -------------------------------------------------------------------------
 * Projection out of collision / into the valid volume (SignedDistanceField::ProjectOutOfCollision*,
 * ProjectOutOfCollisionToMinimumDistance*, ProjectIntoValidVolume*, ProjectIntoValidVolumeToMinimumDistance*; reference
 * include/sdf_tools/sdf.hpp:996-1190), one lane per point, all arithmetic in double without fused multiply-add.
 * For a world-frame point p, with res the cell size, W the world -> grid transform and G the grid -> world transform
 * (each 12 host doubles, row-major 3x4, the full transform including the translation; both are required):
 *   mode SDFGPU_PROJECT_OUT_OF_COLLISION:
 *     1. if floor((W p) * (1 / res)) is outside the grid on some axis, clamp each grid coordinate c of W p into [m, size - m]
 *        (m = res * 1e-4, size = cells * res, as min(size - m, max(m, c))); if any coordinate changed, p = G (clamped);
 *     2. q = W p;  margin = minimum_distance + res * stepsize_multiplier * 1e-4;  max_step = res * stepsize_multiplier;
 *     3. d = the trilinear estimate at q (sdfgpu_query_points' EstimateDistance) in the cell floor(q * (1 / res)); while
 *        d <= minimum_distance: g = the grid-aligned gradient of that cell with edge gradients on; if |g| <= res * 0.25
 *        (NaN included) the point is stuck (FLAT_GRADIENT); else q += (g / |g|) * min(max_step, margin - d) and d is
 *        re-estimated; a cell outside the grid ends the walk (LEFT_GRID);
 *     4. the result is G q -- also for a point that took no step (it comes back through both transforms).
 *   mode SDFGPU_PROJECT_INTO_VALID_VOLUME: step 1 alone, always applied, with m = minimum_distance + res * 1e-4; a point
 *     that no clamp changes comes back as the input bits.
 *   Sums are evaluated left to right ((a + b) + c) + d as eigen_lite.hpp does; |g| = sqrt(((0 + gx gx) + gy gy) + gz gz).
 * Two deviations from the reference (which has no bound and casts NaN coordinates to int64):
 *   - every walk stops after max_steps steps (status STEP_LIMIT, the location reached so far is kept); max_steps = 0 takes the
 *     library default 4 * ceil(sqrt(nx^2 + ny^2 + nz^2) / stepsize_multiplier) + 64, at most SDFGPU_PROJECT_MAX_STEPS_CEILING
 *     (sdfgpu_project_step_limit computes it, for the host walk as well);
 *   - a point with a NaN or infinite coordinate is refused (status NON_FINITE, the input is returned unchanged, 0 steps).
 * Per point: d_out_points[3i..3i+2] the world-frame result (a failed walk keeps the last location it reached), d_out_status[i]
 * one of SDFGPU_PROJECT_* below, d_out_steps[i] the steps taken.  status and steps may be NULL.  n = 0 is a no-op.
 * Refused (SDFGPU_ERR_INVALID_ARGUMENT, with a message): null field, points or out_points (n > 0); non-positive dims; cells
 * overflowing int64; resolution or stepsize_multiplier not positive and finite; max_steps < 0; an unknown mode; null W or G.
 * Cell indices are int64 throughout (fields past 2^31 cells).
 *   sdfgpu_project_points_device: device points and outputs, enqueued on `stream`.
 *   sdfgpu_project_points: host points and outputs against a field in HBM; synchronous, on the device's null stream behind this
 *       handle's last build (the threading note of sdfgpu_query_points applies: a field written by another producer on a
 *       non-blocking stream must be complete before the call).
 *   sdfgpu_project_step_limit: the step limit a call with these arguments uses (*out_limit).
 * ------------------------------------------------------------------------- */
#define SDFGPU_PROJECT_OUT_OF_COLLISION 0
#define SDFGPU_PROJECT_INTO_VALID_VOLUME 1

#define SDFGPU_PROJECT_CONVERGED 0      /* d > minimum_distance reached (or no walk asked for)                         */
#define SDFGPU_PROJECT_FLAT_GRADIENT 1  /* |g| <= res / 4 or NaN: "Encountered flat gradient - stuck"                  */
#define SDFGPU_PROJECT_NO_GRADIENT 2    /* the gradient was empty: "Failed to compute gradient - out of SDF?"          */
#define SDFGPU_PROJECT_LEFT_GRID 3      /* the walk reached a cell outside the grid: "Index out of bounds"             */
#define SDFGPU_PROJECT_STEP_LIMIT 4     /* max_steps steps taken without converging                                    */
#define SDFGPU_PROJECT_NON_FINITE 5     /* a NaN or infinite input coordinate                                          */

#define SDFGPU_PROJECT_MAX_STEPS_CEILING 1048576

int sdfgpu_project_step_limit(int64_t nx, int64_t ny, int64_t nz, double stepsize_multiplier, int max_steps, int* out_limit);
int sdfgpu_project_points_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                 const double world_to_grid[12], const double grid_to_world[12], double minimum_distance,
                                 double stepsize_multiplier, int max_steps, int mode, const double* d_points, int64_t n_points,
                                 double* d_out_points, uint8_t* d_out_status, int32_t* d_out_steps, void* stream);
int sdfgpu_project_points(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                          const double world_to_grid[12], const double grid_to_world[12], double minimum_distance,
                          double stepsize_multiplier, int max_steps, int mode, const double* points, int64_t n_points,
                          double* out_points, uint8_t* out_status, int32_t* out_steps);

/* -------------------------------------------------------------------------
 * Interpolated gradients (SignedDistanceField::GetSmoothGradient*, GetAutoDiffGradient*, DistanceToBoundary*; reference
 * include/sdf_tools/sdf.hpp:528-653, 963-988), one lane per point, all arithmetic in double without fused multiply-add, bit-equal
 * to the host core SignedDistanceField::QueryGradient4d (include/sdf_tools/sdf.hpp, whose comment states the arithmetic).
 * For a world-frame point p, with res the cell size and W the world -> grid transform (12 host doubles, row-major 3x4):
 *   kind SDFGPU_QUERY_AUTODIFF_GRADIENT: the exact derivative of the trilinear estimate (sdfgpu_query_points' distance) with
 *     respect to p, by forward-mode dual numbers through W and the estimate; value = that estimate, bit for bit.
 *   kind SDFGPU_QUERY_SMOOTH_GRADIENT: central differences of the estimate over p -+ |window| along each world axis, one-sided
 *     where one end's cell is outside the grid; value = the estimate at p.  window = 0 gives a NaN (0 / 0) gradient.
 *   kind SDFGPU_QUERY_DISTANCE_TO_BOUNDARY: (a, b, c) = W p; per axis min(a, size - a) (size = cells * res); value = the one
 *     with the first least magnitude; status OK when all three are >= 0.  The gradient is not computed (NaN).  Non-finite points
 *     are not refused for this kind: they give what that arithmetic gives.
 * Per point: d_value[i], d_gradient[3i..3i+2] (world frame; NaN where the reference returns an empty vector or throws),
 * d_status[i] one of SDFGPU_QUERY_* below.  Any output may be NULL.  n = 0 is a no-op.  A point or window end is inside the grid
 * when floor(q * (1 / res)) is, decided on the doubles.  Outside (status OUTSIDE), value = oob_value for the two gradient kinds.
 * A NaN or infinite coordinate (smooth, autodiff): status NON_FINITE, value NaN -- a deviation, the reference casts NaN to int64.
 * Refused (SDFGPU_ERR_INVALID_ARGUMENT, with a message): null field, or null points with n > 0; non-positive dims; cells
 * overflowing int64; resolution not positive and finite; a non-finite window; an unknown kind; null W.  Cell indices are int64.
 *   sdfgpu_query_gradients_device: device points and outputs, enqueued on `stream`.
 *   sdfgpu_query_gradients: host points and outputs against a field in HBM; synchronous, ordered as sdfgpu_query_points.
 * ------------------------------------------------------------------------- */
#define SDFGPU_QUERY_SMOOTH_GRADIENT 0
#define SDFGPU_QUERY_AUTODIFF_GRADIENT 1
#define SDFGPU_QUERY_DISTANCE_TO_BOUNDARY 2

#define SDFGPU_QUERY_OK 0                /* gradient computed / point inside the volume                                     */
#define SDFGPU_QUERY_OUTSIDE 1           /* reference returns an empty vector / point_inside == false                       */
#define SDFGPU_QUERY_WINDOW_TOO_LARGE 2  /* reference throws "Window size for GetSmoothGradient is too large for SDF"       */
#define SDFGPU_QUERY_NON_FINITE 3        /* NaN / inf coordinate (smooth, autodiff)                                          */

int sdfgpu_query_gradients_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                  const double world_to_grid[12], float oob_value, int kind, double window, const double* d_points,
                                  int64_t n_points, double* d_value, double* d_gradient, uint8_t* d_status, void* stream);
int sdfgpu_query_gradients(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, double resolution,
                           const double world_to_grid[12], float oob_value, int kind, double window, const double* points,
                           int64_t n_points, double* out_value, double* out_gradient, uint8_t* out_status);

/* ---------------------------------------------------------------------------
 * Batches of same-shape grids: B grids of one shape (nx, ny, nz) in one launch sequence.  Grid b lies at offset b * nx * ny * nz
 * of the input and of the output, each in the layout above (z fastest).  Every grid comes out bit-equal to its single build
 * (sdfgpu_build_device with resolutions[b], or `resolution` for every grid when resolutions == NULL) and so do its extrema.
 * What callers with many small fields use in place of a host loop over the one-grid calls: a batch of environments
 * (reference src/sdf_tools/utils_3d_tensorflow.py:6-15), one field per object id (tagged_object_collision_map.hpp:875-891).
 *   - fast path: a shape whose three axes are all <= 128 (after singleton axes are moved to the front) is built by an exact
 *     min-plus over whole lines in TWO launches for the whole batch (sdf_tools_amd/csrc/sdfgpu_batch.hip), whatever the scenes
 *     are: no tier, probe or guard is involved.  It uses scratch of its own.
 *   - any other shape: the single build is enqueued once per grid on `stream`, without a host synchronisation between grids.
 *     sdfgpu_last_batch_info reports which of the two ran (*out_fast_path 1 / 0) and the launches of the fast path
 *     (*out_launches: 2; -1 on the other path, which does not count them).
 *   - `resolutions` (host, batch entries) is read before the call returns; the caller may free it.
 *   - a batch build and a single build on one handle do not affect each other's results: sdfgpu_get_extrema keeps answering
 *     for the last SINGLE build, sdfgpu_get_extrema_batch (it waits for the batch) for the last batch build, whose batch it
 *     must be given.  Batch calls take part in the handle's ordering of builds across streams.  The debug hooks and the learnt
 *     tier policy see the single builds of the second path like any other single build.
 * INVALID_ARGUMENT: null pointers, batch < 1 (or > 2^24), non-positive dimensions, a resolution that is not positive and
 * finite ("Resolutions" above), a misaligned cell layout.
 *   sdfgpu_build_batch_device: device pointers, asynchronous on `stream`.
 *   sdfgpu_build_batch: host masks in, host fields and batch (max, min) pairs out (out_max / out_min may be NULL).
 *   sdfgpu_build_tagged_objects: one field per object id from ONE grid of tagged cell records: grid b is filled where the
 *       occupancy says so AND object_id == object_ids[b] (sdfgpu_build_tagged_cells' object_mode 2 with that single id).  The ids
 *       may come in any order, repeat, or be absent from the grid (such a field is all +inf).  The records are uploaded once and
 *       classified inside the batch's first kernel for every id: no per-id mask exists and no per-id classify launch runs (fast
 *       path).  cells == NULL re-uses the records of the previous tagged call, under the rule of sdfgpu_build_tagged_cells.
 *       out_sdf: n_object_ids fields.
 *   sdfgpu_gradient_batch_device: the definition of sdfgpu_gradient_device on every grid of a batch (any shape), one launch;
 *       d_out: [batch][nx,ny,nz,3] float64 (f64 != 0) or float32, bit-equal to the single call per grid.
 * ------------------------------------------------------------------------- */
int sdfgpu_build_batch_device(sdfgpu_handle h, const uint8_t* d_filled, int64_t batch,
                              int64_t nx, int64_t ny, int64_t nz,
                              double resolution, const double* resolutions,
                              int add_virtual_border, float* d_out_sdf, void* stream);
int sdfgpu_get_extrema_batch(sdfgpu_handle h, int64_t batch, double* out_max, double* out_min);
int sdfgpu_build_batch(sdfgpu_handle h, const uint8_t* filled, int64_t batch, int64_t nx, int64_t ny, int64_t nz,
                       double resolution, const double* resolutions, int add_virtual_border,
                       float* out_sdf, double* out_max, double* out_min);
int sdfgpu_build_tagged_objects(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset,
                                size_t object_id_offset, const uint32_t* object_ids, int64_t n_object_ids,
                                int unknown_is_filled, int64_t nx, int64_t ny, int64_t nz, double resolution,
                                int add_virtual_border, float* out_sdf, double* out_max, double* out_min);
int sdfgpu_gradient_batch_device(sdfgpu_handle h, const float* d_sdf, int64_t batch, int64_t nx, int64_t ny, int64_t nz,
                                 double resolution, const double* resolutions, int enable_edge_gradients, int f64,
                                 void* d_out, void* stream);
int sdfgpu_last_batch_info(sdfgpu_handle h, int* out_fast_path, int* out_launches);

/* ---------------------------------------------------------------------------
 * Resample: CollisionMapGrid / TaggedObjectCollisionMapGrid::Resample(new_resolution) (reference src/sdf_tools/collision_map.cpp:673-695,
 * tagged_object_collision_map.cpp:399-422) on the GPU.  DESIGN.md section 21.
 * The caller builds the result grid (the classes do it with VoxelGrid's metric-size constructor: the source's origin transform,
 * ceil(size / new_resolution) cells per axis) and passes both geometries; the library moves the cell records.
 * Indices: cell (x, y, z) of a grid of nx x ny x nz is record (x ny + y) nz + z; records are cell_bytes = 4, 8 or 16 bytes and are
 * copied whole (occupancy bit pattern, component, object id, convex segment: no field is interpreted).  Matrices are row-major
 * 4 x 4, as in the projection entry points (all 16 entries are used, as Isometry3d * Vector4d uses them).
 * Every source cell (x, y, z), in x -> y -> z order:
 *   loc = origin * (src_cell[0] (x + 0.5), src_cell[1] (y + 0.5), src_cell[2] (z + 0.5), 1)
 *   p   = dst_inverse_origin * loc
 *   idx = floor(p[a] * dst_inv_cell[a]) per axis a            (dst_inv_cell = 1.0 / the result's cell sizes: a product, not a division)
 *   idx inside mx x my x mz: the source record overwrites result record idx; otherwise the cell is dropped.
 * So, of the source cells that land in one result cell, the one with the LARGEST source index stays, and a result cell on which no
 * source cell lands holds fill_cell (any upsampling leaves such holes: the reference's behaviour, kept).
 * Arithmetic: double precision, each row as ((m0 v0 + m1 v1) + m2 v2) + m3 v3 with separate products and sums (no FMA): bit for bit
 * what VoxelGrid::GridIndexToLocation and LocationToGridIndex4d compute on the host.  The bounds test is made on the double
 * (v >= 0 && v < n) before it is converted, which for finite values is the host's floor-then-compare; a p that is not finite is
 * dropped.
 * *out_cells_written (optional) = result cells that received a source cell.
 * Refused (SDFGPU_ERR_INVALID_ARGUMENT, with a message, nothing written): cell_bytes not 4, 8 or 16; a dimension that is not
 * positive; a null pointer (out_cells_written excepted); src == dst; device pointers that are not 4-byte aligned.
 *
 *   sdfgpu_resample_cells_device: d_src, d_dst device pointers (4-byte aligned; wider accesses are used when both are 8- or
 *       16-byte aligned), fill_cell a host record.  A memset and two kernels on `stream`, nothing on another stream; returns with
 *       them pending, unless out_cells_written is asked for: then it synchronises `stream`.  The winner words (4 bytes per result
 *       cell, 8 when the source has 2^32 - 1 cells or more) are scratch of the handle: a call on another stream is ordered behind
 *       the last one on the device.
 *   sdfgpu_resample_cells: host src and dst, through the handle's staging buffers on the null stream; synchronous.
 * ------------------------------------------------------------------------- */
int sdfgpu_resample_cells_device(sdfgpu_handle h, const void* d_src, size_t cell_bytes, int64_t nx, int64_t ny, int64_t nz,
                                 const double src_cell[3], const double origin[16], const double dst_inverse_origin[16],
                                 const double dst_inv_cell[3], void* d_dst, int64_t mx, int64_t my, int64_t mz, const void* fill_cell,
                                 uint64_t* out_cells_written, void* stream);
int sdfgpu_resample_cells(sdfgpu_handle h, const void* src, size_t cell_bytes, int64_t nx, int64_t ny, int64_t nz, const double src_cell[3],
                          const double origin[16], const double dst_inverse_origin[16], const double dst_inv_cell[3], void* dst, int64_t mx,
                          int64_t my, int64_t mz, const void* fill_cell, uint64_t* out_cells_written);
/* After sdfgpu_set_option(h, "resample_timing", 1): the device time of the last resample call's memset + winner kernel and of its
 * gather kernel, in milliseconds, from HIP events on its stream (synchronises with them; tools/resample_bench.py). */
int sdfgpu_debug_resample_times(sdfgpu_handle h, double* out_winner_ms, double* out_gather_ms);

/* ---------------------------------------------------------------------------
 * Shape rasteriser: what the reference's SDF_Builder asks MoveIt per voxel (src/sdf_tools/sdf_builder.cpp:281-363), decided on
 * the GPU for a list of primitive shapes.  DESIGN.md section 26.
 * PREDICATE.  Voxel (x, y, z) of an nx x ny x nz grid is filled iff the closed probe cube {p : |p_a - c_a| <= voxel_size / 2 for
 * a = x, y, z} meets the closed solid of at least one shape; touching counts.  The cube's axes are the WORLD's axes, whatever the
 * rotation of `origin` (the reference's prismatic probe does the same: on a rotated origin the probes do not tile the grid), and
 *   c = origin * (voxel_size (x + 0.5), voxel_size (y + 0.5), voxel_size (z + 0.5), 1).
 * voxel_size is the grid's resolution (the classes' GetResolution(): cubic voxels); the message of a refusal calls it the resolution.
 * A shape follows shape_msgs::SolidPrimitive: `pose` is a row-major 4 x 4 mapping the shape frame to the world (its first three
 * rows are read, all 12 entries; the fourth row is not), its rotation block is taken as orthonormal, and the solid is the image
 * of the canonical solid:
 *   SDFGPU_SHAPE_BOX (1)       dims = full extents x, y, z.  The 15 separating axes of cube and oriented box; an axis separates
 *                              only when |t . L| > r_cube + r_box, so a cross axis that degenerates to 0 never does.
 *   SDFGPU_SHAPE_SPHERE (2)    dims = radius.  sum_a max(|c_a - s_a| - voxel_size / 2, 0)^2 <= radius^2.
 *   SDFGPU_SHAPE_CYLINDER (3)  dims = height, radius; the axis is the shape's z.  With q the centre in the shape frame and
 *                              h = voxel_size / 2: empty when |q_z| - height / 2 > 1.75 h or q_x^2 + q_y^2 > (radius + 1.75 h)^2;
 *                              filled when the centre is in the solid; else each of the cube's six faces, in the shape frame,
 *                              is clipped to |z| <= height / 2 (two Sutherland-Hodgman passes) and the voxel is filled iff the
 *                              least squared distance from the axis to the xy projection of a clipped face's edge is <= radius^2,
 *                              or the axis segment passes through the cube (slab test in the world's axes).
 *   SDFGPU_SHAPE_PLANE (5)     see "Planes and triangle meshes" below.
 * Every other type (a cone (4) among them) is refused; meshes have an entry point of their own below.  Arithmetic: double precision, the centre's rows as
 * ((m0 v0 + m1 v1) + m2 v2) + m3 as in Resample, separate products and sums throughout (no FMA); tests/scene_raster_restated.py
 * states every operation.  A shape reaches this test only in regions its world bounds, inflated by `voxel_size` (more than the
 * probe's circum-radius), meet; the slack is far above the rounding, so the culling changes no voxel.
 * OUTPUTS, each optional, at least one: bits (the linear bit field of sdfgpu_build_bits_device: bit v & 31 of word v >> 5 is voxel
 * v = (x ny + y) nz + z, ceil(n / 32) words, the spare bits of the last word zero), mask (uint8 0 / 1 per voxel), object_ids
 * (uint32 per voxel: the object_id of the FIRST shape in list order that meets the probe, 0 where none does; every shape's
 * object_id must then be >= 1).  Every word, byte and id is written by exactly one thread: the result does not depend on scheduling.
 * n_shapes == 0 is valid and clears the outputs; n_shapes above SDFGPU_MAX_SHAPES is refused.
 * Refused (SDFGPU_ERR_INVALID_ARGUMENT, with a message, nothing written): every output null; a dimension or a voxel_size that is
 * not positive (or not finite); an origin entry that is not finite; too many shapes; null shapes with n_shapes > 0; in the device
 * form d_shapes off 8 bytes, d_bits or d_object_ids off 4.  A shape is refused for an unknown type, a dim (of those its type
 * uses) that is negative or not finite, a pose entry (of the 12) that is not finite, or object_id 0 when ids are asked for.
 *
 *   sdfgpu_rasterize_shapes: host shapes and outputs, through the handle's staging buffers on the null stream; synchronous.  The
 *       shapes are checked on the host before anything is launched; the message names the first refused shape's index.
 *   sdfgpu_rasterize_shapes_device: device pointers; a memset and three kernels on `stream`, nothing elsewhere, no host
 *       synchronisation.  The shapes are checked on the device: when one is refused the outputs are CLEARED (all zero) and a
 *       status word holds the lowest such index.  out_bad_shape (optional): the call synchronises `stream`, stores that index
 *       (-1: none) and, if there is one, returns SDFGPU_ERR_INVALID_ARGUMENT naming it; without it the call never waits.  The
 *       scratch (one status block, 48 bytes per shape, one candidate bit per coarse region and shape; at most 4096 regions, so
 *       at most 35 MiB, sized from nx, ny, nz and n_shapes alone) belongs to the handle: a call on another stream is ordered
 *       behind the last one on the device.
 * ------------------------------------------------------------------------- */
#define SDFGPU_SHAPE_BOX 1
#define SDFGPU_SHAPE_SPHERE 2
#define SDFGPU_SHAPE_CYLINDER 3
#define SDFGPU_MAX_SHAPES 65536
typedef struct sdfgpu_shape {
    uint32_t type;
    uint32_t object_id;
    double dims[3];
    double pose[16];
} sdfgpu_shape;
int sdfgpu_rasterize_shapes_device(sdfgpu_handle h, const sdfgpu_shape* d_shapes, int64_t n_shapes, const double origin[16], double voxel_size,
                                   int64_t nx, int64_t ny, int64_t nz, uint32_t* d_bits, uint8_t* d_mask, uint32_t* d_object_ids,
                                   int64_t* out_bad_shape, void* stream);
int sdfgpu_rasterize_shapes(sdfgpu_handle h, const sdfgpu_shape* shapes, int64_t n_shapes, const double origin[16], double voxel_size,
                            int64_t nx, int64_t ny, int64_t nz, uint32_t* bits, uint8_t* mask, uint32_t* object_ids);

/* ---------------------------------------------------------------------------
 * Planes and triangle meshes of a planning scene (shape_msgs::Plane, shape_msgs::Mesh).  DESIGN.md section 27.  The probe, its
 * centre c, h = voxel_size / 2, the outputs' layout and the arithmetic (doubles, separate products and sums, no FMA) are those of
 * the shape rasteriser above; tests/mesh_raster_restated.py states every operation.  Both readings below -- a mesh is its SURFACE
 * (a triangle soup, as MoveIt hands it to FCL), a plane is infinite and has no thickness -- and that touching counts are UNVERIFIED
 * against FCL and MoveIt, which are not available to this project.
 *
 *   SDFGPU_SHAPE_PLANE (5), a member of the shape list above: the plane through the shape frame's origin T with normal
 *       n = dims[0 .. 2] in the shape frame (any sign; refused when a component is not finite or all three are zero).
 *       N_a = (r_a0 n_0 + r_a1 n_1) + r_a2 n_2, s = (N_0 (c_0 - T_0) + N_1 (c_1 - T_1)) + N_2 (c_2 - T_2); the voxel is filled iff
 *       |s| <= h ((|N_0| + |N_1|) + |N_2|).  Its world bounds are unbounded: it is a candidate in every region.
 *
 *   MESHES.  struct sdfgpu_mesh names a run of triangles and a run of vertices of two shared arrays: vertices are double[3] in the
 *       mesh frame, triangles uint32[3] indices RELATIVE to the mesh's first_vertex; `pose` is row-major, mesh frame to world,
 *       12 entries read.  A voxel is filled iff the closed probe cube meets at least one closed triangle; a probe wholly inside a
 *       closed mesh is NOT filled.  Per triangle: W_i = pose * v_i (rows as ((m0 v0 + m1 v1) + m2 v2) + m3), edges f_0 = W_1 - W_0,
 *       f_1 = W_2 - W_1, f_2 = W_0 - W_2, n = f_0 x f_1, u_i = W_i - c.  Thirteen axes in this order: e_x, e_y, e_z; n; e_a x f_j
 *       for a = x, y, z and j = 0, 1, 2.  For an axis a: p_i = a . u_i, r = h (|a_x| + |a_y| + |a_z|); it separates iff
 *       min p > r or max p < -r (both strict), so an axis that degenerates to 0 never separates and a triangle of no area (a
 *       segment, a point) is still decided exactly.  Filled iff no axis separates.  A triangle reaches this test only in voxels of
 *       an index box around it inflated by far more than the probe's circum-radius: culling, which changes no voxel.
 *       The sum of the meshes' n_triangles may not exceed the triangle array's n_triangles (runs may be shared or given in any
 *       order within that).
 *   OUTPUTS as above (bits, mask, object_ids; each optional, at least one).  accumulate == 0: cleared, then written.
 *       accumulate == 1: bits and mask are OR-ed onto what is there (sdfgpu_rasterize_shapes' output, say).  An id is the SMALLEST
 *       object_id among the meshes that meet the probe and, under accumulate, the non-zero id already there; 0 where there is none.
 *       The rule is commutative: the result depends neither on scheduling nor on the order of triangles or meshes.  It DIFFERS
 *       from the shape list's "first in list order"; the two coincide when ids ascend with list order (SDF_Builder's do).
 *   Refused with a message, nothing written (under accumulate: nothing changed): a null or misaligned pointer (meshes and vertices
 *       off 8 bytes; triangles, bits, ids off 4), a count that is negative or above SDFGPU_MAX_MESHES / SDFGPU_MAX_TRIANGLES (or
 *       n_vertices above 2^32), no output, the grid and voxel_size refusals of the shape rasteriser, a value of accumulate other
 *       than 0 and 1.  Per mesh: a triangle or vertex run outside the arrays, triangle counts that sum past n_triangles, a pose
 *       entry or a referenced vertex that is not finite, a vertex index >= the mesh's n_vertices, object_id 0 or 0xFFFFFFFF when
 *       ids are asked for.
 *
 *   sdfgpu_rasterize_meshes: host arrays and outputs on the null stream, synchronous; always clears; everything is checked on the
 *       host first and the message names the first refused mesh.
 *   sdfgpu_rasterize_meshes_device: device pointers; memsets and five kernels (k_mr_meshes, k_mr_setup, k_mr_scan_blocks,
 *       k_mr_scan_top, k_mr_scatter) on `stream`, no host synchronisation.  The meshes are checked on the device: the lowest refused
 *       mesh index goes to a status word that the scatter kernel reads before it writes anything, so a refused call leaves cleared
 *       outputs (accumulate == 0) or untouched ones (accumulate == 1).  out_bad_mesh behaves as out_bad_shape does.  The scratch
 *       (a status block, 8 bytes per mesh, 84 bytes per triangle and 8 per 1024 triangles; sized from n_meshes and n_triangles
 *       alone, 1.4 GiB at the limit) belongs to the handle; a call on another stream is ordered behind the last one on the device.
 * ------------------------------------------------------------------------- */
#define SDFGPU_SHAPE_PLANE 5
#define SDFGPU_MAX_MESHES 65536
#define SDFGPU_MAX_TRIANGLES 16777216
typedef struct sdfgpu_mesh {
    uint32_t object_id;
    uint32_t reserved;
    int64_t first_triangle, n_triangles;
    int64_t first_vertex, n_vertices;
    double pose[16];
} sdfgpu_mesh;
int sdfgpu_rasterize_meshes_device(sdfgpu_handle h, const sdfgpu_mesh* d_meshes, int64_t n_meshes, const double* d_vertices, int64_t n_vertices,
                                   const uint32_t* d_triangles, int64_t n_triangles, const double origin[16], double voxel_size, int64_t nx,
                                   int64_t ny, int64_t nz, uint32_t* d_bits, uint8_t* d_mask, uint32_t* d_object_ids, int accumulate,
                                   int64_t* out_bad_mesh, void* stream);
int sdfgpu_rasterize_meshes(sdfgpu_handle h, const sdfgpu_mesh* meshes, int64_t n_meshes, const double* vertices, int64_t n_vertices,
                            const uint32_t* triangles, int64_t n_triangles, const double origin[16], double voxel_size, int64_t nx, int64_t ny,
                            int64_t nz, uint32_t* bits, uint8_t* mask, uint32_t* object_ids);

/* ---------------------------------------------------------------------------
 * Solid meshes: a closed triangle mesh filled inside.  DESIGN.md section 28; sdf_tools_amd/csrc/sdfgpu_mesh_solid.hpp is the text
 * the kernels compile and tests/mesh_solid_restated.py states every operation.  Same arguments, outputs, id and accumulate rules
 * and refusals as the mesh calls above; EVERY mesh of the call is solid.  A voxel is filled by a mesh iff
 *   (a) its probe cube meets one of the mesh's triangles -- the thirteen-axis test above, unchanged -- or
 *   (b) its centre is inside the mesh by the even-odd rule: the line t -> origin * (res (x + 1/2), res (y + 1/2), t, 1) crosses an
 *       odd number of that mesh's triangles on one side of the centre.
 * Parity is counted PER MESH: two overlapping solid meshes give their union, one mesh made of a cube inside a cube a hollow wall.
 * Triangle orientation plays no part.  The call does not ask whether a mesh is closed: an open mesh gives the parity as defined
 * below, which is deterministic (independent of scheduling and of triangle and mesh order) but means nothing.
 *
 *   (b) in full, in the grid frame.  inverse = the inverse of the origin's 3 x 3 block by cofactors, computed on the host (an
 *       origin without one is refused for these calls); G_i = inverse (W_i - t), rows as (i0 d0 + i1 d1) + i2 d2 with
 *       d = W_i - t, is a triangle's vertex in grid coordinates.  A mesh with a G that is not finite is refused.
 *       C = (res (x + 1/2), res (y + 1/2)) is the centre of column (x, y).
 *       XY COVERAGE.  orient(P, Q, C) = (P_x - C_x)(Q_y - C_y) - (P_y - C_y)(Q_x - C_x).  For the edges (G_1, G_2), (G_2, G_0),
 *       (G_0, G_1): s_j is the EXACT sign of orient over the doubles P, Q, C as they stand (a floating filter -- the value in
 *       doubles is trusted when it exceeds 2^-50 (|l| + |r|) of its two products, both finite and their sum at least 2^-900 -- then
 *       six two-products, by fma, summed into a non-overlapping expansion; exact while every non-zero input is at least 2^-980 of
 *       the largest).  An edge is evaluated from its endpoints in lexicographic (x, then y) order and negated when that swaps
 *       them.  A zero is resolved by the top-left rule: as if C were displaced by (eps, eps^2), that is by the sign of P_y - Q_y,
 *       then of Q_x - P_x; 0 only for P = Q in projection.  The triangle covers the column iff s_0 = s_1 = s_2 != 0; a triangle
 *       of projected area exactly 0 covers nothing.  With exact signs a combinatorially closed mesh covers every column an even
 *       number of times, ties included.  That guarantee is CONDITIONAL on the range above: a mesh with a non-zero grid coordinate
 *       below 2^-980 of the largest coordinate or column centre it is compared with (1e-300 beside centres of order 1, say) is
 *       accepted, the signs of its determinants that the filter does not decide may then be wrong, and a column of it may be
 *       covered an odd number of times.  The result is still deterministic and the same in the device form, the host form and
 *       the host-compiled text.
 *       Z OF THE CROSSING.  w_j = the edge values in doubles; z_c = ((w_0 z_0 + w_1 z_1) + w_2 z_2) / ((w_0 + w_1) + w_2), clamped to
 *       [min z_i, max z_i] (a NaN gives the minimum).  The crossing toggles the first cell k of the column with
 *       res (k + 1/2) > z_c: cell 0 when it lies below the grid, none when no centre is above it.  Cell k is inside iff an odd
 *       number of toggles lies at cells <= k.  A toggle that rounding misplaces moves only cells whose probes meet the triangle,
 *       which (a) fills anyway (section 28).
 *
 *   sdfgpu_rasterize_solid_meshes_device: device pointers, no host synchronisation: the surface call's memsets and kernels, a second
 *       per-triangle count (16 x 16 column tiles of the xy index box; k_ms_setup, which also reduces each mesh's column box) and its
 *       scan, then PER MESH one k_ms_scatter (one lane per column; a crossing is one atomic XOR of one bit) and one k_ms_merge
 *       (prefix parity along z, ORed onto the outputs): 12 + 2 n_meshes launches and memsets.  n_meshes is at most
 *       SDFGPU_MAX_SOLID_MESHES = 256, which bounds a call at about 520 launches; a caller with more splits
 *       the list and accumulates, which costs the dozen shared launches again (SDF_Builder does).  Scratch: the surface call's, 8
 *       more bytes per triangle, 32 per mesh, and a toggle field of nx ny ceil(nz / 32) words that belongs to the handle and is
 *       all zero between calls; all of it sized from the arguments alone.  Refusals, the status word, out_bad_mesh and the cleared
 *       or untouched outputs are those of sdfgpu_rasterize_meshes_device.
 *   sdfgpu_rasterize_solid_meshes: host arrays, synchronous, always clears; everything is checked on the host first, closedness
 *       included, and the message names the mesh.
 *   sdfgpu_check_closed_meshes: host only, no GPU, no handle.  A mesh is closed iff every undirected edge is used by an even number
 *       of its triangles, an edge's endpoints being keyed by their WORLD positions W (bit patterns, -0 as 0): a mesh whose
 *       triangles repeat their vertices ("STL soup") is closed, one with a T-junction is not.  An edge from a position to itself
 *       is no edge, so zero-area triangles do not open a mesh.  Sorts the edges: O(n log n).  Returns SDFGPU_OK when every mesh is
 *       closed.  Otherwise SDFGPU_ERR_INVALID_ARGUMENT, with *out_bad_mesh the first mesh that is open or would be refused and
 *       *out_bad_triangle the lowest of its triangles (relative to its first_triangle) with an edge used an odd number of
 *       times or with a refused vertex; -1 for a refused mesh record, both -1 for refused arguments.  Either may be null.
 * ------------------------------------------------------------------------- */
#define SDFGPU_MAX_SOLID_MESHES 256
int sdfgpu_rasterize_solid_meshes_device(sdfgpu_handle h, const sdfgpu_mesh* d_meshes, int64_t n_meshes, const double* d_vertices, int64_t n_vertices,
                                         const uint32_t* d_triangles, int64_t n_triangles, const double origin[16], double voxel_size, int64_t nx,
                                         int64_t ny, int64_t nz, uint32_t* d_bits, uint8_t* d_mask, uint32_t* d_object_ids, int accumulate,
                                         int64_t* out_bad_mesh, void* stream);
int sdfgpu_rasterize_solid_meshes(sdfgpu_handle h, const sdfgpu_mesh* meshes, int64_t n_meshes, const double* vertices, int64_t n_vertices,
                                  const uint32_t* triangles, int64_t n_triangles, const double origin[16], double voxel_size, int64_t nx, int64_t ny,
                                  int64_t nz, uint32_t* bits, uint8_t* mask, uint32_t* object_ids);
int sdfgpu_check_closed_meshes(const sdfgpu_mesh* meshes, int64_t n_meshes, const double* vertices, int64_t n_vertices, const uint32_t* triangles,
                               int64_t n_triangles, int64_t* out_bad_mesh, int64_t* out_bad_triangle);

/* ---------------------------------------------------------------------------
 * Display export: the device side of the reference's ExportForDisplay family (CollisionMapGrid, TaggedObjectCollisionMapGrid,
 * SignedDistanceField): which voxels are drawn, in which order, where they are and in which colour.  DESIGN.md section 23.
 * Indices: voxel (x, y, z) is (x ny + y) nz + z, a uint32; a grid of more than 2^32 - 1 voxels is refused by its shape before
 * anything is allocated.  Scan order is ascending index, the order of the reference's x -> y -> z loops.
 *
 * SELECT.  A rule yields "drawn?" and a uint32 key per voxel.
 *   SDFGPU_DISPLAY_OCCUPANCY: the class of the occupancy float by the reference's literal comparisons -- F occ > 0.5, E occ < 0.5,
 *     U occ == 0.5, N (NaN) none of them.  key = 0 for F, 1 for E, 2 for U and N (NaN falls into the reference's `else`).  Drawn iff
 *     bit `key` of class_mask (FILLED 1, EMPTY 2, UNKNOWN 4; 0 .. 7) is set and, with surface_only, some in-bounds cell o of the 26
 *     around it makes one of these true: cell E and o in {F, U}; cell F and o in {E, U}; cell U and o in {F, E, N}.  An N cell is
 *     never a surface.  Cells outside the grid do not exist.  key_offset is not used.
 *   SDFGPU_DISPLAY_KEY_FIELD: key = the uint32 at key_offset (component, object_id, convex_segment).  Drawn iff (draw_keys is NULL or
 *     holds the key) and (draw_zero or key != 0) and bit `class of the occupancy` of class_mask is set (7 = every cell; the
 *     occupancy is then not read).  draw_keys is a HOST array of n_draw_keys ascending keys in both forms (non-NULL with
 *     n_draw_keys = 0 draws nothing); surface_only is not used.
 *   sdfgpu_display_select_sdf*: drawn iff d <= 0.0f (NaN is not); key 0.
 * RESULT.  *out_total = the number of drawn voxels, always.  indices = NULL asks for that alone.  Otherwise
 *   grouped = 0: indices[0 .. total) ascending; keys[i] beside them when keys != NULL;
 *   grouped = 1: the same pairs ordered by (key, index), stably; *out_groups = the number of distinct keys G, group_keys[g]
 *     ascending, group g = elements [group_offsets[g], group_offsets[g + 1]), group_offsets[G] = total.  The group arrays are
 *     written on the device; group_offsets holds group_capacity + 1 words.  Only the key bits in which the drawn keys differ
 *     are sorted (eight a pass, from a device reduction of the smallest and largest key); with none it is the plain compaction.
 *   capacity < total, or group_capacity < G: SDFGPU_ERR_INVALID_ARGUMENT; *out_total (and *out_groups) are valid, so the caller
 *     can size the buffers and call again, and nothing is written past either capacity (with a short index buffer nothing
 *     is written at all).
 * EXPAND (sdfgpu_display_expand_device).  Per element e of d_indices[0 .. count): d_points[3 e ..] = cell_sizes[a] * ((double)i_a +
 *   0.5) for the three axis indices of the voxel (one rounding: VoxelGrid::GridIndexToLocationGridFrame bit for bit); d_colors[4 e ..]
 *   = d_color_table[4 key ..] when key = d_keys[e] (0 with d_keys = NULL) is below table_entries, else default_color.  Either of
 *   d_points / d_colors may be NULL.  Returns with its kernel pending on `stream`; uses no scratch.  The indices are TRUSTED: nx, ny, nz
 *   only decompose them, and an index at or past nx ny nz yields a point outside the grid without a word from the call (nothing is
 *   read or written out of bounds: every access is by element number).
 * SDF COLOUR MAP (SignedDistanceField::ExportForDisplay).  max_distance and min_distance are doubles that start at 0.0 and move
 *   on d > max / d < min (NaN moves neither).  Per voxel one rgba: a = min(max(alpha, 0), 1); d > 0: g = float(fabs((double)d / max)
 *   * 0.8 + 0.2); d < 0: r likewise with min; else (0, NaN) b = 1; the other channels 0.  Double arithmetic, the product and the sum
 *   rounded separately.  A NaN alpha is refused.
 * All select and colour-map calls are synchronous (they read status words back and their scratch belongs to the handle: scratch
 * of their own from the library's allocator; the SDF scratch, status block and policy are left as they were).  Device pointers
 * need 4-byte alignment only (d_points included).  The host forms stage records / fields through the handle's staging buffers on
 * the null stream.
 * ------------------------------------------------------------------------- */
#define SDFGPU_DISPLAY_OCCUPANCY 0
#define SDFGPU_DISPLAY_KEY_FIELD 1
#define SDFGPU_DISPLAY_FILLED 1
#define SDFGPU_DISPLAY_EMPTY 2
#define SDFGPU_DISPLAY_UNKNOWN 4
int sdfgpu_display_select_cells_device(sdfgpu_handle h, const void* d_cells, size_t cell_stride, size_t occupancy_offset, size_t key_offset,
                                       int64_t nx, int64_t ny, int64_t nz, int rule, int class_mask, int surface_only,
                                       const uint32_t* draw_keys, int64_t n_draw_keys, int draw_zero, int grouped, uint32_t* d_indices,
                                       uint32_t* d_keys, int64_t capacity, int64_t* out_total, uint32_t* d_group_keys,
                                       uint32_t* d_group_offsets, int64_t group_capacity, int64_t* out_groups, void* stream);
int sdfgpu_display_select_cells(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t key_offset, int64_t nx,
                                int64_t ny, int64_t nz, int rule, int class_mask, int surface_only, const uint32_t* draw_keys,
                                int64_t n_draw_keys, int draw_zero, int grouped, uint32_t* out_indices, uint32_t* out_keys, int64_t capacity,
                                int64_t* out_total, uint32_t* out_group_keys, uint32_t* out_group_offsets, int64_t group_capacity,
                                int64_t* out_groups);
int sdfgpu_display_select_sdf_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, uint32_t* d_indices,
                                     int64_t capacity, int64_t* out_total, void* stream);
int sdfgpu_display_select_sdf(sdfgpu_handle h, const float* sdf, int64_t nx, int64_t ny, int64_t nz, uint32_t* out_indices, int64_t capacity,
                              int64_t* out_total);
int sdfgpu_display_expand_device(sdfgpu_handle h, const uint32_t* d_indices, const uint32_t* d_keys, int64_t count, int64_t nx, int64_t ny,
                                 int64_t nz, const double cell_sizes[3], double* d_points, float* d_colors, const float* d_color_table,
                                 int64_t table_entries, const float default_color[4], void* stream);
int sdfgpu_display_sdf_colors_device(sdfgpu_handle h, const float* d_sdf, int64_t nx, int64_t ny, int64_t nz, float alpha, float* d_colors,
                                     void* stream);
int sdfgpu_display_sdf_colors(sdfgpu_handle h, const float* sdf, int64_t nx, int64_t ny, int64_t nz, float alpha, float* out_colors);

/* ---------------------------------------------------------------------------
 * Display export: contours -- the device side of TaggedObjectCollisionMapGrid::ExportContourOnlyForDisplay and its kin (reference
 * tagged_object_collision_map.cpp:917-1180): the outline of every object, without a distance field.  DESIGN.md section 25.
 * The reference builds one SDF per object (unknown cells filled, no virtual border) and draws a cell iff its own object's distance
 * lies in (-1.9 resolution, 0).  That field is an exact EDT, so the test admits only cells whose squared distance D, in cells, to
 * the nearest cell that is not filled for the object is at most `reach`, a number in 0 .. 3 that depends on the resolution alone:
 *   sdfgpu_display_contour_reach(cell_size, out_reach): host only, no handle.  The largest D in {1, 2, 3} with
 *     dist < 0.0 && dist > bdy for dist = -(float)(sqrt((double)D) * cell_size) and (float)bdy = -1.9 * cell_size, else 0.  3 at every
 *     ordinary size; less only where dist underflows or overflows (2^-149: 2; 1.5 * 2^127: 1; 2^-160, 2^128: 0).  NaN, zero and
 *     negative sizes fail every comparison and give reach 0 with SDFGPU_OK; only out_reach = NULL is refused.
 * SELECT (sdfgpu_display_select_contour*).  key = the uint32 at key_offset.  A cell is filled for key k iff its key is k and its
 *   occupancy is > 0.5, or == 0.5 with unknown_is_filled (NaN never).  Drawn iff the cell is filled for its own key, and (draw_keys
 *   is NULL or holds the key) and (draw_zero or key != 0), and some in-bounds cell n of the 26 around it is not filled for that key
 *   at a squared offset |n - c|^2 <= reach: 1 tests the 6 faces, 2 adds the 12 edges, 3 the 8 corners, 0 draws nothing.  Cells
 *   outside the grid do not exist, so an object that fills the grid draws nothing.  A reach outside 0 .. 3 is refused.
 * RESULT, capacities, refusals, layout checks (key_offset 4-byte aligned and inside the record), the 2^32 - 1 voxel limit, 4-byte
 *   pointer alignment and synchronisation: those of sdfgpu_display_select_cells*, word for word; draw_keys is a HOST array of
 *   ascending keys in both forms.
 * ------------------------------------------------------------------------- */
int sdfgpu_display_contour_reach(double cell_size, int* out_reach);
int sdfgpu_display_select_contour_device(sdfgpu_handle h, const void* d_cells, size_t cell_stride, size_t occupancy_offset, size_t key_offset,
                                         int64_t nx, int64_t ny, int64_t nz, int reach, int unknown_is_filled, const uint32_t* draw_keys,
                                         int64_t n_draw_keys, int draw_zero, int grouped, uint32_t* d_indices, uint32_t* d_keys,
                                         int64_t capacity, int64_t* out_total, uint32_t* d_group_keys, uint32_t* d_group_offsets,
                                         int64_t group_capacity, int64_t* out_groups, void* stream);
int sdfgpu_display_select_contour(sdfgpu_handle h, const void* cells, size_t cell_stride, size_t occupancy_offset, size_t key_offset, int64_t nx,
                                  int64_t ny, int64_t nz, int reach, int unknown_is_filled, const uint32_t* draw_keys, int64_t n_draw_keys,
                                  int draw_zero, int grouped, uint32_t* out_indices, uint32_t* out_keys, int64_t capacity, int64_t* out_total,
                                  uint32_t* out_group_keys, uint32_t* out_group_offsets, int64_t group_capacity, int64_t* out_groups);

/* ---------------------------------------------------------------------------
 * Dynamic spatial hashed map: the device-resident counterpart of DynamicSpatialHashedCollisionMapGrid
 * (reference include/sdf_tools/dynamic_spatial_hashed_collision_map.hpp), a sparse map of 8-byte COLLISION_CELL records
 * that is hashed by chunk, outlives a frame and hands out dense windows as the bit field of sdfgpu_build_bits_device.
 * DESIGN.md section 29 holds the contract (UNVERIFIED against arc_utilities' DynamicSpatialHashedVoxelGrid, which this
 * project has never seen) and the kernels.  In short:
 *   - location -> cell: g = inverse_origin * p in double (row a: ((m_a0 x + m_a1 y) + m_a2 z) + m_a3, no FMA), global cell
 *     i_a = floor(g_a * (1 / cell_size)), chunk c_a = floor_div(i_a, n_a), local l_a = i_a - c_a n_a, cell slot
 *     (l_x n_y + l_y) n_z + l_z
 *   - a location is valid iff it is finite and every c_a lies in [-2^20, 2^20)
 *   - a chunk is absent, chunk-filled (one record stands for all its cells) or cell-filled (one record per cell)
 *   - Get: (default, NOT_FOUND) for an absent chunk or an invalid location, (chunk record, FOUND_IN_CHUNK),
 *     (cell record, FOUND_IN_CELL)
 *   - SetCell: an absent chunk becomes cell-filled with every cell the default, a chunk-filled one cell-filled with every cell
 *     the chunk's record; then the cell is written (SET_CELL).  SetChunk: the chunk becomes chunk-filled with the value, its
 *     cells are dropped (SET_CHUNK).  An invalid location changes nothing (NOT_SET).  Records move byte for byte.
 *   - a batch (one kind: cell sets or chunk sets) leaves the map as if its operations had been applied one after the other in
 *     list order (the last of several writes to one cell or chunk wins); values are one record for the whole batch (one_value,
 *     host memory, 8 bytes) or one per operation (d_values / values, n records) -- exactly one of the two pointers is set
 *
 * A map is an object created on a handle; it owns its table and its chunk pool (device memory of the handle's device, inside
 * red zones when the handle has them) and must be destroyed before the handle.  It grows by itself.  byte_limit (0 = none)
 * bounds the bytes of table + pool: a batch (or a creation) that would pass it is refused with SDFGPU_ERR_UNSUPPORTED_SIZE and
 * leaves the map's content as it was.  initial_chunks (0 = 64) sizes the first pool.  Errors go to the handle's
 * sdfgpu_last_error.
 *
 * Streams: the _device forms run on the caller's stream.  The two setters, sdfgpu_dsh_insert_points_device,
 * sdfgpu_dsh_insert_rays_device and sdfgpu_dsh_fuse_rays_device synchronise that stream once (they read the number of new chunks back before the pool may grow;
 * a call that grows the table or the pool synchronises once more per growth), sdfgpu_dsh_info and the two export forms
 * synchronise too (they read counts back); sdfgpu_dsh_get_device, sdfgpu_dsh_extract_window_device and the two cast forms
 * (sdfgpu_dsh_cast_rays_device, sdfgpu_dsh_cast_segments_device) return with their kernels pending.  The removals (sdfgpu_dsh_remove_chunks_device, sdfgpu_dsh_retain_box) synchronise the stream once, to read the
 * removed count back; a call that removed something and kept something synchronises once more behind the rebuilt table (the
 * rehash's check that no key was lost).  sdfgpu_dsh_shrink synchronises before it frees what it replaced.  Calls on one map from different streams are ordered by the map (an event behind its last call); one host thread
 * per map at a time.
 * ------------------------------------------------------------------------- */
typedef struct sdfgpu_dsh_map_object* sdfgpu_dsh_map;

#define SDFGPU_DSH_NOT_FOUND 0
#define SDFGPU_DSH_FOUND_IN_CHUNK 1
#define SDFGPU_DSH_FOUND_IN_CELL 2
#define SDFGPU_DSH_NOT_SET 0
#define SDFGPU_DSH_SET_CHUNK 1
#define SDFGPU_DSH_SET_CELL 2
#define SDFGPU_DSH_MAX_CHUNK_CELLS 32768

typedef struct sdfgpu_dsh_counts {
    uint64_t chunk_filled;       /* live chunks by state */
    uint64_t cell_filled;
    uint64_t capacity_chunks;    /* chunks the pool holds before it grows */
    uint64_t table_capacity;     /* entries of the hash table (a power of two, at least twice the live chunks) */
    uint64_t bytes_held;         /* table + pool: what byte_limit bounds */
    uint64_t scratch_bytes;      /* per-batch scratch and host-form staging kept between calls (not bounded by byte_limit) */
    uint64_t byte_limit;
} sdfgpu_dsh_counts;

/* One live chunk as the export lists it (48 bytes). */
typedef struct sdfgpu_dsh_chunk {
    int64_t c[3];                /* chunk coordinate */
    uint32_t state;              /* SDFGPU_DSH_FOUND_IN_CHUNK or SDFGPU_DSH_FOUND_IN_CELL */
    uint32_t reserved;           /* 0 */
    uint64_t record;             /* the chunk's record (chunk-filled); 0 for a cell-filled chunk */
    int64_t first_cell;          /* cell-filled: where its n_x n_y n_z records start in the cell list (in records); else -1 */
} sdfgpu_dsh_chunk;

int sdfgpu_dsh_create(sdfgpu_handle h, const double inverse_origin[16], double cell_size, int64_t chunk_nx, int64_t chunk_ny,
                      int64_t chunk_nz, const void* default_cell, int64_t initial_chunks, uint64_t byte_limit, sdfgpu_dsh_map* out_map);
int sdfgpu_dsh_destroy(sdfgpu_dsh_map map);
int sdfgpu_dsh_info(sdfgpu_dsh_map map, sdfgpu_dsh_counts* out_counts);

/* Batches.  locations: n x 3 doubles (x, y, z interleaved); points: n x 3 floats as the streaming path holds them (widened to
 * double, then the same arithmetic).  d_statuses / statuses (optional): one byte per operation, SDFGPU_DSH_SET_* or
 * SDFGPU_DSH_NOT_SET; undefined when the call fails. */
int sdfgpu_dsh_set_cells_device(sdfgpu_dsh_map map, const double* d_locations, int64_t n, const void* d_values, const void* one_value,
                                uint8_t* d_statuses, void* stream);
int sdfgpu_dsh_set_cells(sdfgpu_dsh_map map, const double* locations, int64_t n, const void* values, const void* one_value,
                         uint8_t* statuses);
int sdfgpu_dsh_set_chunks_device(sdfgpu_dsh_map map, const double* d_locations, int64_t n, const void* d_values, const void* one_value,
                                 uint8_t* d_statuses, void* stream);
int sdfgpu_dsh_set_chunks(sdfgpu_dsh_map map, const double* locations, int64_t n, const void* values, const void* one_value,
                          uint8_t* statuses);
int sdfgpu_dsh_insert_points_device(sdfgpu_dsh_map map, const float* d_points, int64_t n, const void* one_value, uint8_t* d_statuses,
                                    void* stream);

/* Sensor rays: one frame of a range sensor carved into the map.  The cells between the sensor and each
 * return become free_value, then the returns become hit_value.  The contract is this project's own, UNVERIFIED against octomap's
 * insertPointCloud and against arc_utilities; tests/dsh_rays_restated.py restates it.  All of it is IEEE double with separate
 * products and sums (no FMA):
 *   - grid coordinates: gs_a = (((m_a0 sx + m_a1 sy) + m_a2 sz) + m_a3) * (1 / cell_size) for the sensor s, ge_a likewise for a
 *     point (n x 3 floats, widened to double); i0 = floor(gs), i1 = floor(ge); R = max_range * (1 / cell_size)
 *   - the whole call is refused with SDFGPU_ERR_INVALID_ARGUMENT, nothing written, when s is not finite or not a valid location, or
 *     when R is not in (0, 65536] (NaN included; there is no unlimited range).  A ray whose point is not finite or not a valid
 *     location is skipped: status SDFGPU_DSH_RAY_SKIPPED, nothing written for it
 *   - the walk: d = ge - gs, len2 = (d_x d_x + d_y d_y) + d_z d_z.  Axis a has |i1_a - i0_a| steps left in direction
 *     sign(i1_a - i0_a) and the crossing parameter t_a = (B_a - gs_a) / d_a, B_a the current cell index (+ 1 when the direction is
 *     positive), +inf when no step is left.  A step takes the axis with the smallest t_a (ties: x before y before z), moves one
 *     cell, and recomputes that axis's t_a.  The walk is c_0 = i0 .. c_N = i1, N = sum_a |i1_a - i0_a|, with entry parameters
 *     t_0 = 0 and t_k = the t_a that step k consumed
 *   - range: cell c_k is in range iff (t_k t_k) len2 <= R R, which holds for a prefix of the walk; a ray is long iff len2 > R R
 *   - a ray that is not long carves c_0 .. c_(N-1) and hits c_N (SDFGPU_DSH_RAY_HIT); a long ray carves the in-range prefix of
 *     c_0 .. c_N and hits nothing (SDFGPU_DSH_RAY_TRUNCATED)
 *   - the frame leaves the map as SetCell(c, free_value) for every carved cell of every ray, then SetCell(c, hit_value) for every
 *     hit cell: a cell that one ray carves and another hits ends up hit; absent and chunk-filled chunks the rays cross become
 *     cell-filled as SetCell makes them
 *   - byte_limit refuses the whole frame (SDFGPU_ERR_UNSUPPORTED_SIZE) and leaves the map, its table and its pool as they were: the
 *     table and the pool are sized for the frees and the hits before a cell is stored.  The table is sized for the live chunks plus
 *     a bound on the chunks the frame can enter (the smallest of: rays x chunks a ray of R cells can cross; the chunks within R of
 *     the sensor; the sum over the rays of the chunks between a ray's two ends), which counts a chunk once per ray that enters it
 *     and so may refuse a frame whose chunks would in fact have fitted
 * free_value, hit_value and sensor are host memory.  d_statuses / statuses (optional): one byte per ray; undefined when the call
 * fails.  out_counts (optional, host memory) is filled when the call succeeds.  The device form synchronises the stream once, as
 * the setters do (it reads the number of new chunks and the counts back before the pool may grow), and once more in front of
 * that on a frame whose worst case would make the table grow (the rays' chunks are counted first). */
enum { SDFGPU_DSH_RAY_SKIPPED = 0, SDFGPU_DSH_RAY_HIT = 1, SDFGPU_DSH_RAY_TRUNCATED = 2 };   /* a ray's status byte */

typedef struct sdfgpu_dsh_ray_counts {
    uint64_t rays_hit;
    uint64_t rays_truncated;
    uint64_t rays_skipped;
    uint64_t cells_carved;       /* with multiplicity: the sum of the rays' carved counts */
    uint64_t new_chunks;         /* chunks that were absent before the frame */
} sdfgpu_dsh_ray_counts;

int sdfgpu_dsh_insert_rays_device(sdfgpu_dsh_map map, const double sensor[3], const float* d_points, int64_t n, double max_range,
                                  const void* free_value, const void* hit_value, uint8_t* d_statuses, sdfgpu_dsh_ray_counts* out_counts,
                                  void* stream);
int sdfgpu_dsh_insert_rays(sdfgpu_dsh_map map, const double sensor[3], const float* points, int64_t n, double max_range,
                           const void* free_value, const void* hit_value, uint8_t* statuses, sdfgpu_dsh_ray_counts* out_counts);

/* Sensor rays: fusion.  One frame of a range sensor folded into the cells' occupancies as evidence, where
 * the carve above overwrites them: a cell seen occupied once among many free sightings stays free, and an obstacle that left
 * fades over a few frames.  The contract is this project's own, UNVERIFIED against octomap's insertPointCloud / updateNode and
 * against arc_utilities; tests/dsh_fusion_restated.py restates it.
 *
 * Everything about the rays is the section above, unchanged: grid coordinates, the walk and its tie order, the range prefix, long,
 * hit and skipped rays, the status bytes, the whole-call refusals (sensor, R outside (0, 65536]), n in 0 .. 2^31 - 1, how the
 * table and the pool are sized, what byte_limit refuses and leaves behind, the stream behaviour, and sdfgpu_dsh_ray_counts with the
 * same meanings (cells_carved with multiplicity).  What differs is what the frame does to the cells:
 *   - H is the set of the frame's hit cells; M the set of cells carved by at least one ray, without H
 *   - the frame leaves the map as SetCell(c, fuse(Get(c), prob_hit)) for every c in H and SetCell(c, fuse(Get(c), prob_miss)) for
 *     every c in M: each cell is updated once, whatever the number of rays through it, and a hit beats a miss
 *   - Get(c) is the record before the frame: the default for an absent chunk, the chunk's record for a chunk-filled one; those
 *     chunks become cell-filled as SetCell makes them.  Every other cell of a touched chunk keeps its bytes (NaN payloads too)
 *   - only the occupancy word (the low 4 bytes) of an updated record changes; the component word is kept
 *   - fuse(p, m) in IEEE float32, every operation rounded by itself (no FMA), the division correctly rounded:
 *         q = p >= clamp_min ? p : clamp_min          (a NaN becomes clamp_min)
 *         q = q <= clamp_max ? q : clamp_max
 *         a = q * m
 *         b = (1.0f - q) * (1.0f - m)                 (1.0f - m is computed once, in float)
 *         r = a / (a + b)
 *         r = r >= clamp_min ? r : clamp_min
 *         r = r <= clamp_max ? r : clamp_max
 *     Bayes' rule in probability space: octomap's log-odds addition without logf / expf.  Clamping before the update is what lets
 *     a default of 0.0 or 1.0 ever change
 *   - the whole call is refused with SDFGPU_ERR_INVALID_ARGUMENT, nothing written, unless prob_hit, prob_miss, clamp_min and
 *     clamp_max all lie in [0.001f, 0.999f] and clamp_min <= clamp_max (a NaN fails).  Inside that domain no product is below
 *     1e-6: no operand is denormal and a + b > 0.  prob_miss <= 0.5 <= prob_hit is not required
 * Memory: a map that has taken a fused frame keeps a mark plane, one byte per cell of the pool's capacity (an eighth of the
 * pool's cell bytes) ON TOP of what byte_limit bounds; sdfgpu_dsh_info counts it in scratch_bytes, not in bytes_held.  It is made
 * by the first fused frame and grows with the pool at a fused frame; where it cannot be allocated the frame is refused and the
 * map, its table and its pool are as they were. */
typedef struct sdfgpu_dsh_sensor_model {
    float prob_hit;              /* octomap's defaults: 0.7 */
    float prob_miss;             /*                     0.4 */
    float clamp_min;             /*                     0.12 */
    float clamp_max;             /*                     0.97 */
} sdfgpu_dsh_sensor_model;

int sdfgpu_dsh_fuse_rays_device(sdfgpu_dsh_map map, const double sensor[3], const float* d_points, int64_t n, double max_range,
                                const sdfgpu_dsh_sensor_model* model, uint8_t* d_statuses, sdfgpu_dsh_ray_counts* out_counts,
                                void* stream);
int sdfgpu_dsh_fuse_rays(sdfgpu_dsh_map map, const double sensor[3], const float* points, int64_t n, double max_range,
                         const sdfgpu_dsh_sensor_model* model, uint8_t* statuses, sdfgpu_dsh_ray_counts* out_counts);

/* Removal: chunks leave the map by list or by an axis-aligned box of cells, and the map hands memory back.
 * The reference's map has no removal: the contract is this project's own, like the two sections above;
 * tests/dsh_remove_restated.py restates it.
 *
 * A removed chunk becomes ABSENT: Get on any of its cells returns (default, NOT_FOUND), a window reads the default there, the
 * export no longer lists it, a later SetCell into it makes a fresh cell-filled chunk whose other cells are the default, and a
 * later carved or fused frame treats it as an absent chunk.  Nothing else in the map changes by a byte.
 *
 * sdfgpu_dsh_remove_chunks_device / sdfgpu_dsh_remove_chunks: n in 0 .. 2^31 - 1 locations (n x 3 doubles), each mapped to a
 *   chunk exactly as SetChunk maps it.  The batch leaves the map as if the removals had been applied one after the other in list
 *   order: the first operation in list order that names a live chunk gets SDFGPU_DSH_CHUNK_REMOVED; a later duplicate, an absent
 *   chunk and an invalid location get SDFGPU_DSH_CHUNK_NOT_REMOVED and change nothing.  out_removed (optional, host memory) is
 *   the number of REMOVED.  d_statuses / statuses (optional): one byte per operation; undefined when the call fails.
 * sdfgpu_dsh_retain_box: the box is the global cells lower[a] .. lower[a] + extent[a] - 1, in the coordinates of
 *   sdfgpu_dsh_extract_window's lower.  With invert == 0 every live chunk that holds NO cell of the box is removed (chunks the
 *   box cuts stay whole); with invert != 0 every live chunk that holds AT LEAST ONE cell of the box is removed.  An extent of 0
 *   on any axis is the empty box: invert == 0 then clears the map, invert != 0 removes nothing.  Refused with
 *   SDFGPU_ERR_INVALID_ARGUMENT, nothing written, unless every |lower[a]| <= 2^40 and 0 <= extent[a] <= 2^40.  The host turns the
 *   box into a closed range of chunk coordinates per axis (floor division by the chunk's dimensions, clamped to [-2^20, 2^20));
 *   the kernel compares unpacked keys with it, so nothing can overflow.  lower, extent and out_removed are host memory.
 * sdfgpu_dsh_shrink: the pool is reallocated to max(live + spare_chunks, 1) chunks and the table to the smallest power of two
 *   that is at least 16 and at least 2 (live + spare_chunks) entries, each only where that is smaller than what the map holds
 *   (spare_chunks >= 0).  The mark plane of fused frames, where one exists, is freed; the next fused frame makes it again.
 *   Content is unchanged by a byte, and sdfgpu_dsh_info afterwards reports exactly the planned capacity_chunks, table_capacity
 *   and bytes_held.  If an allocation fails, the map is as it was.
 * All of them: capacity_chunks, table_capacity and bytes_held do not change on a removal; freed pool slots are reused by the next
 *   batch or frame.  No removal is ever refused by byte_limit: it allocates per-call scratch only, and if that fails the map is as
 *   it was.  Which pool slot a chunk lives in is not visible through this interface. */
enum { SDFGPU_DSH_CHUNK_NOT_REMOVED = 0, SDFGPU_DSH_CHUNK_REMOVED = 1 };   /* a removal's status byte */

int sdfgpu_dsh_remove_chunks_device(sdfgpu_dsh_map map, const double* d_locations, int64_t n, uint8_t* d_statuses, int64_t* out_removed,
                                    void* stream);
int sdfgpu_dsh_remove_chunks(sdfgpu_dsh_map map, const double* locations, int64_t n, uint8_t* statuses, int64_t* out_removed);
int sdfgpu_dsh_retain_box(sdfgpu_dsh_map map, const int64_t lower[3], const int64_t extent[3], int invert, int64_t* out_removed,
                          void* stream);
int sdfgpu_dsh_shrink(sdfgpu_dsh_map map, int64_t spare_chunks, void* stream);

/* Ray casts: what does a ray meet first.  The map is read the way the frames above wrote it: one walk per
 * ray, stopped at the first cell that blocks.  The contract is this project's own, UNVERIFIED against octomap's castRay;
 * tests/dsh_cast_restated.py restates it.
 *
 * Everything about a ray is the "Sensor rays" section, unchanged: grid coordinates, i0, i1, d, len2, R = max_range * (1 / cell_size),
 * the walk c_0 .. c_N with its tie order and its entry parameters t_k, "long iff len2 > R R", the in-range prefix
 * (t_k t_k) len2 <= R R, IEEE double with separate products and sums.  A walk between two valid locations never leaves the valid
 * chunk range: each axis moves monotonically between its ends.
 *
 * The result of one ray:
 *   1. W is the walk's cells: c_0 .. c_N for a ray that is not long, the in-range prefix (which always holds c_0) for a long one
 *   2. the tested cells are W, without c_0 when SDFGPU_DSH_CAST_SKIP_FIRST is set, and without c_N (where the walk reaches it)
 *      when SDFGPU_DSH_CAST_SKIP_LAST is set; both together ask "is the segment between these two cells clear, ends excepted"
 *   3. a cell blocks iff the record Get returns there (the default for an absent chunk, the chunk's record for a chunk-filled one,
 *      the cell's own otherwise) satisfies the window predicate on its low 4 bytes read as a float:
 *      occupancy > 0.5f || (SDFGPU_DSH_CAST_UNKNOWN_IS_FILLED && occupancy == 0.5f).  A NaN occupancy never blocks
 *   4. the first tested cell in walk order that blocks gives SDFGPU_DSH_CAST_BLOCKED, and the hit record describes that cell
 *   5. if no tested cell blocks: SDFGPU_DSH_CAST_CLEAR for a ray that is not long, SDFGPU_DSH_CAST_CLEAR_IN_RANGE for a long one;
 *      the hit record then describes the last cell of W, tested or not
 *   6. a ray with an end that is not finite or not a valid location (in the segment form: either end) gets
 *      SDFGPU_DSH_CAST_SKIPPED and a hit record of 48 zero bytes
 * The kernel writes t and takes no square root: a world distance is the caller's arithmetic (t times the length of end - start).
 *
 * sdfgpu_dsh_cast_rays*: one sensor (host memory) and n x 3 float points, exactly as a frame takes them; the whole call is refused
 *   with SDFGPU_ERR_INVALID_ARGUMENT for a sensor that is not finite or not a valid location.
 * sdfgpu_dsh_cast_segments*: n x 3 doubles each for starts and ends (the type of Get's locations); each start goes through the
 *   grid-coordinate expression on the device, and an invalid start skips that ray only.
 * Both: n in 0 .. 2^31 - 1; R must lie in (0, 65536] (NaN refused), which bounds every walk: there is no unlimited range; a flag
 *   bit outside the three is refused; statuses and hits are each optional, but one must be given, and both are undefined when the
 *   call fails; buffers need their natural alignment (points 4, starts / ends 8, statuses 1, hits 8 bytes).  The device forms
 *   enqueue one kernel on the caller's stream and return with it pending, as sdfgpu_dsh_get_device does; they allocate nothing and
 *   are ordered behind the map's last call by the map's event.  The map is not changed by a byte, and sdfgpu_dsh_info reads the
 *   same before and after (the host forms stage through the map's staging buffer, which scratch_bytes counts and a first call may
 *   grow). */
enum { SDFGPU_DSH_CAST_SKIPPED = 0, SDFGPU_DSH_CAST_CLEAR = 1, SDFGPU_DSH_CAST_CLEAR_IN_RANGE = 2, SDFGPU_DSH_CAST_BLOCKED = 3 };   /* a cast's status byte */
enum { SDFGPU_DSH_CAST_SKIP_FIRST = 1, SDFGPU_DSH_CAST_SKIP_LAST = 2, SDFGPU_DSH_CAST_UNKNOWN_IS_FILLED = 4 };                      /* a cast's flags */

typedef struct sdfgpu_dsh_cast_hit {    /* 48 bytes */
    int64_t cell[3];             /* global cell index, the coordinates of sdfgpu_dsh_extract_window's lower */
    uint64_t record;             /* what Get returns there, byte for byte */
    double t;                    /* the cell's entry parameter t_k (0 for c_0): the fraction of start -> end at which the ray enters it */
    uint32_t step;               /* k: the cell's place in the walk */
    uint32_t found;              /* SDFGPU_DSH_NOT_FOUND / FOUND_IN_CHUNK / FOUND_IN_CELL of that cell */
} sdfgpu_dsh_cast_hit;

int sdfgpu_dsh_cast_rays_device(sdfgpu_dsh_map map, const double sensor[3], const float* d_points, int64_t n, double max_range,
                                uint32_t flags, uint8_t* d_statuses, sdfgpu_dsh_cast_hit* d_hits, void* stream);
int sdfgpu_dsh_cast_rays(sdfgpu_dsh_map map, const double sensor[3], const float* points, int64_t n, double max_range, uint32_t flags,
                         uint8_t* statuses, sdfgpu_dsh_cast_hit* hits);
int sdfgpu_dsh_cast_segments_device(sdfgpu_dsh_map map, const double* d_starts, const double* d_ends, int64_t n, double max_range,
                                    uint32_t flags, uint8_t* d_statuses, sdfgpu_dsh_cast_hit* d_hits, void* stream);
int sdfgpu_dsh_cast_segments(sdfgpu_dsh_map map, const double* starts, const double* ends, int64_t n, double max_range, uint32_t flags,
                             uint8_t* statuses, sdfgpu_dsh_cast_hit* hits);

/* Get for n locations: 8-byte records and / or one status byte each (SDFGPU_DSH_NOT_FOUND / FOUND_IN_CHUNK / FOUND_IN_CELL);
 * either output may be null, not both. */
int sdfgpu_dsh_get_device(sdfgpu_dsh_map map, const double* d_locations, int64_t n, void* d_records, uint8_t* d_statuses, void* stream);
int sdfgpu_dsh_get(sdfgpu_dsh_map map, const double* locations, int64_t n, void* records, uint8_t* statuses);

/* A dense window: voxel (x, y, z) of an nx x ny x nz grid (at most 2^32 - 1 voxels) gets what Get returns at global cell
 * lower[] + (x, y, z).  Outputs, either or both: the 8-byte records in x -> y -> z order, and the bit field of
 * sdfgpu_build_bits_device under the CollisionMapGrid predicate (occupancy > 0.5f || (unknown_is_filled && occupancy == 0.5f)),
 * ceil(nx ny nz / 32) words, each written whole by one owner (bits behind the last voxel are 0): the caller clears nothing.
 * A global cell whose chunk coordinate is out of range reads as the default. */
int sdfgpu_dsh_extract_window_device(sdfgpu_dsh_map map, const int64_t lower[3], int64_t nx, int64_t ny, int64_t nz, int unknown_is_filled,
                                     void* d_records, uint32_t* d_bits, void* stream);
int sdfgpu_dsh_extract_window(sdfgpu_dsh_map map, const int64_t lower[3], int64_t nx, int64_t ny, int64_t nz, int unknown_is_filled,
                              void* records, uint32_t* bits);

/* The whole map: the live chunks in ascending (c_x, c_y, c_z) order as sdfgpu_dsh_chunk records, and the cell-filled chunks'
 * cells (x -> y -> z inside a chunk) in the same order.  chunk_capacity is in chunks, cell_capacity in records; the totals
 * always go to out_chunks / out_cells (either may be null), and a list whose capacity is too small is not written (nor is
 * the other), which is not an error: call once with capacities 0 to size the buffers, or use sdfgpu_dsh_info. */
int sdfgpu_dsh_export_device(sdfgpu_dsh_map map, sdfgpu_dsh_chunk* d_chunks, int64_t chunk_capacity, void* d_cells, int64_t cell_capacity,
                             int64_t* out_chunks, int64_t* out_cells, void* stream);
int sdfgpu_dsh_export(sdfgpu_dsh_map map, sdfgpu_dsh_chunk* chunks, int64_t chunk_capacity, void* cells, int64_t cell_capacity,
                      int64_t* out_chunks, int64_t* out_cells);

/* Frontier cells: where seen-free space ends in never-seen space.  The contract is this project's own;
 * tests/dsh_frontier_restated.py restates it.
 *
 * Classes.  For a global cell i take the record Get returns there (the default for an absent chunk or an out-of-range chunk
 * coordinate, the chunk's record for a chunk-filled chunk, the cell's own otherwise) and read its low 4 bytes as a float f:
 *   free iff f < 0.5f; unknown iff f == 0.5f; a NaN is neither.
 * A cell is a frontier cell iff
 *   1. its chunk is live (found != SDFGPU_DSH_NOT_FOUND): a cell of an absent chunk never is one, whatever the default,
 *   2. it is free, and
 *   3. at least one neighbour is unknown: one of the 6 face neighbours, or of all 26 under SDFGPU_DSH_FRONTIER_26.
 * Neighbours are read wherever they lie: in the same chunk, in another live chunk, in an absent chunk or beyond +-2^20 chunks
 * (both: the default).  A window or a box restricts which cells are candidates, never which neighbours are read.  Any flag bit
 * but SDFGPU_DSH_FRONTIER_26 is refused.
 *
 * sdfgpu_dsh_frontier_window*: the bit field of sdfgpu_build_bits_device over the window (bit set iff the voxel's cell is a frontier
 *   cell).  Limits and layout are sdfgpu_dsh_extract_window's: at most 2^32 - 1 voxels, ceil(n / 32) words, each written whole by
 *   one owner, bits behind the last voxel 0.  The device form enqueues one kernel and returns with it pending; it allocates
 *   nothing and is ordered behind the map's last call by the map's event, as the cast and window forms are.
 * sdfgpu_dsh_frontier_cells*: the frontier cells among the cells of live chunks in the box lower[a] .. lower[a] + extent[a] - 1
 *   (the coordinates of the window's lower; every extent[a] >= 1, and lower + extent - 1 must not overflow int64), or, with lower
 *   and extent both null, of the whole map.  int64[3] per cell, in ascending (c_x, c_y, c_z) order of the chunk and ascending cell
 *   slot (l_x n_y + l_y) n_z + l_z inside it: the list is fully determined.  capacity is in cells; the total always goes to
 *   out_total (required), and a list whose capacity is too small is not written, which is not an error (as sdfgpu_dsh_export).
 *   The device form synchronises the stream once, to read the total; its scratch (a count, an offset and a bit mask of
 *   ceil(n_x n_y n_z / 64) 64-bit words per live chunk) is the map's per-call scratch, which scratch_bytes counts.
 * Neither changes the map by a byte, and sdfgpu_dsh_info reads the same before and after except scratch_bytes.  Null or misaligned
 * buffers (bits 4, cells 8 bytes) and bad sizes are refused with SDFGPU_ERR_INVALID_ARGUMENT. */
enum { SDFGPU_DSH_FRONTIER_26 = 1 };   /* a frontier call's flags */

int sdfgpu_dsh_frontier_window_device(sdfgpu_dsh_map map, const int64_t lower[3], int64_t nx, int64_t ny, int64_t nz, uint32_t flags,
                                      uint32_t* d_bits, void* stream);
int sdfgpu_dsh_frontier_window(sdfgpu_dsh_map map, const int64_t lower[3], int64_t nx, int64_t ny, int64_t nz, uint32_t flags,
                               uint32_t* bits);
int sdfgpu_dsh_frontier_cells_device(sdfgpu_dsh_map map, const int64_t lower[3], const int64_t extent[3], uint32_t flags,
                                     int64_t* d_cells, int64_t capacity, int64_t* out_total, void* stream);
int sdfgpu_dsh_frontier_cells(sdfgpu_dsh_map map, const int64_t lower[3], const int64_t extent[3], uint32_t flags, int64_t* cells,
                              int64_t capacity, int64_t* out_total);

/* Dynamic spatial hashed map: connected components.  The labels of the whole map, written in place into
 * the component word (the high 4 bytes) of its records.  The contract is this project's own -- the reference has no such method on
 * this class -- and UNVERIFIED against it; tests/dsh_components_restated.py restates it.
 *
 * Nodes.  Every cell of a cell-filled chunk is a node; every chunk-filled chunk is ONE node (its cells share one record, are of one
 *   class and connected to each other).  Cells of absent chunks are no nodes and connect nothing, as space outside a dense grid
 *   connects nothing.
 * Classes, from the record's low 4 bytes read as a float f.  With flags == 0 the dense rule of sdfgpu_components*: filled iff
 *   f > 0.5f, everything else (unknown and NaN included) free.  With SDFGPU_DSH_COMPONENTS_UNKNOWN_APART three classes: f > 0.5f,
 *   f < 0.5f, and the rest (f == 0.5f and NaN), so that known-free space is not joined with never-seen cells of live chunks.
 * Connectivity.  Two nodes are joined iff they are of the same class and some cell of one is a 6-face neighbour, in global cell
 *   coordinates (across chunk borders too), of some cell of the other.
 * Numbering.  1..K in the order of each component's first node in export order: chunks in ascending (c_x, c_y, c_z), cells in
 *   ascending slot (l_x n_y + l_y) n_z + l_z inside a chunk, a chunk-filled chunk at its chunk's place.  The labels do not depend on
 *   the pool's slot order and are fully determined.
 * Result.  The component word of every cell record of a cell-filled chunk, and of a chunk-filled chunk's record, becomes its
 *   node's label.  No occupancy byte changes; table, pool layout, live counts and bytes_held stay, and Get, the windows, the export
 *   and the casts return what they returned apart from that word -- and hand the labels out as part of the records.
 * Size.  N = cell_filled * cells_per_chunk + chunk_filled must be below 2^32 - 1: otherwise SDFGPU_ERR_UNSUPPORTED_SIZE, and
 *   nothing is written.  An empty map gives K = 0.
 * Validity.  The map keeps K, the flags K was computed under, and whether both still hold.  sdfgpu_dsh_update_components sets all
 *   three.  Every call that changes the map's content clears the validity: the setters and insert_points when at least one location
 *   was valid, insert_rays / fuse_rays when at least one ray was hit or truncated, the removals and retain_box when they removed a
 *   chunk.  A call that is refused, or sets or removes nothing, leaves it; sdfgpu_dsh_shrink moves records byte for byte and keeps
 *   it (and the labels).  K and the validity are the MAP's: every holder of the handle sees the same.
 *
 * sdfgpu_dsh_update_components always recomputes (skipping a valid map is the caller's business).  It runs on `stream`, ordered
 *   like every other call by the map's event, and synchronises the stream twice: behind the count of the chunks by state (N sizes
 *   the scratch and is checked before anything is written) and at its end, to read K back.  out_count may be null.  Any flag bit
 *   but SDFGPU_DSH_COMPONENTS_UNKNOWN_APART is SDFGPU_ERR_INVALID_ARGUMENT.  A call that fails after its first kernel leaves the
 *   validity cleared.
 *   Scratch: 4 bytes per live chunk, 4 bytes per node and the rank tables (a little over 1 bit per node), from the library's
 *   allocator (red zones cover it).  It is the map's per-call scratch: kept between calls, counted in scratch_bytes and NOT
 *   bounded by byte_limit.
 * sdfgpu_dsh_components_info is host-only: it makes no GPU call and waits for nothing.  Any output may be null. */
enum { SDFGPU_DSH_COMPONENTS_UNKNOWN_APART = 1 };   /* sdfgpu_dsh_update_components' flags */

int sdfgpu_dsh_update_components(sdfgpu_dsh_map map, uint32_t flags, uint32_t* out_count, void* stream);
int sdfgpu_dsh_components_info(sdfgpu_dsh_map map, uint32_t* out_count, uint32_t* out_flags, int* out_valid);

/* Red zones (round 6).  With SDFGPU_REDZONE=1 in the environment when sdfgpu_create runs -- or after
 * sdfgpu_set_option(h, "redzone", 1) -- every device allocation of the library (scratch fields, status block, extrema slots,
 * staging buffers, sdfgpu_device_malloc memory) carries 4 KiB of canary bytes in front and behind, and every entry point that
 * may have launched a kernel ends with one check kernel over all of them and a synchronisation: a store outside a buffer
 * fails THAT call with SDFGPU_ERR_REDZONE and a message that names the buffer and the offset.  Debug mode (calls become
 * synchronous; results are unchanged).  sdfgpu_redzone_check runs the same check on demand (wrappers with device buffers from
 * sdfgpu_device_malloc: libsdfgpu_multi); SDFGPU_OK when the mode is off.  Switching the option (on or off) releases every
 * buffer the handle holds (the single and batch builds' scratch, the staging, the scratch of the component, topology, surface,
 * extrema and resample calls), so that it comes back with (or without) canaries: results of earlier calls kept on the handle
 * go with it, and sdfgpu_get_extrema / sdfgpu_get_extrema_batch / sdfgpu_last_batch_info / sdfgpu_convex_last_info answer
 * again after the next call of their kind (until then the batch pair and sdfgpu_convex_last_info return INVALID_ARGUMENT). */
int sdfgpu_redzone_check(sdfgpu_handle h, void* stream);

/* Debug / test hooks: copy the intermediates of the most recent
 * sdfgpu_build*_device call to host buffers (N int16 / N int32). */
int sdfgpu_debug_copy_zsweep(sdfgpu_handle h, int16_t* out_host, int64_t n);
/* ... and float(sqrt((double)D) * resolution) (sdf_generation.hpp:254-265) for D = 0 .. n - 1 (n <= 2^24) into d_out[n] (device):
 * fast = 0 the fp64 sequence of the far-field x sweep, fast = 1 the fp32 form of sdf_tools_amd/csrc/sdfgpu_finish.hpp (round 6: exact,
 * measured slower than the fp64 sequence on MI355X and therefore not used by the kernels; kept with its exhaustive tests);
 * *out_slow_lanes = lanes of the fp32 form that asked for the fp64 sequence. */
int sdfgpu_debug_finish_table(sdfgpu_handle h, float* d_out, int64_t n, double resolution, int fast, uint32_t* out_slow_lanes);
int sdfgpu_debug_copy_yzsweep(sdfgpu_handle h, int32_t* out_host, int64_t n);
/* The device-side habit of the far-field y sweep's two-valued tiles (option "flat_tiles" = 1; synchronises with the last build):
 * out_score = the votes so far -- clamped to [0, 256] in front of every y sweep that consults it, tiles that tried and did not qualify
 * add 1, tiles that qualified subtract 3 -- and out_gate = what the last such sweep was told (1: every candidate tile tries, 0: every
 * 64th).  Results never depend on either. */
int sdfgpu_debug_flat_habit(sdfgpu_handle h, int* out_score, int* out_gate);

/* Per-stage timing with HIP events recorded on the build's own stream (bench.py's roofline leg).
 * While enabled, every sdfgpu_build*_device call brackets its seven stages with events:
 * [0] K0 pack, [1] KD dense ball kernel, [2] K1 z sweep, [3] K2 / K12 y (z+y) sweep, [4] KE2 envelope y
 * sweep, [5] K3 x sweep, [6] KE3 envelope x sweep (a stage that is not launched, or exits on its guard
 * flag, shows ~0).  sdfgpu_get_stage_times
 * synchronises, adds the elapsed times since the last call into out_ms_sum[7] (milliseconds),
 * returns the number of builds they cover in *out_builds and resets the accumulators.
 * enable = 2 brackets only the dominant kernel of the dense path (stage [1]; the other stages then read 0):
 * two events per build instead of five, for timed benchmark loops; enable = 3 does that on every 4th build
 * only (out_builds then counts the sampled builds). */
int sdfgpu_set_profiling(sdfgpu_handle h, int enable);
int sdfgpu_get_stage_times(sdfgpu_handle h, double* out_ms_sum, int64_t* out_builds);

/* Named integer options.  EVERY option leaves the results exact: they move work between kernels, switch a measured optimisation
 * off for an A/B, or put the handle's policy into a state a test needs.  Unknown names return SDFGPU_ERR_INVALID_ARGUMENT.
 * No option skips work: the profiling builds whose switches did were removed after commit 4eb6a2c, and the names of those
 * switches and the switches retired with this commit are unknown names here.
 * [T] = test / fuzz only (forces a state the policy reaches by itself), [AB] = A/B switch of a measured optimisation (default = the
 * faster setting; DESIGN.md / LAB_NOTES.md hold the measurement), [U] = for users.
 *
 *  tier selection                     default  meaning
 *  "dense"                   [U]      1        try the bit-parallel dense tier first (0: sweeps / far-field pair only)
 *  "dense_generic"           [AB]     1        shapes the tuned dense kernels do not take (nz not 32 * 2^k) use their generic forms
 *  "dense_retry"             [U]      16       after an uncertified dense attempt, try again only every N-th build (0: always)
 *  "envelope"                [AB]     1        bound the marching scans and redo far-field sweeps with k_envelope_dc (0: unbounded scans)
 *  "envelope_dc"             [AB]     1        0: never use the far-field kernel
 *  "envelope_mode"           [T]      0        1: the far-field kernel is the only sweep of both axes, no probes
 *  "far_predict"             [U]      1        handles whose recent builds were far-field skip probes + marching launches (0 off, 2 always)
 *  "far_threshold_y/_x"      [T]      16, 9    an axis is far-field when > 1/5 (y), 1/24 (x) of the probed voxels have d^2 >= this
 *  "probe_window"            [AB]     1        tier probes as window statistics (0: level A of the far-field search on sampled tiles)
 *  "policy_reset"            [T]      -        forget what the handle learned from earlier builds
 *  "expect_dense"            [T]      0        put the handle into the "dense tier trusted" state (stand-by pair behind it)
 *  "fixup_mode", "dense3_mode" [T]    0        force the fix-up stage / KD3 in KD's place with the next build
 *
 *  dense tier
 *  "dense3"                  [AB]     1        wide ball kernel KD3 (|offset| <= 3) as the fix-up stage's first kernel
 *  "dense3_staged"           [AB]     1        builds that cannot expect KD to decide the scene carry KD3 + KF behind it, guarded
 *  "dense3_fixed"            [AB]     1        KD3's nz = 512 instance (compile-time row pitch)
 *  "dense_shell"             [AB]     1        shell pass KD6 (16 <= d^2 <= 36) between KD3 and KF
 *  "shell_min_words"         [AB]     128      KD6: open words below which a tile group is left to KF
 *  "standby_far"             [AB]     1        stand-by behind a trusted dense tier = far-field pair (0: fused z+y + marching x, unbounded)
 *  "standby_fold"            [AB]     1        the stand-by x sweep's launch also folds the extrema (one launch less per build)
 *  "standby_single"          [AB]     1        the stand-by y sweep, x sweep and fold are ONE guarded launch (tiles by ticket; 0: two launches)
 *  "standby_grid"            [AB]     1024     workgroups of the stand-by launches
 *  "ball_serpentine"         [AB]     1        a whole build that rewrites the last build's buffer walks KD's tiles in the opposite order
 *
 *  sweeps
 *  "fused_zy"                [AB]     1        let the policy use the fused z+y kernel (0 never, 2 always when the shape allows)
 *  "fused_window"            [AB]     2        its register-window radius at nz = 512 (2 or 3)
 *  "plane16"                 [AB]     1        int16 plane field + int32 side table between the y and x sweeps (0: int32 plane field)
 *  "z_wave"                  [AB]     1        z sweep with whole rows per wave where nz = 64 ... 1024
 *  "x16_voxels_per_lane", "x16_window"  [AB]  4 / 3   K3/16 variant: voxels per lane (4 or 8), window radius (2, 3 or 8)
 *  "i32_handoff"             [AB]     1        far-field pair hands exact int32 plane values from the y to the x sweep
 *  "dc_fixed"                [AB]     1        far-field kernel: instances with the 512- / 1024-voxel line geometry at compile time
 *  "plane_skip"              [AB]     1        builds that go straight to the far-field pair skip the x-planes without a filled voxel
 *  "flat_tiles"              [AB]     1        ... and their y sweep skips its search in tiles whose lines hold at most two values outside
 *                                              their zero sites (a floor under open space, table tops, boxes in open space); tried on
 *                                              grids with a floor and, for y lines longer than 512, on any scene; 1: while it pays (a
 *                                              device-side habit, sdfgpu_debug_flat_habit), 2: every candidate tile tries, 0: never
 *
 *  host side / debugging
 *  "host_pack"               [U]      1        host-buffer builds classify on the host and upload 1 bit / voxel (0: upload + classify on
 *                                              the device; 2: whatever the size)
 *  "defer_fold"              [U]      0        stage entry points leave their maxima in the slots until sdfgpu_fold_extrema_device
 *  "redzone"                 [U]      0        canaries around every device allocation, checked at the end of every call (see above)
 *  "resample_plain_atomics"  [AB]     0        sdfgpu_resample_cells*: one atomic per source cell instead of one per run of neighbouring
 *                                              lanes with the same result cell (DESIGN.md section 21 holds the measurement)
 *  "resample_timing"         [U]      0        HIP events around the two Resample kernels (sdfgpu_debug_resample_times) */
int sdfgpu_set_option(sdfgpu_handle h, const char* name, int value);

/* Which kernels the most recent sdfgpu_build*_device call used: bit 0 = fused z+y kernel (K12),
 * bit 1 = 16-bit plane field (K3/16), bit 2 = dense kernel (K0 + KD) enqueued in front, bit 3 = the guarded
 * stand-by behind a trusted dense tier was the far-field pair (K1 -> KE2 -> KE3, bounded on any scene), bit 4 = the
 * dense stage was its wide form (KD3 + fix-up kernel in KD's place), bit 5 = that form was enqueued BEHIND KD, guarded on
 * KD's verdict (a build that had no reason to expect that KD decides the scene), bit 6 = the far-field pair was enqueued
 * without probes and marching launches because the handle's recent builds were far-field on both axes (option
 * "far_predict": 0 never, 1 learnt -- the default --, 2 every build; exact either way, every 16th build probes again).
 * Also answers for the last sdfgpu_sweep_x_lines_device call: bit 7 = that call chose its tier on the device (the far-field
 * kernel enqueued behind the marching sweep; 0: the marching sweep alone, unbounded).  Bits 8..12 = 1 + the instance of the
 * far-field kernel that the last build or lines call enqueued for its x sweep (0: none): + 1 stage 3, + 2 vector loads, + 4 the
 * looping stand-by form, + 8 512 lanes (lines above 512); 13 / 15 = the instances with a 512- / 1024-voxel line as compile-time
 * constants.  Bit 13 = the stand-by pair of bit 3 was enqueued as ONE launch (option "standby_single").  (Enqueued, not
 * necessarily run: whether a guarded launch did work is sdfgpu_last_dense_certified's far flags.) */
int sdfgpu_last_build_info(sdfgpu_handle h, int* out_fused_zy);

/* Which path did the work of the last build (synchronises): bit 0 = the dense kernel decided every voxel
 * (the general pipeline behind it exited immediately); bit 1 / bit 2 = the y / x sweep was done by the far-field
 * kernel (chosen by the probe, after a marching sweep hit its scan bound, or as the stand-by pair); bits 8..13 = why the
 * dense tier handed the scene on (diagnostics): 8 a staged tile held one class only, 9 a wave without a single decided
 * voxel, 10 a wave with more undecided voxels than the fix-up kernel takes, 11 a tile over the fix-up kernel's cap,
 * 12 a voxel beyond the fix-up kernel's reach (d^2 > 64), 13 a voxel beyond the ball with no fix-up stage behind. */
int sdfgpu_last_dense_certified(sdfgpu_handle h, int* out_certified);

/* Tuning hook (benchmarks): rows marched per thread in the y / x sweeps
 * (0 = automatic). */
int sdfgpu_set_tuning(sdfgpu_handle h, int rows_per_chunk_y, int rows_per_chunk_x);

#ifdef __cplusplus
}
#endif
#endif /* SDFGPU_H */
