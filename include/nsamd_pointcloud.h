/*
 * nsamd_pointcloud.h — the part of libnsamd.so's C ABI that serves point-cloud export (ns-export pointcloud): what
 * generate_point_cloud (exporter/exporter_utils.py:83-223) does after the model. Conventions as in nsamd.h: device pointers,
 * dense row-major tensors, small POD structs passed by value, a hipStream_t; 0 (NSAMD_OK) or a negative nsamd_status, nothing
 * launched on error, no allocation, no synchronisation. Paths are relative to the reference's nerfstudio/ package.
 *
 * The outlier rule (nsamd_knn_mean_distance, nsamd_select_below and the threshold between them) RESTATES Open3D's
 * PointCloud::RemoveStatisticalOutliers from its source and documentation: Open3D itself was not available to compare
 * against. The float64 restatement in tests/pointcloud_reference.py is this project's definition of it.
 */
#ifndef NSAMD_POINTCLOUD_H
#define NSAMD_POINTCLOUD_H

#include "nsamd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NSAMD_SELECT_BLOCK 256 /* rays (entries) per workgroup of the two selection entry points                   */
/* int64 words of `scratch` the selection entry points need for n entries: one header word and one int32 per workgroup */
#define NSAMD_SELECT_SCRATCH_WORDS(n) (1 + (((n) + NSAMD_SELECT_BLOCK - 1) / NSAMD_SELECT_BLOCK + 1) / 2)
#define NSAMD_SELECT_MAX_CAPACITY ((int64_t)1 << 40)
#define NSAMD_KNN_MAX_K 32           /* neighbours per query the kernels keep (Open3D's default nb_neighbors is 20)  */
#define NSAMD_KNN_MAX_CELLS (1 << 24) /* cells of the uniform grid                                                   */

/* Oriented crop box (data/scene_box.py:86-108): a point p is inside when q = world2box · (p, 1) lies STRICTLY inside
 * (-half_scale, +half_scale) on all three axes. world2box: the first three rows of the inverse of [R T; 0 1], row-major. */
typedef struct nsamd_crop_box {
  int32_t enabled; /* 0: every point is inside */
  float world2box[12];
  float half_scale[3]; /* S / 2 */
} nsamd_crop_box;

/* ------------------------------------------------------------------------------------------------------------
 * Selection with order-preserving append (exporter_utils.py:155-178). Per ray i of N: p = o + d * depth (a separately rounded
 * fp32 multiply and add: the bits of torch's `origins + directions * depth`); colour = rgb when alpha is NULL, else
 * rgb / max(alpha, 1e-10) (the "random"-background branch of Model.get_rgba_image, models/base_model.py:216-225); the ray is
 * kept when a > 0.5 — a = 1 without alpha, so every ray passes — and, with the box enabled, p is inside it. The comparisons
 * are false on NaN, as torch's are: a NaN in p (with the box enabled) or in alpha drops the ray.
 * The kept rays are appended IN RAY ORDER — the order of the reference's boolean indexing — at row cursor[0] of
 * out_points, out_colors, out_view_dirs [cap,3] (= p, colour, d) and out_normals [cap,3] (= normals01 * 2 - 1; both NULL or
 * neither), and cursor[0] (int64, on the device) advances by the number kept. If the batch would run past cap, NOTHING of it
 * is written, cursor[0] stays and cursor[1] is set to 1 (it is never cleared here).
 * Three launches: per-workgroup counts, a one-workgroup scan of the counts that also makes the overflow decision, the
 * writes. No atomics, no waiting between workgroups: the same bits run to run, capturable.
 * scratch: NSAMD_SELECT_SCRATCH_WORDS(N) int64 words, contents irrelevant. N == 0 is a no-op; N > 2^31 - 1 or
 * cap > NSAMD_SELECT_MAX_CAPACITY: NSAMD_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------------------------ */
int nsamd_points_select(const float* origins, const float* directions, const float* depth, const float* rgb,
                        const float* alpha, const float* normals01, int64_t N, nsamd_crop_box box, float* out_points,
                        float* out_colors, float* out_view_dirs, float* out_normals, int64_t cap, int64_t* cursor,
                        int64_t* scratch, nsamd_stream_t stream);

/* The same ordered compaction for the outlier rule: out_indices [n] int64 receives, ascending, every i with
 * avg[i] > 0 && avg[i] < threshold[0] (float64, on the device: no host round trip between the reductions and this), and
 * count[0] (int64) their number. scratch as above. n == 0 writes count[0] = 0. */
int nsamd_select_below(const double* avg, int64_t n, const double* threshold, int64_t* out_indices, int64_t* count,
                       int64_t* scratch, nsamd_stream_t stream);

/* Uniform grid over (part of) a point cloud. The box origin + dims * cell_size need not contain every point: a point's cell
 * is its coordinate clamped into the box, per axis. Clamping is a projection onto a convex set and does not increase
 * per-axis differences, so "a point in a cell m rings away is farther than (m - 1) * cell_size" holds outside the box too. */
typedef struct nsamd_point_grid {
  float origin[3];
  float cell_size; /* > 0 */
  int32_t dims[3]; /* >= 1 each, product <= NSAMD_KNN_MAX_CELLS */
} nsamd_point_grid;

/* keys [n] int64: the cell (x * dims[1] + y) * dims[2] + z of every point — the ONE definition of a point's cell, shared
 * with the search below. A NaN coordinate falls into cell 0 of its axis. */
int nsamd_point_cell_keys(const float* points, int64_t n, nsamd_point_grid grid, int64_t* keys, nsamd_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * avg [n] float64: the mean distance of every point to its min(k, n) nearest points of the cloud, ITSELF INCLUDED at distance
 * 0 (Open3D's SearchKNN returns the query point). EXACT: each distance is computed in float64 from the fp32 coordinates
 * (differences, squares, sum, sqrt), the min(k, n) smallest are summed IN ASCENDING ORDER and divided by their number, so the
 * value is a function of the point set alone — not of the grid, the visiting order or the path that found the neighbours.
 * order [n] int32: the points sorted by cell key (stable); cell_start [cells + 1] int32: first position in `order` of every
 * cell. Phase A, one lane per query in cell order: the k best in LDS, rings 0, 1, ... of cells around the query's, done
 * when the k-th best distance is <= ring * cell_size; after max_rings rings the query is appended to `unfinished`. Phase B,
 * one workgroup per unfinished query: ALL points, per-lane candidates merged. max_rings == 0 sends every query to phase B.
 * unfinished [1 + n] int32: word 0 receives the number of phase-B queries, the rest their indices (in no particular
 * order: each query writes only its own avg). A point with a NaN coordinate is nobody's neighbour; its own avg is +inf when
 * it has fewer than min(k, n) finite distances.
 * 1 <= k <= NSAMD_KNN_MAX_K, else NSAMD_ERR_UNSUPPORTED; n > 2^31 - 1 or a grid beyond its limits likewise. n == 0 is a no-op.
 * ------------------------------------------------------------------------------------------------------------ */
int nsamd_knn_mean_distance(const float* points, int64_t n, const int32_t* order, const int32_t* cell_start,
                            nsamd_point_grid grid, int32_t k, int32_t max_rings, double* avg, int32_t* unfinished,
                            nsamd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NSAMD_POINTCLOUD_H */
