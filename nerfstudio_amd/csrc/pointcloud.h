// Per-ray and per-query arithmetic of point-cloud export (gfx950; the host compiler sees it only through tests/hostcheck).
// Reference: nerfstudio/exporter/exporter_utils.py generate_point_cloud :83-223, data/scene_box.py OrientedBox.within :95-108,
// models/base_model.py get_rgba_image :216-225; the outlier rule restates Open3D's RemoveStatisticalOutliers
// (include/nsamd_pointcloud.h). fp32 with the reference's operations in the reference's order where the order decides
// something (the library is built with -ffp-contract=off); the neighbour search is float64 and exact.
#pragma once

#include "common.h"
#include "../../include/nsamd_pointcloud.h"

namespace nsamd {

// ---- argument limits, shared by the entry points and the host build of the tests (no HIP runtime call) --------------------------
constexpr int64_t kPointsMaxN = 0x7fffffffLL;  // entries per call: workgroup counts and their sum stay in 32 bits

NSAMD_HD int select_sizes_check(int64_t n, int64_t cap) {
  if (n < 0 || cap < 0) return NSAMD_ERR_INVALID_ARG;
  return (n > kPointsMaxN || cap > NSAMD_SELECT_MAX_CAPACITY) ? NSAMD_ERR_UNSUPPORTED : NSAMD_OK;
}

NSAMD_HD int point_grid_check(const nsamd_point_grid& g) {
  if (!(g.cell_size > 0.0f) || g.dims[0] < 1 || g.dims[1] < 1 || g.dims[2] < 1) return NSAMD_ERR_INVALID_ARG;
  if (!(g.origin[0] == g.origin[0] && g.origin[1] == g.origin[1] && g.origin[2] == g.origin[2])) return NSAMD_ERR_INVALID_ARG;
  const int64_t cells = (int64_t)g.dims[0] * g.dims[1];  // < 2^62
  if (cells > NSAMD_KNN_MAX_CELLS || cells * g.dims[2] > NSAMD_KNN_MAX_CELLS) return NSAMD_ERR_UNSUPPORTED;
  return NSAMD_OK;
}

NSAMD_HD int cell_keys_sizes_check(int64_t n, const nsamd_point_grid& g) {
  if (n < 0) return NSAMD_ERR_INVALID_ARG;
  const int limits = point_grid_check(g);
  if (limits != NSAMD_OK) return limits;
  return n > kPointsMaxN ? NSAMD_ERR_UNSUPPORTED : NSAMD_OK;
}

NSAMD_HD int knn_sizes_check(int64_t n, int32_t k, int32_t max_rings, const nsamd_point_grid& g) {
  if (n < 0 || max_rings < 0 || k < 1) return NSAMD_ERR_INVALID_ARG;
  if (k > NSAMD_KNN_MAX_K || n > kPointsMaxN) return NSAMD_ERR_UNSUPPORTED;
  return point_grid_check(g);
}

// ---- selection (:155-178) ----------------------------------------------------------------------------------------------------
// One row of world2box · (p, 1), left to right as a dot product is written. (The reference goes through a BLAS matmul whose
// association is its own: the tests exclude points within a few ulp of a face from the comparison with it.)
NSAMD_HD float box_coord(const float* row, const float* p) { return ((row[0] * p[0] + row[1] * p[1]) + row[2] * p[2]) + row[3]; }

// strictly inside on all three axes; false on NaN
NSAMD_HD bool box_within(const nsamd_crop_box& box, const float* p) {
  for (int a = 0; a < 3; ++a) {
    const float q = box_coord(box.world2box + 4 * a, p);
    if (!(q > -box.half_scale[a] && q < box.half_scale[a])) return false;
  }
  return true;
}

// p = o + d * depth for ray i; whether the ray is kept. alpha NULL: a = 1.
NSAMD_HD bool select_ray(const float* origins, const float* directions, const float* depth, const float* alpha,
                         const nsamd_crop_box& box, int64_t i, float* p) {
  const float t = depth[i];
  for (int c = 0; c < 3; ++c) p[c] = origins[3 * i + c] + directions[3 * i + c] * t;
  if (alpha != nullptr && !(alpha[i] > 0.5f)) return false;
  return box.enabled == 0 || box_within(box, p);
}

// the kept ray's rows at position `at` of the outputs
NSAMD_HD void select_store(const float* directions, const float* rgb, const float* alpha, const float* normals01, int64_t i,
                           const float* p, int64_t at, float* out_points, float* out_colors, float* out_view_dirs,
                           float* out_normals) {
  const float a = alpha != nullptr ? fmaxf(alpha[i], 1e-10f) : 1.0f;
  for (int c = 0; c < 3; ++c) {
    out_points[3 * at + c] = p[c];
    out_colors[3 * at + c] = alpha != nullptr ? rgb[3 * i + c] / a : rgb[3 * i + c];
    out_view_dirs[3 * at + c] = directions[3 * i + c];
    if (out_normals != nullptr) out_normals[3 * at + c] = normals01[3 * i + c] * 2.0f - 1.0f;  // :154
  }
}

// the outlier rule's keep test; false on NaN
NSAMD_HD bool below_threshold(double avg, double threshold) { return avg > 0.0 && avg < threshold; }

// ---- uniform grid ------------------------------------------------------------------------------------------------------------
// Cell of a coordinate along one axis: the coordinate clamped into the box. Monotone in x; NaN -> 0.
NSAMD_HD int32_t grid_cell(float x, float origin, float cell_size, int32_t dim) {
  const double t = ((double)x - (double)origin) / (double)cell_size;
  return t >= (double)dim ? dim - 1 : (t > 0.0 ? (int32_t)t : 0);
}

NSAMD_HD void grid_cell3(const nsamd_point_grid& g, const float* p, int32_t* c) {
  for (int a = 0; a < 3; ++a) c[a] = grid_cell(p[a], g.origin[a], g.cell_size, g.dims[a]);
}

NSAMD_HD int64_t grid_key(const nsamd_point_grid& g, const int32_t* c) {
  return ((int64_t)c[0] * g.dims[1] + c[1]) * g.dims[2] + c[2];
}

// ---- k nearest neighbours ----------------------------------------------------------------------------------------------------
// A query's k best SQUARED distances, ascending, at best[slot * stride] (the kernels keep them in LDS as [slot][lane]; a
// runtime-indexed register array would live in scratch memory). sqrt is monotone, so the k smallest squares are the k smallest
// distances; ties carry the same value, so which of them is kept does not matter.
NSAMD_HD double knn_infinity() { return (double)INFINITY; }

NSAMD_HD void knn_init(double* best, int stride, int k) {
  for (int s = 0; s < k; ++s) best[s * stride] = knn_infinity();
}

// differences, squares, sum: float64 from the fp32 coordinates
NSAMD_HD double knn_dist2(const float* a, const float* b) {
  const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// NaN never enters: the comparison is false
NSAMD_HD void knn_insert(double* best, int stride, int k, double d2) {
  if (!(d2 < best[(k - 1) * stride])) return;
  int s = k - 1;
  for (; s > 0 && best[(s - 1) * stride] > d2; --s) best[s * stride] = best[(s - 1) * stride];
  best[s * stride] = d2;
}

// every point of one cell
NSAMD_HD void knn_visit_cell(const float* points, const int32_t* order, const int32_t* cell_start, int64_t cell, const float* q,
                             double* best, int stride, int k) {
  const int32_t end = cell_start[cell + 1];
  for (int32_t j = cell_start[cell]; j < end; ++j) knn_insert(best, stride, k, knn_dist2(points + 3 * (int64_t)order[j], q));
}

// The cells at Chebyshev distance exactly r from cell c, inside the grid.
NSAMD_HD void knn_visit_ring(const float* points, const int32_t* order, const int32_t* cell_start, const nsamd_point_grid& g,
                             const int32_t* c, int32_t r, const float* q, double* best, int stride, int k) {
  const int32_t x0 = c[0] - r < 0 ? 0 : c[0] - r, x1 = c[0] + r >= g.dims[0] ? g.dims[0] - 1 : c[0] + r;
  const int32_t y0 = c[1] - r < 0 ? 0 : c[1] - r, y1 = c[1] + r >= g.dims[1] ? g.dims[1] - 1 : c[1] + r;
  const int32_t z0 = c[2] - r < 0 ? 0 : c[2] - r, z1 = c[2] + r >= g.dims[2] ? g.dims[2] - 1 : c[2] + r;
  for (int32_t x = x0; x <= x1; ++x) {
    const bool x_face = x - c[0] == r || c[0] - x == r;
    for (int32_t y = y0; y <= y1; ++y) {
      const bool xy_face = x_face || y - c[1] == r || c[1] - y == r;
      const int64_t row = ((int64_t)x * g.dims[1] + y) * g.dims[2];
      if (xy_face) {
        for (int32_t z = z0; z <= z1; ++z) knn_visit_cell(points, order, cell_start, row + z, q, best, stride, k);
      } else {  // only the two z faces of the shell, where they are inside the grid
        if (c[2] - r >= 0) knn_visit_cell(points, order, cell_start, row + (c[2] - r), q, best, stride, k);
        if (r > 0 && c[2] + r < g.dims[2]) knn_visit_cell(points, order, cell_start, row + (c[2] + r), q, best, stride, k);
      }
    }
  }
}

// Rings 0 .. max_rings - 1 around the query's cell. After ring r every unvisited point lies in a cell at least r + 1 rings
// away, farther than r * cell_size along one axis (clamped coordinates, which are no farther apart than the true ones). The
// cell index is computed in float64 with two roundings of relative 1.1e-16 each on a value below 2^24: the 1e-9 the bound is
// shortened by covers them a thousand times over. Done too once the rings cover the whole grid. Returns whether the k best
// are final.
NSAMD_HD bool knn_ring_search(const float* points, const int32_t* order, const int32_t* cell_start, const nsamd_point_grid& g,
                              const float* q, int32_t max_rings, double* best, int stride, int k) {
  int32_t c[3];
  grid_cell3(g, q, c);
  int32_t reach = 0;  // the ring that reaches the farthest face of the grid
  for (int a = 0; a < 3; ++a) {
    const int32_t far = c[a] > g.dims[a] - 1 - c[a] ? c[a] : g.dims[a] - 1 - c[a];
    reach = far > reach ? far : reach;
  }
  for (int32_t r = 0; r < max_rings; ++r) {
    knn_visit_ring(points, order, cell_start, g, c, r, q, best, stride, k);
    if (r >= reach) return true;
    const double bound = (double)r * (double)g.cell_size * (1.0 - 1e-9);
    if (best[(k - 1) * stride] <= bound * bound) return true;
  }
  return false;
}

// sqrt of each of the k best, summed in ascending order, over k
NSAMD_HD double knn_mean(const double* best, int stride, int k) {
  double sum = 0.0;
  for (int s = 0; s < k; ++s) sum += sqrt(best[s * stride]);
  return sum / (double)k;
}

}  // namespace nsamd
