// Host build of nerfstudio_amd/csrc/pointcloud.h for tests/test_pointcloud_cpu.py (and tests/hostcheck/pointcloud_main.cc): the
// per-ray and per-query arithmetic of the point-cloud entry points, looped the way the kernels compose it — workgroups of 256
// entries counted, the counts scanned, the kept entries written at count-derived rows; one query per lane in cell order over the
// rings, then the unfinished queries over ALL points with 128 per-lane candidate lists merged by "smallest head". Host memory in
// place of device memory; the size and grid checks are the entry points' own (pointcloud.h). Test infrastructure: the product never loads it.
#include <vector>

#include "../../nerfstudio_amd/csrc/pointcloud.h"

using namespace nsamd;

namespace {

constexpr int64_t kBlock = NSAMD_SELECT_BLOCK;
constexpr int kBruteLanes = 128;

// counts per workgroup -> rows before each workgroup (exclusive scan in place); returns the total
template <class Keep>
int64_t count_and_scan(int64_t n, int32_t* counts, Keep keep) {
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  for (int64_t b = 0; b < blocks; ++b) {
    int32_t c = 0;
    for (int64_t i = b * kBlock; i < n && i < (b + 1) * kBlock; ++i) c += keep(i) ? 1 : 0;
    counts[b] = c;
  }
  int64_t total = 0;
  for (int64_t b = 0; b < blocks; ++b) {
    const int32_t c = counts[b];
    counts[b] = (int32_t)total;
    total += c;
  }
  return total;
}

}  // namespace

extern "C" int hc_points_select(const float* origins, const float* directions, const float* depth, const float* rgb,
                                const float* alpha, const float* normals01, int64_t N, nsamd_crop_box box, float* out_points,
                                float* out_colors, float* out_view_dirs, float* out_normals, int64_t cap, int64_t* cursor,
                                int64_t* scratch) {
  const int sizes = select_sizes_check(N, cap);
  if (sizes != NSAMD_OK) return sizes;
  if (N == 0) return NSAMD_OK;
  if (!(origins && directions && depth && rgb && out_points && out_colors && out_view_dirs && cursor && scratch))
    return NSAMD_ERR_INVALID_ARG;
  if ((normals01 == nullptr) != (out_normals == nullptr)) return NSAMD_ERR_INVALID_ARG;
  int32_t* counts = reinterpret_cast<int32_t*>(scratch + 1);
  float p[3];
  const int64_t total = count_and_scan(N, counts, [&](int64_t i) { return select_ray(origins, directions, depth, alpha, box, i, p); });
  const int64_t first = cursor[0];
  if (first < 0 || first > cap || total > cap - first) {
    scratch[0] = -1;
    cursor[1] = 1;
    return NSAMD_OK;
  }
  scratch[0] = first;
  cursor[0] = first + total;
  for (int64_t b = 0; b * kBlock < N; ++b) {
    int64_t rank = 0;
    for (int64_t i = b * kBlock; i < N && i < (b + 1) * kBlock; ++i) {
      if (!select_ray(origins, directions, depth, alpha, box, i, p)) continue;
      select_store(directions, rgb, alpha, normals01, i, p, first + counts[b] + rank++, out_points, out_colors, out_view_dirs,
                   out_normals);
    }
  }
  return NSAMD_OK;
}

extern "C" int hc_select_below(const double* avg, int64_t n, const double* threshold, int64_t* out_indices, int64_t* count,
                               int64_t* scratch) {
  if (!count || !scratch) return NSAMD_ERR_INVALID_ARG;
  const int sizes = select_sizes_check(n, 0);
  if (sizes != NSAMD_OK) return sizes;
  if (n > 0 && !(avg && threshold && out_indices)) return NSAMD_ERR_INVALID_ARG;
  int32_t* counts = reinterpret_cast<int32_t*>(scratch + 1);
  count[0] = count_and_scan(n, counts, [&](int64_t i) { return below_threshold(avg[i], threshold[0]); });
  for (int64_t b = 0; b * kBlock < n; ++b) {
    int64_t rank = 0;
    for (int64_t i = b * kBlock; i < n && i < (b + 1) * kBlock; ++i)
      if (below_threshold(avg[i], threshold[0])) out_indices[counts[b] + rank++] = i;
  }
  return NSAMD_OK;
}

extern "C" int hc_point_cell_keys(const float* points, int64_t n, nsamd_point_grid grid, int64_t* keys) {
  const int sizes = cell_keys_sizes_check(n, grid);
  if (sizes != NSAMD_OK) return sizes;
  if (n == 0) return NSAMD_OK;
  if (!points || !keys) return NSAMD_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n; ++i) {
    int32_t c[3];
    grid_cell3(grid, points + 3 * i, c);
    keys[i] = grid_key(grid, c);
  }
  return NSAMD_OK;
}

extern "C" int hc_knn_mean_distance(const float* points, int64_t n, const int32_t* order, const int32_t* cell_start,
                                    nsamd_point_grid grid, int32_t k, int32_t max_rings, double* avg, int32_t* unfinished) {
  const int sizes = knn_sizes_check(n, k, max_rings, grid);
  if (sizes != NSAMD_OK) return sizes;
  if (n == 0) return NSAMD_OK;
  if (!(points && order && cell_start && avg && unfinished)) return NSAMD_ERR_INVALID_ARG;
  const int32_t kk = (int64_t)k < n ? k : (int32_t)n;
  unfinished[0] = 0;
  std::vector<double> best((size_t)kk);
  for (int64_t slot = 0; slot < n; ++slot) {  // phase A: the queries in cell order
    const int32_t query = order[slot];
    knn_init(best.data(), 1, kk);
    if (knn_ring_search(points, order, cell_start, grid, points + 3 * (int64_t)query, max_rings, best.data(), 1, kk))
      avg[query] = knn_mean(best.data(), 1, kk);
    else
      unfinished[1 + unfinished[0]++] = query;
  }
  std::vector<double> lists((size_t)kk * kBruteLanes), merged((size_t)kk);
  for (int32_t u = 0; u < unfinished[0]; ++u) {  // phase B: [slot][lane] lists over the points lane, lane + 128, ...
    const int32_t query = unfinished[1 + u];
    int32_t head[kBruteLanes] = {};
    for (int lane = 0; lane < kBruteLanes; ++lane) {
      knn_init(lists.data() + lane, kBruteLanes, kk);
      for (int64_t j = lane; j < n; j += kBruteLanes)
        knn_insert(lists.data() + lane, kBruteLanes, kk, knn_dist2(points + 3 * j, points + 3 * (int64_t)query));
    }
    for (int32_t round = 0; round < kk; ++round) {
      double value = knn_infinity();
      int winner = -1;
      for (int lane = 0; lane < kBruteLanes; ++lane) {
        const double v = head[lane] < kk ? lists[(size_t)head[lane] * kBruteLanes + lane] : knn_infinity();
        if (winner < 0 || v < value) value = v, winner = lane;
      }
      ++head[winner];
      merged[round] = value;
    }
    avg[query] = knn_mean(merged.data(), 1, kk);
  }
  return NSAMD_OK;
}
