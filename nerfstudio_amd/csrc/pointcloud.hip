// Point-cloud export after the model (include/nsamd_pointcloud.h): ordered selection of the rays that become points,
// nsamd_points_select / nsamd_select_below, and the exact k-nearest-neighbour mean distance of the statistical outlier rule,
// nsamd_point_cell_keys / nsamd_knn_mean_distance. What the reference does with two boolean-index passes over four tensors
// per batch plus a host k-d tree (exporter/exporter_utils.py:155-193) stays on the device. The per-element arithmetic is
// pointcloud.h.
#include "block_scan.h"
#include "launch.h"
#include "pointcloud.h"

using namespace nsamd;

namespace {

constexpr int kSelectThreads = NSAMD_SELECT_BLOCK;  // four wavefronts
constexpr int kSelectWaves = kSelectThreads / 64;

// ---- ordered compaction: counts, scan, writes ----------------------------------------------------------------------------------
// scratch: word 0 = the row the launch's first kept entry goes to, or -1 (overflow: nothing is written); from word 1 on, one
// int32 per workgroup: its number of kept entries, turned by the scan into the number kept by the workgroups before it.
// Every placement is a sum of counts: no atomics, no workgroup waits for another inside a launch. The scans are block_scan.h.
struct RayPredicate {
  const float *origins, *directions, *depth, *alpha;
  nsamd_crop_box box;
  __device__ bool operator()(int64_t i, float* p) const { return select_ray(origins, directions, depth, alpha, box, i, p); }
};

struct BelowPredicate {
  const double *avg, *threshold;
  __device__ bool operator()(int64_t i, float*) const { return below_threshold(avg[i], threshold[0]); }
};

__device__ __forceinline__ uint32_t* select_counts(int64_t* scratch) { return reinterpret_cast<uint32_t*>(scratch + 1); }

// kept entries of this workgroup before the calling lane's, and in the whole workgroup. All threads of the block call it.
__device__ __forceinline__ uint32_t block_rank(bool keep, uint32_t* total) {
  const uint32_t mine = keep ? 1u : 0u;
  uint32_t rank;
  block_scan_exclusive_u32<kSelectWaves>(&mine, &rank, total);
  return rank;
}

template <class Predicate>
__global__ __launch_bounds__(kSelectThreads) void select_count_kernel(Predicate pred, int64_t n, int64_t* __restrict__ scratch) {
  const int64_t i = (int64_t)blockIdx.x * kSelectThreads + threadIdx.x;
  float p[3];
  const bool keep = i < n && pred(i, p);
  uint32_t total;
  block_rank(keep, &total);
  if (threadIdx.x == 0) select_counts(scratch)[blockIdx.x] = total;
}

// ONE workgroup: exclusive scan of the counts in place (their sum is at most n < 2^31), then the decision. append: the first
// row is cursor[0], which advances by the total unless that runs past cap — then cursor[1] = 1 and nothing moves. Otherwise
// (select_below) the first row is 0 and cursor[0] receives the total.
__global__ __launch_bounds__(kSelectThreads) void select_scan_kernel(int64_t* __restrict__ scratch, int64_t blocks, int append,
                                                                      int64_t cap, int64_t* __restrict__ cursor) {
  uint32_t* const counts = select_counts(scratch);
  uint64_t sum;
  block_sweep_exclusive_u32<kSelectWaves, 1>(&counts, blocks, &sum);
  if (threadIdx.x != 0) return;
  const int64_t total = (int64_t)sum;
  if (!append) {
    scratch[0] = 0;
    cursor[0] = total;
    return;
  }
  const int64_t first = cursor[0];
  if (first < 0 || first > cap || total > cap - first) {
    scratch[0] = -1;
    cursor[1] = 1;
    return;
  }
  scratch[0] = first;
  cursor[0] = first + total;
}

__global__ __launch_bounds__(kSelectThreads) void points_write_kernel(
    RayPredicate pred, const float* __restrict__ rgb, const float* __restrict__ normals01, int64_t n,
    const int64_t* __restrict__ scratch, float* __restrict__ out_points, float* __restrict__ out_colors,
    float* __restrict__ out_view_dirs, float* __restrict__ out_normals) {
  const int64_t first = scratch[0];
  if (first < 0) return;  // overflow: uniform over the launch
  const int64_t i = (int64_t)blockIdx.x * kSelectThreads + threadIdx.x;
  float p[3];
  const bool keep = i < n && pred(i, p);
  uint32_t total;
  const uint32_t rank = block_rank(keep, &total);
  if (!keep) return;
  const int64_t at = first + (int64_t)(uint32_t)reinterpret_cast<const int32_t*>(scratch + 1)[blockIdx.x] + rank;
  select_store(pred.directions, rgb, pred.alpha, normals01, i, p, at, out_points, out_colors, out_view_dirs, out_normals);
}

__global__ __launch_bounds__(kSelectThreads) void below_write_kernel(BelowPredicate pred, int64_t n,
                                                                      const int64_t* __restrict__ scratch,
                                                                      int64_t* __restrict__ out_indices) {
  const int64_t i = (int64_t)blockIdx.x * kSelectThreads + threadIdx.x;
  const bool keep = i < n && pred(i, nullptr);
  uint32_t total;
  const uint32_t rank = block_rank(keep, &total);
  if (keep) out_indices[(int64_t)(uint32_t)reinterpret_cast<const int32_t*>(scratch + 1)[blockIdx.x] + rank] = i;
}

// ---- neighbour search ------------------------------------------------------------------------------------------------------------
constexpr int kKnnLanes = 64;     // phase A: one wavefront per workgroup, one query per lane
constexpr int kKnnThreads = 128;  // phase B: one workgroup per query; [32][128] doubles of LDS stay below the 64 KiB that need no opt-in
constexpr int kKnnWaves = kKnnThreads / 64;
constexpr int64_t kKnnMaxBlocksB = 8192;  // phase B's grid strides over the unfinished queries, whose number the host never reads

__global__ __launch_bounds__(kSelectThreads) void cell_keys_kernel(const float* __restrict__ points, int64_t n,
                                                                    nsamd_point_grid grid, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kSelectThreads + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
  int32_t c[3];
  grid_cell3(grid, p, c);
  keys[i] = grid_key(grid, c);
}

__global__ void knn_reset_kernel(int32_t* unfinished) { unfinished[0] = 0; }

// Phase A. Lane l of workgroup b takes the query order[64 b + l]: the lanes of a wavefront sit in the same or neighbouring cells
// and walk nearly the same rings. best: [k][64] doubles of LDS. The list of unfinished queries is appended with an atomic counter:
// its order decides nothing, every query writes only its own avg.
__global__ __launch_bounds__(kKnnLanes) void knn_rings_kernel(const float* __restrict__ points, int32_t n,
                                                               const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ cell_start, nsamd_point_grid grid,
                                                               int32_t k, int32_t max_rings, double* __restrict__ avg,
                                                               int32_t* __restrict__ unfinished) {
  extern __shared__ __attribute__((aligned(16))) double knn_lds[];
  const int64_t slot = (int64_t)blockIdx.x * kKnnLanes + threadIdx.x;
  if (slot >= n) return;
  const int32_t query = order[slot];
  const float q[3] = {points[3 * (int64_t)query], points[3 * (int64_t)query + 1], points[3 * (int64_t)query + 2]};
  double* best = knn_lds + threadIdx.x;
  knn_init(best, kKnnLanes, k);
  if (knn_ring_search(points, order, cell_start, grid, q, max_rings, best, kKnnLanes, k)) {
    avg[query] = knn_mean(best, kKnnLanes, k);
  } else {
    unfinished[1 + atomicAdd(unfinished, 1)] = query;
  }
}

// Phase B. Every lane keeps the k best of the points tid, tid + 128, ...; the lists are then merged by k rounds of "the smallest
// head of all lists" ((value, lane) lexicographic, so every lane names the same winner), which yields the k best ascending.
__global__ __launch_bounds__(kKnnThreads) void knn_brute_kernel(const float* __restrict__ points, int32_t n, int32_t k,
                                                                 double* __restrict__ avg,
                                                                 const int32_t* __restrict__ unfinished) {
  // [k][128] candidates, [32] merged, the wavefronts' minima and their lanes: all of it in the dynamic region, whose base then
  // stays aligned for the 8-byte accesses
  extern __shared__ __attribute__((aligned(16))) double knn_lds[];
  double* best = knn_lds + threadIdx.x;
  double* merged = knn_lds + (int64_t)k * kKnnThreads;
  double* wave_value = merged + NSAMD_KNN_MAX_K;
  int32_t* wave_lane = reinterpret_cast<int32_t*>(wave_value + kKnnWaves);
  const int32_t count = unfinished[0];
  for (int32_t u = (int32_t)blockIdx.x; u < count; u += (int32_t)gridDim.x) {
    const int32_t query = unfinished[1 + u];
    const float q[3] = {points[3 * (int64_t)query], points[3 * (int64_t)query + 1], points[3 * (int64_t)query + 2]};
    knn_init(best, kKnnThreads, k);
    for (int64_t j = threadIdx.x; j < n; j += kKnnThreads) knn_insert(best, kKnnThreads, k, knn_dist2(points + 3 * j, q));  // (n up to 2^31 - 1)
    int32_t head = 0;
    for (int32_t round = 0; round < k; ++round) {
      double value = head < k ? best[head * kKnnThreads] : knn_infinity();
      int32_t lane = (int32_t)threadIdx.x;
      for (int step = 1; step < 64; step <<= 1) {  // all 64 lanes end with the wavefront's minimum
        const double other_value = __shfl_xor(value, step);
        const int32_t other_lane = __shfl_xor(lane, step);
        if (other_value < value || (other_value == value && other_lane < lane)) value = other_value, lane = other_lane;
      }
      if ((threadIdx.x & 63) == 0) wave_value[wave_index()] = value, wave_lane[wave_index()] = lane;
      __syncthreads();
      value = wave_value[0], lane = wave_lane[0];
      for (int w = 1; w < kKnnWaves; ++w)
        if (wave_value[w] < value || (wave_value[w] == value && wave_lane[w] < lane)) value = wave_value[w], lane = wave_lane[w];
      if (lane == (int32_t)threadIdx.x) ++head;
      if (threadIdx.x == 0) merged[round] = value;
      __syncthreads();  // wave_value is rewritten by the next round
    }
    if (threadIdx.x == 0) avg[query] = knn_mean(merged, 1, k);
    __syncthreads();  // merged and the lists are rewritten by the next query
  }
}

}  // namespace

extern "C" int nsamd_points_select(const float* origins, const float* directions, const float* depth, const float* rgb,
                                   const float* alpha, const float* normals01, int64_t N, nsamd_crop_box box, float* out_points,
                                   float* out_colors, float* out_view_dirs, float* out_normals, int64_t cap, int64_t* cursor,
                                   int64_t* scratch, nsamd_stream_t stream) {
  const int sizes = select_sizes_check(N, cap);
  if (sizes != NSAMD_OK) return sizes;
  if (N == 0) return NSAMD_OK;
  NSAMD_REQUIRE(origins && directions && depth && rgb && out_points && out_colors && out_view_dirs && cursor && scratch);
  NSAMD_REQUIRE((normals01 == nullptr) == (out_normals == nullptr));
  if (box.enabled != 0)
    for (int a = 0; a < 3; ++a) NSAMD_REQUIRE(box.half_scale[a] >= 0.0f);
  const int64_t nblocks = (N + kSelectThreads - 1) / kSelectThreads;
  unsigned blocks = 0;
  const int status = grid_blocks(nblocks, &blocks);
  if (status != NSAMD_OK) return status;
  const RayPredicate pred{origins, directions, depth, alpha, box};
  hipStream_t s = (hipStream_t)stream;
  select_count_kernel<<<blocks, kSelectThreads, 0, s>>>(pred, N, scratch);
  NSAMD_CHECK_LAUNCH();
  select_scan_kernel<<<1, kSelectThreads, 0, s>>>(scratch, nblocks, 1, cap, cursor);
  NSAMD_CHECK_LAUNCH();
  points_write_kernel<<<blocks, kSelectThreads, 0, s>>>(pred, rgb, normals01, N, scratch, out_points, out_colors, out_view_dirs,
                                                        out_normals);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int nsamd_select_below(const double* avg, int64_t n, const double* threshold, int64_t* out_indices, int64_t* count,
                                  int64_t* scratch, nsamd_stream_t stream) {
  NSAMD_REQUIRE(count != nullptr && scratch != nullptr);
  const int sizes = select_sizes_check(n, 0);
  if (sizes != NSAMD_OK) return sizes;
  NSAMD_REQUIRE(n == 0 || (avg && threshold && out_indices));
  const int64_t nblocks = (n + kSelectThreads - 1) / kSelectThreads;
  unsigned blocks = 0;
  const int status = grid_blocks(nblocks, &blocks);
  if (status != NSAMD_OK) return status;
  const BelowPredicate pred{avg, threshold};
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    select_count_kernel<<<blocks, kSelectThreads, 0, s>>>(pred, n, scratch);
    NSAMD_CHECK_LAUNCH();
  }
  select_scan_kernel<<<1, kSelectThreads, 0, s>>>(scratch, nblocks, 0, 0, count);
  NSAMD_CHECK_LAUNCH();
  if (n > 0) {
    below_write_kernel<<<blocks, kSelectThreads, 0, s>>>(pred, n, scratch, out_indices);
    NSAMD_CHECK_LAUNCH();
  }
  return NSAMD_OK;
}

extern "C" int nsamd_point_cell_keys(const float* points, int64_t n, nsamd_point_grid grid, int64_t* keys,
                                     nsamd_stream_t stream) {
  const int sizes = cell_keys_sizes_check(n, grid);
  if (sizes != NSAMD_OK) return sizes;
  if (n == 0) return NSAMD_OK;
  NSAMD_REQUIRE(points && keys);
  unsigned blocks = 0;
  const int status = grid_blocks((n + kSelectThreads - 1) / kSelectThreads, &blocks);
  if (status != NSAMD_OK) return status;
  cell_keys_kernel<<<blocks, kSelectThreads, 0, (hipStream_t)stream>>>(points, n, grid, keys);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int nsamd_knn_mean_distance(const float* points, int64_t n, const int32_t* order, const int32_t* cell_start,
                                       nsamd_point_grid grid, int32_t k, int32_t max_rings, double* avg, int32_t* unfinished,
                                       nsamd_stream_t stream) {
  const int sizes = knn_sizes_check(n, k, max_rings, grid);
  if (sizes != NSAMD_OK) return sizes;
  if (n == 0) return NSAMD_OK;
  NSAMD_REQUIRE(points && order && cell_start && avg && unfinished);
  const int32_t kk = (int64_t)k < n ? k : (int32_t)n;  // min(k, n) neighbours
  unsigned blocks_a = 0;
  const int status = grid_blocks((n + kKnnLanes - 1) / kKnnLanes, &blocks_a);
  if (status != NSAMD_OK) return status;
  const unsigned blocks_b = (unsigned)(n < kKnnMaxBlocksB ? n : kKnnMaxBlocksB);
  hipStream_t s = (hipStream_t)stream;
  knn_reset_kernel<<<1, 1, 0, s>>>(unfinished);
  NSAMD_CHECK_LAUNCH();
  // dynamic LDS: at most 32 * 64 * 8 = 16 KiB (phase A) and (32 * 128 + 36) * 8 = 32.3 KiB (phase B)
  knn_rings_kernel<<<blocks_a, kKnnLanes, (size_t)kk * kKnnLanes * sizeof(double), s>>>(points, (int32_t)n, order, cell_start, grid,
                                                                                       kk, max_rings, avg, unfinished);
  NSAMD_CHECK_LAUNCH();
  knn_brute_kernel<<<blocks_b, kKnnThreads, ((size_t)kk * kKnnThreads + NSAMD_KNN_MAX_K + 2 * kKnnWaves) * sizeof(double), s>>>(points, (int32_t)n, kk, avg,
                                                                                                  unfinished);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}
