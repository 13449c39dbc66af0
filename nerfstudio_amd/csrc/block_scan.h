// Workgroup-level exclusive scans of 32-bit counts: the two pieces of every ordered stream compaction here (per-workgroup counts,
// a one-workgroup scan of them, writes at count-derived rows: no atomics, no workgroup waits for another) — nsamd_points_select,
// nsamd_select_below (pointcloud.hip), nsamd_mesh_count (mesh.hip). Device-only. Built on wave_scan_inclusive_u32 (wave.h),
// whose DPP steps need all lanes active: EVERY thread of the block calls these and none has returned before; a lane with
// nothing to count passes 0. Not a caller: packed_info_kernel (packed.hip), 1024 threads and per-sweep sums that may pass 2^32.
#pragma once
#include "wave.h"

namespace nsamd {

// Over the 64 * WAVES threads of the block, CHANNELS independent values per thread in ONE call: before[c] = the sum of mine[c]
// over the threads before the caller, total[c] = over the block (modulo 2^32). It owns its LDS words, a row per channel, and the
// barrier between writing and reading them. It does NOT end with a barrier: several values go through one call as channels, and
// a kernel that calls it again puts a __syncthreads() between the calls (the sweep below does) — the next call rewrites words
// that a slower wavefront may still have to read.
template <int WAVES, int CHANNELS = 1>
__device__ __forceinline__ void block_scan_exclusive_u32(const uint32_t* mine, uint32_t* before, uint32_t* total) {
  __shared__ uint32_t wave_total[CHANNELS][WAVES];
  uint32_t inclusive[CHANNELS];
  for (int c = 0; c < CHANNELS; ++c) inclusive[c] = wave_scan_inclusive_u32(mine[c]);  // independent chains: they interleave
  if ((threadIdx.x & 63) == 63)
    for (int c = 0; c < CHANNELS; ++c) wave_total[c][wave_index()] = inclusive[c];
  __syncthreads();
  for (int c = 0; c < CHANNELS; ++c) {
    uint32_t waves_before = 0, sum = 0;
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave_index()) waves_before += wave_total[c][w];
      sum += wave_total[c][w];
    }
    before[c] = waves_before + inclusive[c] - mine[c], total[c] = sum;
  }
}

// ONE workgroup of 64 * WAVES threads: exclusive scan IN PLACE of counts[c][0 .. n) in global memory, 64 * WAVES entries at a
// sweep, CHANNELS arrays at once. Uniform trip count (an entry past n counts 0): every lane stays active. The carries are 64-bit
// and end as totals[c]; an entry gets the low 32 bits of its sum, so one above 2^32 wraps: the caller refuses such totals.
template <int WAVES, int CHANNELS>
__device__ __forceinline__ void block_sweep_exclusive_u32(uint32_t* const* counts, int64_t n, uint64_t* totals) {
  for (int c = 0; c < CHANNELS; ++c) totals[c] = 0;
  for (int64_t base = 0; base < n; base += 64 * WAVES) {
    const int64_t i = base + threadIdx.x;
    uint32_t mine[CHANNELS], before[CHANNELS], chunk[CHANNELS];
    for (int c = 0; c < CHANNELS; ++c) mine[c] = i < n ? counts[c][i] : 0u;
    block_scan_exclusive_u32<WAVES, CHANNELS>(mine, before, chunk);
    for (int c = 0; c < CHANNELS; ++c) {
      if (i < n) counts[c][i] = (uint32_t)totals[c] + before[c];
      totals[c] += chunk[c];
    }
    __syncthreads();  // the scan's LDS words are rewritten by the next sweep
  }
}

}  // namespace nsamd
