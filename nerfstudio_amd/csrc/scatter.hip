// Table-gradient scatter of the hash encoding for gfx950 (backward of HashEncoding.pytorch_fwd,
// /root/reference/nerfstudio/field_components/encodings.py:417-458 — autograd's index_put accumulate into the dense
// [L*T, 2] gradient). HBM-bound byte work: 8 corners x 16 B read-modify-write per (point, level) algorithmically.
//
// fp32 global atomics retire at ~20 G lane-ops/s on this part (profiles/r01_probe_scatter*.log) — 2.9 ms for the
// nerfacto main table — so the scatter is two passes over 16-B records with NO float atomics anywhere:
//
//  PASS 1 (route)  derives every corner update once and appends a record to the queue of the (level, tile) it hashes
//    into. Records are x-PAIRS: idx = x ^ y*P1 ^ z*P2 differs only in low bits between x and x+1, so both
//    x-neighbours of a cell edge share a tile and everything but the x weight: (g0*bz*by, g1*bz*by, wx, ia|ib<<14|flag).
//    Fine levels (scatter_route_fine_kernel): a tile's queue starts with one STATIC segment per pass-1 workgroup, so a
//    record's slot is  segment base + ds_add_rtn rank  — no reservation round trip to global memory, one barrier, the
//    store leaves as soon as the rank is back. Only what overflows a segment (non-uniform levels) takes the classic
//    route: one returning global atomic per (workgroup, tile) into the tile's dynamic area, records recomputed in a
//    second sweep. Coarse levels (scatter_route_runs_kernel, cell wider than the sample spacing): a thread walks 4
//    consecutive samples and sums the corner contributions in registers while the cell stays the same (fixed order),
//    then count -> reserve -> emit in two sweeps.
//  PASS 2 (apply)  one workgroup per tile accumulates its queue in LDS and stores (write-only call) or adds the tile
//    with coalesced accesses.
//
// Determinism: pass 2 accumulates in 64-bit fixed point (scatter.h) with ds_add_u64 — native, fire-and-forget, 3.0
// lane-ops/clk/CU with divergent addresses and no slower on one hot address (the float CAS loop of round 1: 2.2, and
// it collapsed on hot coarse cells). Integer addition is associative, so queue order, the static/dynamic/spill
// routing and the atomics' order do not reach the result: two runs on the same inputs give the same bits. Records that
// find no room in their tile go to a spill list; pass 2 folds the first kSpillFold of them into their tiles (still
// exact and order-free), the finish kernel applies any rest with float atomics and counts them (hdr[kHdrEvtUnordered]).

#include <type_traits>

#include "field_reduce.h"
#include "launch.h"
#include "scatter.h"
#include "wave.h"

NSAMD_PROBE_DEFINE(scatter)

namespace nsamd {

// Gated calls (nsamd_hashgrid_encode_bwd_gated): `gate` points at the flag nsamd_weights_bwd_gate raises when any ray
// of the level carries gradient. While it is clear every value of `denc` would be an exact zero (it is not even
// written), the accumulating scatter adds nothing, and all of its kernels return at once.
__device__ __forceinline__ bool gate_is_clear(const uint32_t* gate) {
  return gate != nullptr && __hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
}

constexpr int kRunLen = 4;        // consecutive samples per thread in the run kernel
constexpr int kRunThreads = 256;  // -> 1024 points per workgroup
constexpr int kMaxLog2Bins = 10;  // pass-1 LDS counters: 3 x 4 levels x bins x 4 B <= 48 KiB

// ---- pass 1, fine levels -------------------------------------------------------------------------------------------
// kThreads x kPts points per workgroup, kLevels levels per thread (position computed once, 4 * kLevels * kPts
// independent record chains per thread to cover the load -> LDS rank -> store latencies).
template <int kThreads, int kPts, int kLevels>
__global__ __launch_bounds__(kThreads) void scatter_route_fine_kernel(
    nsamd_points P, int64_t M, int transform, nsamd_aabb box, nsamd_grid grid, const float* __restrict__ denc,
    int64_t stride_p, int64_t stride_k, ScatterGeom G, LevelList levels, ScatterBufs buf,
    const uint32_t* __restrict__ gate, const uint8_t* __restrict__ ray_mask) {
  static_assert(kPts * kLevels * 4 <= 32, "overflow mask is 32 bits");
  if (gate_is_clear(gate)) return;  // gated call with no gradient anywhere: nothing to route (see scatter_launch)
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_u[];
  const int B = 1 << G.log2_bins;
  uint32_t* cnt = lds_u;               // [kLevels][B] records of this workgroup per tile
  uint32_t* cnt2 = cnt + kLevels * B;  // [kLevels][B] ranks inside the dynamic reservation (second sweep)
  uint32_t* base = cnt2 + kLevels * B; // [kLevels][B] start of the dynamic reservation
  uint32_t* lmax = base + kLevels * B; // [kLevels] max |gradient| bits
  PROBE_STAMP(0, 0);
  for (int t = threadIdx.x; t < 2 * kLevels * B; t += kThreads) cnt[t] = 0u;
  if (threadIdx.x < kLevels) lmax[threadIdx.x] = 0u;
  const int first = blockIdx.y * kLevels;
  int lvl[kLevels];
#pragma unroll
  for (int i = 0; i < kLevels; ++i) lvl[i] = first + i < levels.count ? (int)levels.level[first + i] : -1;
  float g0[kPts][kLevels], g1[kPts][kLevels];
  float x[kPts], y[kPts], z[kPts];
  bool inside[kPts];
  // Every load of the prologue — the ray's mask byte, the 2 * kLevels gradients, the position's inputs — is UNCONDITIONAL (at a
  // clamped point, a level-0 address for an absent level, a dummy byte without a mask) and issued before the first is used;
  // what must not count is zeroed by a select afterwards. Under their predicates (`inside && lvl >= 0`, the mask) each load
  // sat in a branch of its own and was waited for before the next was issued: mask, gradients, bin edges, origin / direction
  // were four memory round trips in a row per workgroup (read off the ISA), which is all a sparse gated call consists of.
  uint8_t mask_raw[kPts];
  int64_t pcl[kPts];
  // (the mask bytes FIRST, alone: a workgroup none of whose rays carries gradient — most of them while the interlevel loss
  //  reaches few rays — leaves after this one small round trip, before it has asked for a single gradient or position)
#pragma unroll
  for (int j = 0; j < kPts; ++j) {
    const int64_t p = ((int64_t)blockIdx.x * kPts + j) * kThreads + threadIdx.x;
    inside[j] = p < M;
    pcl[j] = inside[j] ? p : M - 1;
    // per-ray mask of a gated call: samples of rays without gradient are exact zeros that were never written
    mask_raw[j] = ray_mask != nullptr ? ray_mask[pcl[j] / P.samples_per_ray] : (uint8_t)1;
  }
  if (ray_mask != nullptr) {
    bool marked = false;
#pragma unroll
    for (int j = 0; j < kPts; ++j) marked = marked || (inside[j] && mask_raw[j] != 0);
    if (!__syncthreads_or(marked)) {  // nothing to route: publish the zero segment counts of this workgroup's levels and leave
      for (int t = threadIdx.x; t < kLevels * B; t += kThreads) {
        const int i = t >> G.log2_bins;
        if (lvl[i] < 0) continue;
        const uint32_t tile = ((uint32_t)lvl[i] << G.log2_bins) + (uint32_t)(t & (B - 1));
        buf.counts[(size_t)tile * G.segs + blockIdx.x] = 0u;
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < kPts; ++j) {
    const int64_t pc = pcl[j];
#pragma unroll
    for (int i = 0; i < kLevels; ++i) {
      const float* gptr = denc + pc * stride_p + (int64_t)(2 * (lvl[i] >= 0 ? lvl[i] : 0)) * stride_k;
      g0[j][i] = gptr[0];
      g1[j][i] = gptr[stride_k];
    }
  }
  load_positions_burst<kPts>(P, pcl, x, y, z);
#pragma unroll
  for (int j = 0; j < kPts; ++j) {
    if (ray_mask != nullptr) inside[j] = inside[j] && mask_raw[j] != 0;
#pragma unroll
    for (int i = 0; i < kLevels; ++i) {
      const bool live = inside[j] && lvl[i] >= 0;
      g0[j][i] = live ? g0[j][i] : 0.0f;
      g1[j][i] = live ? g1[j][i] : 0.0f;
    }
    if (inside[j]) {
      (void)normalise_position(transform, box, x[j], y[j], z[j]);
    } else {
      x[j] = y[j] = z[j] = 0.0f;
    }
  }
  // A workgroup whose points carry no gradient at all (proposal levels: the interlevel loss reaches few samples,
  // profiles/r02_study_proposal_sparsity.txt) has nothing to route: it skips the sweep and only publishes its zero
  // segment counts. (`x != 0` is true for NaN: a non-finite gradient is never skipped.) The test rides on the barrier
  // that was here anyway and adds no dependence to the loads above.
  bool carries = false;
#pragma unroll
  for (int j = 0; j < kPts; ++j)
#pragma unroll
    for (int i = 0; i < kLevels; ++i) carries = carries || g0[j][i] != 0.0f || g1[j][i] != 0.0f;
  const int any_gradient = __syncthreads_or(carries);
  PROBE_STAMP(0, 1);
  const uint32_t mask = (1u << grid.log2_table_size) - 1u;
  const int sl = G.slice_log2;
  const uint32_t local_mask = (1u << sl) - 1u;
  const uint32_t C = G.seg_cap;
  const uint32_t static_end = G.segs * C;
  uint32_t over = 0u;  // bit ((j * kLevels + i) * 4 + q): the record found its static segment full

  auto sweep = [&](auto tag) {
    constexpr int SW = decltype(tag)::value;
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
#pragma unroll
      for (int i = 0; i < kLevels; ++i) {
        const int slot = (j * kLevels + i) * 4;
        if (lvl[i] < 0 || !inside[j] || (g0[j][i] == 0.0f && g1[j][i] == 0.0f)) continue;  // adding zero is a no-op
        if (SW == 1 && ((over >> slot) & 0xfu) == 0u) continue;
        const Cell c = locate_cell(x[j], y[j], z[j], grid.scalings[lvl[i]]);
        if (SW == 0) {  // integer compare of |bits|: a NaN or Inf wins and marks the level non-finite
          // (one LDS atomic per live thread and level, as it was: a thread has ONE point, so there is no loop to carry a
          //  running maximum across as the field backward's producer does over its tiles (field_mlp.hip, route_publish_max),
          //  and a fold over the wave in front of the atomic would need every lane here, inside the `continue`s of the
          //  sweep. This kernel is not on the benchmark's step — the main table's records come from the field backward,
          //  the proposal levels go through the run kernel —, so such a fold could not be measured there either.)
          const uint32_t b0 = __float_as_uint(g0[j][i]) & 0x7fffffffu, b1 = __float_as_uint(g1[j][i]) & 0x7fffffffu;
          atomicMax(lmax + i, b0 > b1 ? b0 : b1);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (SW == 1 && !((over >> (slot + q)) & 1u)) continue;
          const PairHash h = pair_hash(c, q, mask);
          const uint32_t bin = h.ia >> sl;
          const uint32_t tile = ((uint32_t)lvl[i] << G.log2_bins) + bin;
          const uint32_t Q = G.level_cap[lvl[i]];
          uint4* const queue = buf.queues + ((size_t)G.level_off[lvl[i]] + (size_t)bin * Q);
          float a0, a1;
          pair_share(c, q, g0[j][i], g1[j][i], a0, a1);
          if ((h.ib >> sl) != bin) {
            // the pair straddles two tiles (needs a carry past bit slice_log2: only when res >= 2^slice_log2, which the
            // host avoids whenever the table allows): two single records through the spill list, in the second sweep
            if (SW == 0) {
              over |= 1u << (slot + q);
            } else {
              spill_append(buf, G.spill_cap, tile,
                           single_record(a0 * (1.0f - c.w[0]), a1 * (1.0f - c.w[0]), h.ia & local_mask));
              spill_append(buf, G.spill_cap, ((uint32_t)lvl[i] << G.log2_bins) + (h.ib >> sl),
                           single_record(a0 * c.w[0], a1 * c.w[0], h.ib & local_mask));
            }
            continue;
          }
          const uint4 rec = pair_record(a0, a1, c.w[0], h.ia & local_mask, h.ib & local_mask);
          if (SW == 0) {
            const uint32_t rank = atomicAdd(cnt + (i << G.log2_bins) + bin, 1u);  // ds_add_rtn_u32
            if (rank < C) rec_store(queue + (blockIdx.x * C + rank), rec);
            else over |= 1u << (slot + q);
          } else {
            const uint32_t pos = base[(i << G.log2_bins) + bin] + atomicAdd(cnt2 + (i << G.log2_bins) + bin, 1u);
            if (pos < Q - static_end) rec_store(queue + (static_end + pos), rec);
            else spill_append(buf, G.spill_cap, tile, rec);
          }
        }
      }
    }
  };

  if (any_gradient) sweep(std::integral_constant<int, 0>{});
  PROBE_STAMP(0, 2);
  const int any_over = __syncthreads_or(over != 0u);
  PROBE_STAMP(0, 3);
  for (int t = threadIdx.x; t < kLevels * B; t += kThreads) {
    const int i = t >> G.log2_bins;
    const int level = first + i < levels.count ? (int)levels.level[first + i] : -1;
    if (level < 0) continue;
    const uint32_t n = cnt[t];
    const uint32_t tile = ((uint32_t)level << G.log2_bins) + (uint32_t)(t & (B - 1));
    buf.counts[(size_t)tile * G.segs + blockIdx.x] = n < C ? n : C;
    if (any_over) base[t] = n > C ? atomicAdd(buf.dyn_cursor + tile, n - C) : 0u;
  }
  if (threadIdx.x < kLevels) {
    const int level = first + (int)threadIdx.x < levels.count ? (int)levels.level[first + threadIdx.x] : -1;
    if (level >= 0 && lmax[threadIdx.x] != 0u) atomicMax(buf.hdr + level, lmax[threadIdx.x]);
  }
  PROBE_STAMP(0, 4);
  if (!any_over) return;
  __syncthreads();
  sweep(std::integral_constant<int, 1>{});
  PROBE_STAMP(0, 5);
}

// ---- pass 1, coarse levels -----------------------------------------------------------------------------------------
// Every thread walks kRunLen CONSECUTIVE samples and merges those that stay in one cell (a run): per-corner sums in
// registers, in sample order. A run of one sample leaves as 4 x-pair records, a longer one as 8 single records
// (value pair + local index). Sweep 0 counts per tile, the workgroup reserves its share of every tile's queue with one
// returning atomic, sweep 1 recomputes the runs and stores — nothing is kept in registers or LDS between the sweeps.
template <int kLevels>
__device__ __forceinline__ void scatter_route_runs_body(
    const nsamd_points& P, int64_t M, int transform, const nsamd_aabb& box, const nsamd_grid& grid,
    const float* __restrict__ denc, int64_t stride_p, int64_t stride_k, const ScatterGeom& G, const LevelList& levels,
    const ScatterBufs& buf, const uint32_t* __restrict__ gate, const uint8_t* __restrict__ ray_mask) {
  if (gate_is_clear(gate)) return;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_u[];
  const int B = 1 << G.log2_bins;
  uint32_t* cnt = lds_u;
  uint32_t* cnt2 = cnt + kLevels * B;
  uint32_t* base = cnt2 + kLevels * B;
  uint32_t* lmax = base + kLevels * B;
  PROBE_STAMP(0, 20);
  for (int t = threadIdx.x; t < 2 * kLevels * B; t += kRunThreads) cnt[t] = 0u;
  if (threadIdx.x < kLevels) lmax[threadIdx.x] = 0u;
  const int first = blockIdx.y * kLevels;
  int lvl[kLevels];
#pragma unroll
  for (int i = 0; i < kLevels; ++i) lvl[i] = first + i < levels.count ? (int)levels.level[first + i] : -1;
  const int64_t p0 = ((int64_t)blockIdx.x * kRunThreads + threadIdx.x) * kRunLen;
  float g0[kRunLen][kLevels], g1[kRunLen][kLevels];
  float px[kRunLen], py[kRunLen], pz[kRunLen];
  bool act[kRunLen];
  // (unconditional loads at clamped points, all issued before the first is used, selects afterwards: see the fine kernel —
  //  here the predicated form was one round trip per sample for the mask and gradients and two more per sample for the position)
  uint8_t mask_raw[kRunLen];
  int64_t pcl[kRunLen];
#pragma unroll
  for (int s = 0; s < kRunLen; ++s) {  // (the mask bytes first, alone: see the fine kernel)
    act[s] = p0 + s < M;
    pcl[s] = act[s] ? p0 + s : M - 1;
    mask_raw[s] = ray_mask != nullptr ? ray_mask[pcl[s] / P.samples_per_ray] : (uint8_t)1;
  }
  if (ray_mask != nullptr) {
    bool marked = false;
#pragma unroll
    for (int s = 0; s < kRunLen; ++s) marked = marked || (act[s] && mask_raw[s] != 0);
    if (!__syncthreads_or(marked)) return;  // (this kernel keeps no per-workgroup state in the workspace)
  }
#pragma unroll
  for (int s = 0; s < kRunLen; ++s) {
    const int64_t pc = pcl[s];
#pragma unroll
    for (int i = 0; i < kLevels; ++i) {
      const float* gptr = denc + pc * stride_p + (int64_t)(2 * (lvl[i] >= 0 ? lvl[i] : 0)) * stride_k;
      g0[s][i] = gptr[0];
      g1[s][i] = gptr[stride_k];
    }
  }
  load_positions_burst<kRunLen>(P, pcl, px, py, pz);
#pragma unroll
  for (int s = 0; s < kRunLen; ++s) {
    if (ray_mask != nullptr) act[s] = act[s] && mask_raw[s] != 0;
#pragma unroll
    for (int i = 0; i < kLevels; ++i) {
      const bool live = act[s] && lvl[i] >= 0;
      g0[s][i] = live ? g0[s][i] : 0.0f;
      g1[s][i] = live ? g1[s][i] : 0.0f;
    }
    if (act[s]) {
      (void)normalise_position(transform, box, px[s], py[s], pz[s]);
    } else {
      px[s] = py[s] = pz[s] = 0.0f;
    }
  }
  // no gradient anywhere in this workgroup's samples: nothing to count, reserve or emit — and this kernel keeps no
  // per-workgroup state in the workspace, so the workgroup may simply leave (the test rides on the barrier that was
  // here anyway; `x != 0` is true for NaN)
  {
    bool carries = false;
#pragma unroll
    for (int s = 0; s < kRunLen; ++s)
#pragma unroll
      for (int i = 0; i < kLevels; ++i) carries = carries || g0[s][i] != 0.0f || g1[s][i] != 0.0f;
    if (!__syncthreads_or(carries)) return;
  }
  PROBE_STAMP(0, 21);
  const uint32_t mask = (1u << grid.log2_table_size) - 1u;
  const int sl = G.slice_log2;
  const uint32_t local_mask = (1u << sl) - 1u;

  auto sweep = [&](auto tag) {
    constexpr int SW = decltype(tag)::value;
    auto emit = [&](int i, uint32_t tile_bin, uint4 rec) {
      const uint32_t tile = ((uint32_t)lvl[i] << G.log2_bins) + tile_bin;
      const uint32_t Q = G.level_cap[lvl[i]];
      if (SW == 0) {
        atomicAdd(cnt + (i << G.log2_bins) + tile_bin, 1u);
      } else {
        const uint32_t pos = base[(i << G.log2_bins) + tile_bin] + atomicAdd(cnt2 + (i << G.log2_bins) + tile_bin, 1u);
        if (pos < Q) rec_store(buf.queues + ((size_t)G.level_off[lvl[i]] + (size_t)tile_bin * Q + pos), rec);
        else spill_append(buf, G.spill_cap, tile, rec);
      }
    };
#pragma unroll
    for (int i = 0; i < kLevels; ++i) {
      if (lvl[i] < 0) continue;
      const float scale = grid.scalings[lvl[i]];
      Cell cur{};
      float a0[8], a1[8];       // per-corner sums of the open run (valid when len >= 2)
      float f0 = 0.f, f1 = 0.f; // gradient of the run's first sample (len == 1: pair records)
      int len = 0;
      uint32_t gmax = 0u;  // max |gradient| bits (integer compare: NaN / Inf win)
#pragma unroll
      for (int s = 0; s <= kRunLen; ++s) {
        bool live = false;
        Cell c = cur;
        if (s < kRunLen) {
          live = (p0 + s < M) && !(g0[s][i] == 0.0f && g1[s][i] == 0.0f);
          if (live) c = locate_cell(px[s], py[s], pz[s], scale);
        }
        const bool same = len > 0 && live && c.lo[0] == cur.lo[0] && c.lo[1] == cur.lo[1] && c.lo[2] == cur.lo[2] &&
                          c.hi[0] == cur.hi[0] && c.hi[1] == cur.hi[1] && c.hi[2] == cur.hi[2];
        if (len > 0 && (s == kRunLen || (live && !same))) {  // the run ends
          if (len == 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const PairHash h = pair_hash(cur, q, mask);
              float v0, v1;
              pair_share(cur, q, f0, f1, v0, v1);
              if ((h.ib >> sl) == (h.ia >> sl)) {
                emit(i, h.ia >> sl, pair_record(v0, v1, cur.w[0], h.ia & local_mask, h.ib & local_mask));
              } else {  // straddling pair: two singles
                emit(i, h.ia >> sl, single_record(v0 * (1.0f - cur.w[0]), v1 * (1.0f - cur.w[0]), h.ia & local_mask));
                emit(i, h.ib >> sl, single_record(v0 * cur.w[0], v1 * cur.w[0], h.ib & local_mask));
              }
            }
          } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const uint32_t idx = corner_index(cur, k, mask);
              emit(i, idx >> sl, single_record(a0[k], a1[k], idx & local_mask));
            }
          }
          len = 0;
        }
        if (s < kRunLen && live) {
          if (SW == 0) {
            const uint32_t b0 = __float_as_uint(g0[s][i]) & 0x7fffffffu, b1 = __float_as_uint(g1[s][i]) & 0x7fffffffu;
            gmax = max(gmax, max(b0, b1));
          }
          if (same) {
            if (len == 1) {  // second sample of the run: open the per-corner sums with the first one (cell weights of cur)
#pragma unroll
              for (int k = 0; k < 8; ++k) {
                a0[k] = corner_share(cur, k, f0);
                a1[k] = corner_share(cur, k, f1);
              }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              a0[k] += corner_share(c, k, g0[s][i]);
              a1[k] += corner_share(c, k, g1[s][i]);
            }
            len += 1;
          } else {
            cur = c;
            f0 = g0[s][i];
            f1 = g1[s][i];
            len = 1;
          }
        }
      }
      // a merged record carries up to kRunLen gradients: the scale bound accounts for that
      // (exponent + 2 = x kRunLen; saturates into the non-finite range only for gradients beyond 2^125)
      // (the running maximum of the thread's kRunLen samples is a register already: one LDS atomic per thread and level)
      if (SW == 0 && gmax != 0u) atomicMax(lmax + i, min(gmax + (2u << 23), 0x7fc00000u));
    }
  };

  sweep(std::integral_constant<int, 0>{});
  PROBE_STAMP(0, 22);
  __syncthreads();
  for (int t = threadIdx.x; t < kLevels * B; t += kRunThreads) {
    const int i = t >> G.log2_bins;
    const int level = first + i < levels.count ? (int)levels.level[first + i] : -1;
    if (level < 0) continue;
    const uint32_t n = cnt[t];
    const uint32_t tile = ((uint32_t)level << G.log2_bins) + (uint32_t)(t & (B - 1));
    base[t] = n ? atomicAdd(buf.dyn_cursor + tile, n) : 0u;
  }
  if (threadIdx.x < kLevels) {
    const int level = first + (int)threadIdx.x < levels.count ? (int)levels.level[first + threadIdx.x] : -1;
    if (level >= 0 && lmax[threadIdx.x] != 0u) atomicMax(buf.hdr + level, lmax[threadIdx.x]);
  }
  __syncthreads();
  PROBE_STAMP(0, 23);
  sweep(std::integral_constant<int, 1>{});
  PROBE_STAMP(0, 24);
}

template <int kLevels>
__global__ __launch_bounds__(kRunThreads) void scatter_route_runs_kernel(
    nsamd_points P, int64_t M, int transform, nsamd_aabb box, nsamd_grid grid, const float* __restrict__ denc,
    int64_t stride_p, int64_t stride_k, ScatterGeom G, LevelList levels, ScatterBufs buf,
    const uint32_t* __restrict__ gate, const uint8_t* __restrict__ ray_mask) {
  scatter_route_runs_body<kLevels>(P, M, transform, box, grid, denc, stride_p, stride_k, G, levels, buf, gate, ray_mask);
}

// TWO independent scatters in one launch (the two proposal levels' table gradients on an update iteration: each of these
// kernels is as long as its slowest workgroup's chain of round trips, not as its work — side by side they cost one such chain).
// blockIdx.z selects the call; a call's own grid is a corner of the launch's.
struct RunsCall {
  nsamd_points P;
  int64_t M;
  int transform;
  nsamd_aabb box;
  nsamd_grid grid;
  const float* denc;
  int64_t stride_p, stride_k;
  ScatterGeom G;
  LevelList levels;
  ScatterBufs buf;
  const uint32_t* gate;
  const uint8_t* ray_mask;
  uint32_t grid_x, grid_y;
};

template <int kLevels>
__global__ __launch_bounds__(kRunThreads) void scatter_route_runs_pair_kernel(RunsCall a, RunsCall b) {
  if (blockIdx.z == 0) {
    if (blockIdx.x >= a.grid_x || blockIdx.y >= a.grid_y) return;
    scatter_route_runs_body<kLevels>(a.P, a.M, a.transform, a.box, a.grid, a.denc, a.stride_p, a.stride_k, a.G, a.levels, a.buf,
                                     a.gate, a.ray_mask);
  } else {
    if (blockIdx.x >= b.grid_x || blockIdx.y >= b.grid_y) return;
    scatter_route_runs_body<kLevels>(b.P, b.M, b.transform, b.box, b.grid, b.denc, b.stride_p, b.stride_k, b.G, b.levels, b.buf,
                                     b.gate, b.ray_mask);
  }
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------
// One workgroup per (level, tile): static segments, dynamic area and the folded part of the spill list are summed into
// an LDS tile of 2 x int64 per entry; the finished tile is converted once and stored / added with coalesced accesses.
// kRider: the launch carries the main field's weight-gradient reduce along (its own instantiation: the rider's registers —
// 118 against 48 — must not cost the small-tile launches of the proposal levels their occupancy).
template <bool kRider>
__device__ __forceinline__ void scatter_apply_body(const nsamd_grid& grid, const ScatterGeom& G, const ScatterBufs& buf,
                                                   float* __restrict__ dtable, int overwrite,
                                                   const uint32_t* __restrict__ gate, const ReduceRider& rider) {
  if (gate_is_clear(gate)) return;
  extern __shared__ __attribute__((aligned(16))) unsigned long long acc[];  // [entries][2]
  if (kRider && (int)blockIdx.y >= G.num_levels) {
    // RIDER workgroups (rows of the grid behind the levels): the main field's weight-gradient reduce, which needs nothing of
    // this pass and which this pass needs nothing of (field_reduce.h) — dispatched after the tiles, they fill the compute
    // units the last round of tiles leaves idle instead of being a launch of their own
    const int block = ((int)blockIdx.y - G.num_levels) * (int)gridDim.x + (int)blockIdx.x;
    if (block < rider.blocks)
      field_dw_reduce_body(reinterpret_cast<float*>(acc), block, rider.partials, rider.num_partials, rider.grads, rider.app_dim,
                           rider.app_rows, rider.cams, rider.num_rays, rider.tiles_per_ray);
    return;
  }
  const int bin = blockIdx.x, level = blockIdx.y;
  const uint32_t tile = ((uint32_t)level << G.log2_bins) + (uint32_t)bin;
  const int entries = 1 << G.slice_log2;
  PROBE_STAMP(0, 10);
  const bool coarse = (G.coarse_mask >> level) & 1u;
  const uint32_t Q = G.level_cap[level], C = G.seg_cap;
  // Everything the tile reads before its first record is asked for HERE, together — the level's maximum, the dynamic cursor,
  // the spill count, and the counts of the wave's first 64 static segments (wave w owns segments w, w + nw, ...; one count
  // per lane): unconditional loads of words that always exist (a lane without a segment, and every lane of a run-routed
  // tile, reads the tile's first count: `counts` holds tiles x segs words with segs >= 1), what must not count is selected
  // away below. These are four-byte COUNT words, one request per wave; no lane asks for a RECORD it does not add. Under their conditions they were three memory round trips in a row in front
  // of every tile — and a compute unit runs its four tiles of the main table one after the other (MI355X, the main table's
  // pass eager: 85.3 -> 84.2 us, profiles/scatter_dense_stream_ab.txt).
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t nw = blockDim.x >> 6;
  const uint32_t* cnts = buf.counts + (size_t)tile * G.segs;
  const uint32_t mine = !coarse && G.segs > wave ? (G.segs - wave + nw - 1u) / nw : 0u;  // static segments of this wave
  const uint32_t cv_first = cnts[(uint32_t)lane < mine ? wave + (uint32_t)lane * nw : 0u];
  const uint32_t max_bits = buf.hdr[level], cursor = buf.dyn_cursor[tile], spilled = buf.hdr[kHdrSpillCount];
  // headroom of the fixed-point sums: <= 2 summands per record (a pair whose corners coincide) over the queue and the
  // folded spill records; one more bit for the sign
  const int headroom = 2 + (32 - __clz((int)(Q + kSpillFold - 1u)));
  const FixedScale fs = fixed_scale(max_bits, headroom);
  if (fs.empty && !overwrite) {
    // an accumulating call and nothing (or only flushed denormals) recorded on this level: the tile stays as it is
    if (threadIdx.x == 0) buf.dyn_cursor[tile] = 0u;
    return;
  }
  const uint32_t static_end = coarse ? 0u : G.segs * C;
  const uint32_t n_dyn = min(cursor, Q - static_end);
  const uint32_t n_spill = min(min(spilled, G.spill_cap), kSpillFold);
  if (!overwrite && n_spill == 0u) {
    // Accumulating call: a tile nothing was routed into (the proposal levels while few rays carry gradient,
    // profiles/r03_proposal_sparsity.txt) keeps its gradient as it is — no LDS fill, no conversion, no read-modify-write.
    // Static segments: one count per pass-1 workgroup, read once here (the accumulation below reads them again from L2).
    bool any = n_dyn != 0u;
    if (!coarse && !any) {
      for (uint32_t sgi = threadIdx.x; sgi < G.segs; sgi += blockDim.x) any = any || cnts[sgi] != 0u;
    }
    if (!__syncthreads_or(any)) {
      if (threadIdx.x == 0) buf.dyn_cursor[tile] = 0u;
      return;
    }
  }
  const uint4* q = buf.queues + ((size_t)G.level_off[level] + (size_t)bin * Q);
  const int kk = fs.k;
  auto add_rec = [&](const uint4& r) {
    const float f0 = rec_f0(r), f1 = rec_f1(r);
    if (rec_is_pair(r)) {  // x-pair: the x factor of the product ((g*wz)*wy)*wx is applied here
      const float wx = rec_wx(r), omx = 1.0f - wx;
      unsigned long long* a = acc + 2 * rec_local_a(r);
      unsigned long long* b = acc + 2 * rec_local_b(r);
      atomicAdd(a, to_fixed(f0 * omx, kk));  // ds_add_u64, no return
      atomicAdd(a + 1, to_fixed(f1 * omx, kk));
      atomicAdd(b, to_fixed(f0 * wx, kk));
      atomicAdd(b + 1, to_fixed(f1 * wx, kk));
    } else {
      unsigned long long* a = acc + 2 * rec_local_a(r);
      atomicAdd(a, to_fixed(f0, kk));
      atomicAdd(a + 1, to_fixed(f1, kk));
    }
  };
  // Static segments, 64 of the wave's at a time (a round). The records of a round's segments are taken as ONE DENSE STREAM:
  // with the exclusive prefix sum of the counts (DPP scan, wave.h) lane l of batch b takes stream position 64 b + l, so
  // every batch but the round's last runs all 64 lanes through the conversions and the LDS atomics. One wave step per
  // segment — the form this replaces — ran the main table's ~48-record segments of the field backward's producers on
  // three quarters of the lanes, issued a second, empty step per segment for records 64 .. 127, and left nearly every
  // lane idle on a sparse call's few-record segments. Integer sums: which lane adds which record does not reach the result.
  // (On its own, with the loads of a trip still settled together, this took the main table's pass from 96.4 to 95.6 us: a
  // quarter of the conversions and LDS atomics gone and next to nothing gained — the pass waits for its records, not for
  // its VALU or the LDS pipe. What the dense stream buys is the ring below.)
  uint32_t c0 = 0u;              // the round's first segment (among the wave's)
  uint32_t cv, pre, total = 0u;  // per lane: the segment's count and the stream position of its first record; the stream's length
  unsigned long long rem = 0ull; // the round's non-empty segments that the stream has not passed yet
  uint4 r[4];
  // (stream position -> record) is a WAVE-UNIFORM WALK over the non-empty segments (their lanes in a ballot, scalar bit
  // scans — an accumulating call on few points leaves most of a tile's segments empty): per segment that overlaps the
  // batch two v_readlane and four VALU (subtract, compare, add, select), against ~60 VALU and four LDS atomics per
  // record batch. A segment that runs past the batch's end stays at the head of the walk for the next batch.
  auto locate = [&](uint32_t first) {  // the queue index of the record at stream position first + lane (calls in stream order)
    const uint32_t p = first + (uint32_t)lane;
    uint32_t idx = 0u;
    while (rem != 0ull) {
      const int j = __builtin_ctzll(rem);
      const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)pre, j);
      if (s >= first + 64u) break;
      const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)cv, j);
      const uint32_t seg0 = (wave + (c0 + (uint32_t)j) * nw) * C;  // (fits 32 bits: inside the tile's queue, Q < 2^30)
      idx = p - s < n ? seg0 - s + p : idx;
      if (s + n > first + 64u) break;
      rem &= rem - 1ull;
    }
    return idx;
  };
  // FULL batches need no lane predicate, so their loads are plain straight-line code: a ring of four batches per wave,
  // each slot reloaded as soon as its record has gone through the LDS atomics — the wave waits for the OLDEST of four
  // loads in flight (s_waitcnt vmcnt(3)), not for all of them. (Per-segment steps had a lane predicate on every load:
  // each sat in a branch of its own, and a trip of loads was settled with vmcnt(0) before the first add. The
  // unconditional form of THAT schedule — idle lanes re-reading a record — measured 2-3 us slower:
  // profiles/r04_negative_results.txt; here no lane asks for anything it does not add.) MI355X, main table, eager:
  // 96.4 -> 85.3 us per launch, three alternating repeats each way (profiles/scatter_dense_stream_ab.txt).
  auto open_stream = [&](uint32_t counts) {  // all 64 lanes; asks for the ring's first four batches
    cv = counts;
    const uint32_t incl = wave_scan_inclusive_u32(cv);
    pre = incl - cv;
    total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    rem = __ballot(cv != 0u);
    if ((total >> 8) != 0u) {
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = rec_load(q + locate(64u * u));
    }
  };
  auto run_stream = [&]() {
    const uint32_t groups = total >> 8;  // groups of 4 full batches
    for (uint32_t g = 1; g < groups; ++g) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        add_rec(r[u]);
        r[u] = rec_load(q + locate(256u * g + 64u * u));
      }
    }
    // the stream's last, partial group (up to 3 full batches and one partly filled): predicated loads, requested
    // before the ring's last four batches are added
    uint4 rt[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t first = 256u * groups + 64u * u;
      const uint32_t idx = locate(first);
      rt[u] = first + (uint32_t)lane < total ? rec_load(q + idx) : make_uint4(0u, 0u, 0u, 0u);
    }
    if (groups != 0u) {
#pragma unroll
      for (int u = 0; u < 4; ++u) add_rec(r[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (256u * groups + 64u * u + (uint32_t)lane < total) add_rec(rt[u]);
  };
  const bool sums = !fs.empty && !fs.bad;
  // the first round's first records are on their way while the tile is cleared
  if (sums && !coarse) open_stream((uint32_t)lane < mine ? cv_first : 0u);
  {
    uint4* z = reinterpret_cast<uint4*>(acc);
    for (int e = threadIdx.x; e < entries; e += blockDim.x) z[e] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  PROBE_STAMP(0, 11);
  // self-cleaning cursor: the next call finds zeros again (the workspace state is zero-initialised once by its owner)
  if (threadIdx.x == 0) buf.dyn_cursor[tile] = 0u;
  if (sums) {
    if (!coarse) {
      run_stream();
      for (c0 = 64u; c0 < mine; c0 += 64u) {
        open_stream(c0 + (uint32_t)lane < mine ? cnts[wave + (c0 + (uint32_t)lane) * nw] : 0u);
        run_stream();
      }
    }
    PROBE_STAMP(0, 12);
    // dynamic area: contiguous, 4 records in flight per thread
    const uint4* dq = q + static_end;
    for (uint32_t e0 = 0; e0 < n_dyn; e0 += blockDim.x * 4u) {
      uint4 r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t e = e0 + (uint32_t)u * blockDim.x + threadIdx.x;
        r[u] = e < n_dyn ? rec_load(dq + e) : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e0 + (uint32_t)u * blockDim.x + threadIdx.x < n_dyn) add_rec(r[u]);
    }
    PROBE_STAMP(0, 13);
    // spill list (normally empty): every tile scans the folded prefix for its own records
    for (uint32_t e = threadIdx.x; e < n_spill; e += blockDim.x)
      if (buf.spill_tile[e] == tile) add_rec(buf.spill_rec[e]);
  }
  PROBE_STAMP(0, 14);
  __syncthreads();
  PROBE_STAMP(0, 15);
  float4* out = reinterpret_cast<float4*>(
      dtable + ((((size_t)level << grid.log2_table_size) + ((size_t)bin << G.slice_log2)) << 1));
  const uint4* a4 = reinterpret_cast<const uint4*>(acc);  // one entry = (lo0, hi0, lo1, hi1)
  const float nan = __uint_as_float(0x7fc00000u);
  for (int i = threadIdx.x; i < entries / 2; i += blockDim.x) {  // two entries = one float4 of the gradient
    const uint4 e0 = a4[2 * i], e1 = a4[2 * i + 1];
    float4 v;
    if (fs.bad) {
      v = make_float4(nan, nan, nan, nan);
    } else {
      v.x = from_fixed(((unsigned long long)e0.y << 32) | e0.x, fs.k);
      v.y = from_fixed(((unsigned long long)e0.w << 32) | e0.z, fs.k);
      v.z = from_fixed(((unsigned long long)e1.y << 32) | e1.x, fs.k);
      v.w = from_fixed(((unsigned long long)e1.w << 32) | e1.z, fs.k);
    }
    if (overwrite) {  // write-only gradient: no zero-fill before the call, no read here
      out[i] = v;
    } else if ((e0.x | e0.y | e0.z | e0.w | e1.x | e1.y | e1.z | e1.w) != 0u || fs.bad) {  // sole owner of the tile
      float4 o = out[i];
      o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
      out[i] = o;
    }
  }
  PROBE_STAMP(0, 16);
}

template <bool kRider>
__global__ void scatter_apply_kernel(nsamd_grid grid, ScatterGeom G, ScatterBufs buf, float* __restrict__ dtable,
                                     int overwrite, const uint32_t* __restrict__ gate, ReduceRider rider) {
  scatter_apply_body<kRider>(grid, G, buf, dtable, overwrite, gate, rider);
}

struct ApplyCall {
  nsamd_grid grid;
  ScatterGeom G;
  ScatterBufs buf;
  float* dtable;
  int overwrite;
  const uint32_t* gate;
};

// two calls' pass 2 in one launch (see scatter_route_runs_pair_kernel); both with the same workgroup size and LDS tile
__global__ void scatter_apply_pair_kernel(ApplyCall a, ApplyCall b) {
  if (blockIdx.z == 0) {
    if (blockIdx.x >= (1u << a.G.log2_bins) || (int)blockIdx.y >= a.G.num_levels) return;
    scatter_apply_body<false>(a.grid, a.G, a.buf, a.dtable, a.overwrite, a.gate, ReduceRider{});
  } else {
    if (blockIdx.x >= (1u << b.G.log2_bins) || (int)blockIdx.y >= b.G.num_levels) return;
    scatter_apply_body<false>(b.grid, b.G, b.buf, b.dtable, b.overwrite, b.gate, ReduceRider{});
  }
}

// After pass 2: spill records beyond the folded prefix (a pathological batch) are applied with float atomics — exact
// sums, but in no fixed order, so they are counted; then the per-call header state goes back to zero.
__device__ __forceinline__ void scatter_finish_body(const nsamd_grid& grid, const ScatterGeom& G, const ScatterBufs& buf,
                                                    float* __restrict__ dtable, const uint32_t* __restrict__ gate) {
  if (gate_is_clear(gate)) return;  // nothing was routed: the per-call state is still zero
  const uint32_t total = buf.hdr[kHdrSpillCount];  // (may exceed the capacity: the excess went out directly)
  const uint32_t n = min(total, G.spill_cap);
  for (uint32_t e = kSpillFold + blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    const uint4 r = buf.spill_rec[e];
    const uint32_t tile = buf.spill_tile[e];
    const uint32_t level = tile >> G.log2_bins, bin = tile & ((1u << G.log2_bins) - 1u);
    float* t = dtable + ((((size_t)level << grid.log2_table_size) + ((size_t)bin << G.slice_log2)) << 1);
    rec_add_unordered(t, r);
  }
  __syncthreads();
  // the last workgroup to finish (every workgroup has read the counter by then) resets the per-call state
  if (threadIdx.x == 0 && atomicAdd(buf.hdr + kHdrTicket, 1u) == gridDim.x - 1) {
    for (int l = 0; l < NSAMD_MAX_LEVELS; ++l) buf.hdr[l] = 0u;
    if (total) {
      buf.hdr[kHdrEvtSpill] += total;
      if (n > kSpillFold) buf.hdr[kHdrEvtUnordered] += n - kSpillFold;
    }
    buf.hdr[kHdrSpillCount] = 0u;
    buf.hdr[kHdrTicket] = 0u;
  }
}

__global__ void scatter_finish_kernel(nsamd_grid grid, ScatterGeom G, ScatterBufs buf, float* __restrict__ dtable,
                                      const uint32_t* __restrict__ gate) {
  scatter_finish_body(grid, G, buf, dtable, gate);
}

__global__ void scatter_finish_pair_kernel(ApplyCall a, ApplyCall b) {  // (same grid for both calls)
  if (blockIdx.z == 0) scatter_finish_body(a.grid, a.G, a.buf, a.dtable, a.gate);
  else scatter_finish_body(b.grid, b.G, b.buf, b.dtable, b.gate);
}

// ---- host ---------------------------------------------------------------------------------------------------------
// fine-kernel shape: threads and levels per thread (one point per thread). Measured on MI355X
// (profiles/r02_scatter_variants.txt): 1024 x 1 x 4 is the fastest or within noise of it; 512 threads, two points per thread,
// two levels per thread and an LDS-staged coalescing variant were slower and are gone.
constexpr int kFineThreads = 1024, kFineLevels = 4;
constexpr int kScatterTargetTiles = 512;

constexpr int kSliceLog2Max = 13;  // 8192 entries x 2 x int64 = 128 KiB of the 160 KiB LDS

// Tiles of a grid: slice_log2, log2_bins and num_levels of `g`. False: no such grid, or more than 2^max_log2_bins tiles per
// level (the LDS counters of whoever routes: kMaxLog2Bins for the route kernels, kProducerMaxLog2Bins for producers).
static bool tile_geometry(const nsamd_grid& grid, int max_log2_bins, ScatterGeom& g) {
  if (grid.num_levels <= 0 || grid.num_levels > NSAMD_MAX_LEVELS) return false;
  int bits = 0;
  while ((grid.num_levels << bits) < kScatterTargetTiles) ++bits;
  int sl = grid.log2_table_size - bits;
  // a tile at least as wide as the finest resolution keeps every x-pair inside one tile (no straddling pairs)
  float res_max = 0.0f;
  for (int l = 0; l < grid.num_levels; ++l) res_max = grid.scalings[l] > res_max ? grid.scalings[l] : res_max;
  int sl_pair = 1;
  while ((1 << sl_pair) < (int)res_max + 2 && sl_pair < kSliceLog2Max) ++sl_pair;
  sl = sl < sl_pair ? sl_pair : sl;
  sl = sl > kSliceLog2Max ? kSliceLog2Max : (sl < 8 ? 8 : sl);
  if (sl > grid.log2_table_size) sl = grid.log2_table_size;
  g.slice_log2 = sl;
  g.log2_bins = grid.log2_table_size - sl;
  g.num_levels = grid.num_levels;
  return g.log2_bins <= max_log2_bins;
}

// The workspace, in 32-bit words: [header | per-tile cursors | counts[tile][seg] | queues | spill records | spill tiles].
// Header and cursors are the state that must be zero before the first call.
struct ScatterLayout {
  int64_t counts, queues, spill_rec, spill_tile, total;  // first word of each region; `counts` = the state's words
};
static ScatterLayout scatter_layout(int64_t tiles, int64_t segs, int64_t queue_records, int64_t spill_cap) {
  ScatterLayout w;
  const int64_t cursor_words = (tiles + 3) & ~(int64_t)3;
  const int64_t count_words = (tiles * segs + 3) & ~(int64_t)3;
  w.counts = kHdrWords + cursor_words;
  w.queues = w.counts + count_words;  // 16-B aligned: all sizes above are multiples of 4 words
  w.spill_rec = w.queues + 4 * queue_records;
  w.spill_tile = w.spill_rec + 4 * spill_cap;
  w.total = w.spill_tile + ((spill_cap + 3) & ~(int64_t)3);
  return w;
}

// Completes a plan whose tile geometry is set: `Q[level]` records per tile queue, of which `segs` static segments of
// `seg_cap`, and a spill list of `spill` records. Sets `ok` unless a count leaves the 32-bit fields of the kernels.
static void plan_queues(ScatterPlan& p, const int64_t* Q, int64_t segs, int64_t seg_cap, int64_t spill) {
  ScatterGeom& g = p.geom;
  const int64_t bins = (int64_t)1 << g.log2_bins;
  p.tiles = bins * g.num_levels;
  int64_t total = 0;
  for (int l = 0; l < g.num_levels; ++l) {
    if (total >= 0x7fffffffLL) return;
    if (Q[l] + (int64_t)kSpillFold >= ((int64_t)1 << 30)) return;  // the per-level headroom is derived in pass 2
    g.level_off[l] = (uint32_t)total;
    g.level_cap[l] = (uint32_t)Q[l];
    total += bins * Q[l];
  }
  if (total >= 0x7fffffffLL || segs >= 0x7fffffffLL || seg_cap >= 0x3fffffffLL || spill >= 0x7fffffffLL) return;
  g.queue_records = (uint32_t)total;
  g.segs = (uint32_t)segs;
  g.seg_cap = (uint32_t)seg_cap;
  g.spill_cap = (uint32_t)spill;
  g.headroom = 0;
  g.coarse_mask = 0u;
  const ScatterLayout w = scatter_layout(p.tiles, segs, total, spill);
  p.state_words = w.counts;
  p.total_words = w.total;
  p.ok = true;
}

ScatterPlan scatter_plan(const nsamd_grid& grid, int64_t M, bool max_spill) {
  ScatterPlan p{};
  ScatterGeom& g = p.geom;
  if (M <= 0 || !tile_geometry(grid, kMaxLog2Bins, g)) return p;
  g.block_points = (uint32_t)kFineThreads;
  const int64_t bins = (int64_t)1 << g.log2_bins;
  const int64_t segs = (M + g.block_points - 1) / g.block_points;
  // static segment: 2x the uniform-hash expectation of 4 pair records per point and level
  int64_t C = 2 * ((4 * (int64_t)g.block_points + bins - 1) / bins);
  C = (C + 3) & ~(int64_t)3;
  if (C < 16) C = 16;
  const int64_t expect = (4 * M + bins - 1) / bins;  // pair records per tile, uniform hash
  // Queue capacity per tile: static segments + a dynamic area, at least 2.5x the uniform-hash expectation. Levels whose
  // lattice (res + 1)^3 fills less than half of the table are SPARSE: their few reachable entries concentrate the updates
  // of whole regions of space on a handful of tiles (r02b: level 0 of the bench overflowed a 2.5x queue on every step),
  // so they get 8x.
  int64_t Qn = segs * C + expect / 2 + 64;
  if (Qn < 2 * expect + expect / 2 + 64) Qn = 2 * expect + expect / 2 + 64;  // run-mode levels use the whole queue
  Qn = (Qn + 3) & ~(int64_t)3;
  int64_t Qs = segs * C + 6 * expect + 64;
  if (Qs < 8 * expect + 64) Qs = 8 * expect + 64;
  Qs = (Qs + 3) & ~(int64_t)3;
  int64_t Q[NSAMD_MAX_LEVELS];
  for (int l = 0; l < grid.num_levels; ++l) {
    const double lattice = ((double)grid.scalings[l] + 1.0) * ((double)grid.scalings[l] + 1.0) * ((double)grid.scalings[l] + 1.0);
    Q[l] = lattice * 2.0 <= (double)((int64_t)1 << grid.log2_table_size) ? Qs : Qn;
  }
  // spill list: worst case (every record of the call: 4 pairs, or after run merging at most as many singles, per point
  // and level) for write-only calls; otherwise a quarter of the expected total
  int64_t spill = 4 * M * grid.num_levels + 64;
  if (!max_spill) {
    const int64_t part = M * grid.num_levels + 4096;
    spill = spill < part ? spill : part;
  }
  plan_queues(p, Q, segs, C, spill);
  return p;
}

ScatterPlan scatter_plan_in(const nsamd_grid& grid, int64_t M, bool max_spill, const float* workspace, int64_t workspace_floats) {
  ScatterPlan p{};
  if (workspace != nullptr) p = scatter_plan(grid, M, max_spill);
  if (p.ok && p.total_words > workspace_floats) p.ok = false;
  return p;
}

ScatterPlan scatter_plan_producers(const nsamd_grid& grid, int64_t M, int workgroups, int seg_cap) {
  ScatterPlan p{};
  ScatterGeom& g = p.geom;
  // tiles as scatter_plan chooses them; the producer keeps one LDS counter per (level, tile)
  if (M <= 0 || workgroups <= 0 || seg_cap < 16 || !tile_geometry(grid, kProducerMaxLog2Bins, g)) return p;
  g.block_points = 0u;
  const int64_t bins = (int64_t)1 << g.log2_bins;
  const int64_t segs = workgroups, C = (seg_cap + 3) & ~3;
  const int64_t expect = (4 * M + bins - 1) / bins;  // pair records per tile, uniform hash
  // static segments (scripts/study_fused_route_overflow.py: a 256-record segment holds every level of the benchmark's
  // batches but ~60 records of level 0) + a dynamic area for what overflows them
  int64_t Q[NSAMD_MAX_LEVELS];
  for (int l = 0; l < grid.num_levels; ++l) Q[l] = (segs * C + expect / 2 + 64 + 3) & ~(int64_t)3;
  // spill list, worst case: the gradient is write-only, nothing may be lost
  plan_queues(p, Q, segs, C, 4 * M * grid.num_levels + 64);
  return p;
}

ScatterBufs scatter_bufs(float* workspace, const ScatterPlan& p) {
  const ScatterLayout w = scatter_layout(p.tiles, p.geom.segs, p.geom.queue_records, p.geom.spill_cap);
  ScatterBufs b;
  uint32_t* base = reinterpret_cast<uint32_t*>(workspace);
  b.hdr = base;
  b.dyn_cursor = base + kHdrWords;
  b.counts = base + w.counts;
  b.queues = reinterpret_cast<uint4*>(base + w.queues);
  b.spill_rec = reinterpret_cast<uint4*>(base + w.spill_rec);
  b.spill_tile = base + w.spill_tile;
  b.direct_table = nullptr;
  b.log2_table_size = 0;
  b.log2_bins = p.geom.log2_bins;
  b.slice_log2 = p.geom.slice_log2;
  return b;
}

// 128 KiB of dynamic LDS need the opt-in, per device
static int apply_lds_attribute() {
  static LdsOptIn opted_in;
  const size_t bytes = (size_t)16 << kSliceLog2Max;
  return lds_opt_in(opted_in, scatter_apply_kernel<false>, bytes, scatter_apply_kernel<true>, bytes, scatter_apply_pair_kernel, bytes);
}

// threads of an apply-pass workgroup for tiles of 2^slice_log2 entries
static unsigned apply_threads(int slice_log2) {
  return slice_log2 > 11 ? 1024u : (slice_log2 > 9 ? 512u : 256u);
}

bool scatter_apply_takes_rider(const ScatterPlan& plan) { return apply_threads(plan.geom.slice_log2) == 1024u; }

// Which levels of a call go through the run-merging kernel (coarse) and which through the plain route (fine); sets G.coarse_mask.
// Levels whose cells are wide against the sample spacing go through the run-merging kernel: with >= 192 samples per
// ray (the first proposal level) consecutive samples share cells on every level of the small proposal grids and
// merging pays (75 vs 107 us at M = 1 M); with 48 samples per ray the plain route is faster on every level
// (178 vs 197 us for the main table; profiles/r02a_*).
static void classify_levels(const nsamd_points& pts, const nsamd_grid& grid, ScatterGeom& G, LevelList& coarse,
                            LevelList& fine) {
  float coarse_below = 0.0f;
  // Round 6 (profiles/r06_s12_*, r06_s14_*): since the run kernel and the apply pass on non-empty segments (rounds 3 - 5) the
  // 96-sample level is cheaper merged as well — its route + apply read 40 + 37 us plain against 35 + 9 us for the 2.7 x larger
  // 256-sample level merged; all five of its levels through the run kernel: long run 0.6919 / 0.6883 against 0.6971 / 0.6959 ms
  // from step 40, window 0.657 / 0.658 against 0.667 / 0.667 from step 0.
  if (pts.positions == nullptr && pts.samples_per_ray >= 96)
    coarse_below = pts.samples_per_ray >= 192 ? (float)pts.samples_per_ray : 1e30f;
  for (int l = 0; l < grid.num_levels; ++l) {
    if (grid.scalings[l] < coarse_below) {
      G.coarse_mask |= 1u << l;
      coarse.level[coarse.count++] = (int8_t)l;
    } else {
      fine.level[fine.count++] = (int8_t)l;
    }
  }
}

// levels per thread of the run kernel: fewer levels per thread = more, shorter workgroups — its time is the latency of one
// workgroup's two sweeps (profiles/r03_sparse_regime_kernel_stats.csv)
// (MI355X, driver window of the bench: 4 -> 75 us, 2 -> 54, 1 -> 54 per launch of the 256-sample level's scatter)
constexpr int kRunLevels = 2;

// A checked call with everything its launches take: what the kernels are passed, and the shapes of the run kernel's launch
// (coarse levels) and of the apply pass's.
struct ScatterPrepared {
  ScatterGeom G;  // coarse_mask set
  ScatterBufs buf;  // log2_table_size and direct_table set
  LevelList coarse, fine;
  dim3 runs_grid, apply_grid;  // (apply: without a rider's rows)
  size_t runs_lds, apply_lds;
  unsigned apply_threads;
};

static int scatter_prepare(const ScatterCall& c, ScatterPrepared& p) {
  NSAMD_REQUIRE(c.plan.ok);                          // (a plan the caller's scratch does not hold is not ok: scatter_plan_in)
  NSAMD_REQUIRE(c.gate == nullptr || !c.overwrite);  // a write-only gradient must always be written
  NSAMD_REQUIRE(c.ray_mask == nullptr || (c.gate != nullptr && c.pts.positions == nullptr));  // ray mode only
  p.G = c.plan.geom;
  p.buf = scatter_bufs(c.workspace, c.plan);
  p.buf.log2_table_size = c.grid.log2_table_size;
  if (!c.overwrite) p.buf.direct_table = c.dtable;
  p.coarse = LevelList{};
  p.fine = LevelList{};
  classify_levels(c.pts, c.grid, p.G, p.coarse, p.fine);
  const int64_t per_block = (int64_t)kRunThreads * kRunLen;
  p.runs_grid = dim3((unsigned)((c.M + per_block - 1) / per_block), (unsigned)((p.coarse.count + kRunLevels - 1) / kRunLevels));
  p.runs_lds = sizeof(uint32_t) * (3 * (size_t)kRunLevels * ((size_t)1 << p.G.log2_bins) + kRunLevels);
  p.apply_grid = dim3(1u << p.G.log2_bins, (unsigned)c.grid.num_levels);
  p.apply_lds = (size_t)16 << p.G.slice_log2;
  p.apply_threads = apply_threads(p.G.slice_log2);
  return apply_lds_attribute();
}

// apply (pass 2) + finish of a prepared call; `rider` (nullable): extra rows of workgroups behind the levels
static int scatter_apply_finish(const ScatterCall& c, const ScatterPrepared& p, const ReduceRider* rider, hipStream_t st) {
  dim3 g2 = p.apply_grid;
  const int overwrite = c.overwrite ? 1 : 0;
  if (rider != nullptr && rider->blocks > 0) {
    if (p.apply_threads != (unsigned)kReduceThreads) return NSAMD_ERR_UNSUPPORTED;  // (callers check `scatter_apply_takes_rider` first)
    g2.y += ((unsigned)rider->blocks + g2.x - 1u) >> p.G.log2_bins;
    scatter_apply_kernel<true><<<g2, p.apply_threads, p.apply_lds, st>>>(c.grid, p.G, p.buf, c.dtable, overwrite, c.gate, *rider);
  } else {
    scatter_apply_kernel<false><<<g2, p.apply_threads, p.apply_lds, st>>>(c.grid, p.G, p.buf, c.dtable, overwrite, c.gate,
                                                                         ReduceRider{});
  }
  NSAMD_CHECK_LAUNCH();
  scatter_finish_kernel<<<32, 256, 0, st>>>(c.grid, p.G, p.buf, c.dtable, c.gate);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

int scatter_apply_launch(const nsamd_grid& grid, const ScatterPlan& plan, float* workspace, float* dtable, bool overwrite,
                         hipStream_t st, const ReduceRider* rider) {
  // (no points: nothing is routed here, and every level's records sit in static segments + dynamic area)
  const ScatterCall c{nsamd_points{}, 0, 0, nsamd_aabb{}, grid, nullptr, 0, 0, dtable, workspace, plan, overwrite, nullptr, nullptr};
  ScatterPrepared p;
  const int rc = scatter_prepare(c, p);
  return rc ? rc : scatter_apply_finish(c, p, rider, st);
}

// route (fine levels, then coarse levels) + apply + finish of one prepared call
static int scatter_launch_one(const ScatterCall& c, const ScatterPrepared& p, hipStream_t st) {
  if (p.fine.count > 0) {
    const size_t lds = sizeof(uint32_t) * (3 * (size_t)kFineLevels * ((size_t)1 << p.G.log2_bins) + kFineLevels);
    dim3 g1(p.G.segs, (unsigned)((p.fine.count + kFineLevels - 1) / kFineLevels));
    scatter_route_fine_kernel<kFineThreads, 1, kFineLevels><<<g1, kFineThreads, lds, st>>>(
        c.pts, c.M, c.transform, c.aabb, c.grid, c.denc, c.stride_p, c.stride_k, p.G, p.fine, p.buf, c.gate, c.ray_mask);
    NSAMD_CHECK_LAUNCH();
  }
  if (p.coarse.count > 0) {
    scatter_route_runs_kernel<kRunLevels><<<p.runs_grid, kRunThreads, p.runs_lds, st>>>(
        c.pts, c.M, c.transform, c.aabb, c.grid, c.denc, c.stride_p, c.stride_k, p.G, p.coarse, p.buf, c.gate, c.ray_mask);
    NSAMD_CHECK_LAUNCH();
  }
  return scatter_apply_finish(c, p, nullptr, st);
}

// Two calls share their route, apply and finish launches (blockIdx.z selects the call; a call's own grid is a corner of the
// launch's) when both route every level through the run kernel (the proposal levels of nerfacto: 256 and 96 samples per ray
// on small grids), with the same apply workgroup size, and share neither workspace nor gradient.
static bool scatter_pair_shares_launches(const ScatterCall* c, const ScatterPrepared* p) {
  for (int i = 0; i < 2; ++i)
    if (p[i].fine.count != 0 || p[i].coarse.count == 0) return false;
  return c[0].workspace != c[1].workspace && c[0].dtable != c[1].dtable && p[0].apply_threads == p[1].apply_threads;
}

static int scatter_launch_pair(const ScatterCall* c, const ScatterPrepared* p, hipStream_t st) {
  RunsCall rc[2];
  ApplyCall ac[2];
  for (int i = 0; i < 2; ++i) {
    rc[i] = RunsCall{c[i].pts, c[i].M, c[i].transform, c[i].aabb, c[i].grid, c[i].denc, c[i].stride_p, c[i].stride_k, p[i].G,
                     p[i].coarse, p[i].buf, c[i].gate, c[i].ray_mask, p[i].runs_grid.x, p[i].runs_grid.y};
    ac[i] = ApplyCall{c[i].grid, p[i].G, p[i].buf, c[i].dtable, c[i].overwrite ? 1 : 0, c[i].gate};
  }
  const auto larger = [](dim3 a, dim3 b) { return dim3(a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y, 2u); };
  scatter_route_runs_pair_kernel<kRunLevels><<<larger(p[0].runs_grid, p[1].runs_grid), kRunThreads,
                                               p[0].runs_lds > p[1].runs_lds ? p[0].runs_lds : p[1].runs_lds, st>>>(rc[0], rc[1]);
  NSAMD_CHECK_LAUNCH();
  scatter_apply_pair_kernel<<<larger(p[0].apply_grid, p[1].apply_grid), p[0].apply_threads,
                              p[0].apply_lds > p[1].apply_lds ? p[0].apply_lds : p[1].apply_lds, st>>>(ac[0], ac[1]);
  NSAMD_CHECK_LAUNCH();
  scatter_finish_pair_kernel<<<dim3(32u, 1u, 2u), 256, 0, st>>>(ac[0], ac[1]);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

int scatter_launch(const ScatterCall* calls, int n, hipStream_t st) {
  NSAMD_REQUIRE(calls != nullptr && (n == 1 || n == 2));
  ScatterPrepared p[2];
  int rc[2];
  for (int i = 0; i < n; ++i) rc[i] = scatter_prepare(calls[i], p[i]);
  if (n == 2 && !rc[0] && !rc[1] && scatter_pair_shares_launches(calls, p)) return scatter_launch_pair(calls, p, st);
  for (int i = 0; i < n; ++i) {
    if (!rc[i]) rc[i] = scatter_launch_one(calls[i], p[i], st);
    if (rc[i]) return rc[i];
  }
  return NSAMD_OK;
}

}  // namespace nsamd
