// Normals of the nerfacto field in the eval render, forward only (reference: Field.get_normals, fields/base_field.py:79-99;
// NerfactoField.get_density :203-229 and get_outputs :287-295; PredNormalsFieldHead, field_components/field_heads.py;
// NormalsRenderer / NormalsShader, model_components/renderers.py, shaders.py; call site models/nerfacto.py:325-329).
//
// nsamd_field_normals. The analytic normal of a sample is minus the normalised gradient of the density PRE-activation with
// respect to the normalised, selector-masked position. The reference gets it from a second pass through autograd; here it is one
// kernel behind the chunk's hash forward, which left the encoded features `enc` [32, M] in the schedule's buffer:
//   z = W0 enc + b0,  h = relu(z),  geo = W1[1:16] h + b1[1:16]           (the base MLP again: 3 072 MACs per sample)
//   g_enc = W0^T (W1[0, :] * [z > 0])                                      (data gradient of the pre-activation: 2 048 MACs)
//   g = sum_l scalings[l] sum_f g_enc[l, f] d blend_l,f / d offset         (position gradient of HashEncoding.pytorch_fwd)
// The three products run on v_mfma_f32_16x16x4_f32 in the chain layout of field_mlp.hip: one wavefront owns 16 samples, lane
// (j = lane & 15, g = lane >> 4) holds feature 16 t + 4 g + r of sample j, a layer's accumulators are the next layer's B
// operands. That layout also splits the gather work with no lane movement: the lane's eight g_enc values ARE levels 2 g, 2 g + 1,
// 8 + 2 g, 9 + 2 g of its sample, so every lane gathers and differentiates four levels of one sample (32 8-B corner fetches in
// flight — the rows the forward just touched), and the four partial gradients of a sample meet in a fixed two-step butterfly.
// Weights are staged once per workgroup in LDS as MFMA fragments; workgroups are persistent over tiles. No atomics.
// Edge cases as the reference has them: where ceil == floor on an axis both corners of that axis are the same table row, their
// difference — that axis' share on the level — is exactly 0; a masked-out sample sits at hash(0, 0, 0) on every level: g = 0,
// normal = -0 / max(0, 1e-12) = 0.
// What bounds it: the gathers. 1 024 B of corner fetches per sample against 128 B of features and 72 B of results, the address
// unit's ~0.47 lines per clock and CU (hashgrid.hip); the 5 120 MACs per sample are 10 MFMAs per tile beside 32 gathers per lane.
//
// nsamd_normals_composite. One wavefront per ray: pred = normalize(tanh(x)) per sample, the weighted sums of both normal
// channels (double partial sums, the DPP scan of wave.h: a fixed order), r = s / (|s| + 1e-10), shaded (r + 1) / 2.
//
// nsamd_normals_losses. The two training losses on those normals with their gradients (normals_loss.h), one wavefront per ray
// as the composite: lane l takes samples l, l + 64, ..., writes their pre-activation gradients, and the ray's two loss terms and
// its view-direction gradient are double partial sums through the same scan. No atomics, the same bits on every run.
#include "common.h"
#include "launch.h"
#include "mfma_chain.h"
#include "normals_loss.h"
#include "wave.h"

namespace nsamd {

constexpr int kNrmWaves = 4;
constexpr int kNrmThreads = 64 * kNrmWaves;
constexpr int kNrmMaxBlocks = 1024;
// LDS image (floats): MFMA fragments frag[n][t][lane][r], then the vectors
constexpr int kNrmW0 = 0;                  // [4][2][64][4]  W0[16n + j][16t + 4g + r]          z = W0 enc
constexpr int kNrmW1 = kNrmW0 + 2048;      // [1][4][64][4]  W1[j][16t + 4g + r]                o16 = W1 h
constexpr int kNrmW0T = kNrmW1 + 1024;     // [2][4][64][4]  W0[16t + 4g + r][16n + j]          g_enc = W0^T s
constexpr int kNrmB0 = kNrmW0T + 2048;     // [64]
constexpr int kNrmB1 = kNrmB0 + 64;        // [16]
constexpr int kNrmW1Row0 = kNrmB1 + 16;    // [64]  W1[0, :]
constexpr int kNrmScale = kNrmW1Row0 + 64; // [16]  grid.scalings
constexpr int kNrmLds = kNrmScale + 16;

__global__ __launch_bounds__(kNrmThreads, 2) void field_normals_kernel(
    nsamd_points P, int64_t M, int transform, nsamd_aabb box, const float2* __restrict__ table, nsamd_grid grid,
    const float* __restrict__ enc, const float* __restrict__ W0, const float* __restrict__ b0, const float* __restrict__ W1,
    const float* __restrict__ b1, float* __restrict__ normals, float* __restrict__ gradient, float* __restrict__ geo,
    int64_t geo_stride, int64_t geo_offset) {
  __shared__ __attribute__((aligned(16))) float lds[kNrmLds];
  for (int e = threadIdx.x; e < 2048; e += kNrmThreads) {
    const int r = e & 3, l = (e >> 2) & 63, tile = e >> 8;
    const int j = l & 15, g = l >> 4;
    {  // [4][2]
      const int t = tile & 1, n = tile >> 1;
      lds[kNrmW0 + e] = W0[(16 * n + j) * 32 + 16 * t + 4 * g + r];
    }
    {  // [2][4]
      const int t = tile & 3, n = tile >> 2;
      lds[kNrmW0T + e] = W0[(16 * t + 4 * g + r) * 32 + 16 * n + j];
    }
    if (e < 1024) lds[kNrmW1 + e] = W1[j * 64 + 16 * tile + 4 * g + r];  // [1][4]: tile = t
  }
  if (threadIdx.x < 64) {
    lds[kNrmB0 + threadIdx.x] = b0[threadIdx.x];
    lds[kNrmW1Row0 + threadIdx.x] = W1[threadIdx.x];
  } else if (threadIdx.x < 80) {
    lds[kNrmB1 + threadIdx.x - 64] = b1[threadIdx.x - 64];
  } else if (threadIdx.x < 96) {
    lds[kNrmScale + threadIdx.x - 80] = grid.scalings[threadIdx.x - 80];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const uint32_t mask = (1u << grid.log2_table_size) - 1u;
  const int64_t tiles = (M + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * kNrmWaves + wave; tile < tiles; tile += (int64_t)gridDim.x * kNrmWaves) {
    asm volatile("" ::: "memory");  // (the fragments are loop-invariant LDS data: keep them out of registers, field_mlp.hip)
    const int64_t p_raw = tile * 16 + j;
    const bool live = p_raw < M;
    const int64_t p = live ? p_raw : M - 1;
    v4f x[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[t][r] = enc[(int64_t)(16 * t + 4 * g + r) * M + p];
    float px, py, pz;
    load_position(P, p, px, py, pz);
    (void)normalise_position(transform, box, px, py, pz);
    // the lane's four levels: 8 t + 2 g + q — gathers in flight before the matrix work
    float2 v[4][8];
    float w[4][3], scale[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int level = 8 * (i >> 1) + 2 * g + (i & 1);
      scale[i] = lds[kNrmScale + level];
      const Cell c = locate_cell(px, py, pz, scale[i]);
      w[i][0] = c.w[0]; w[i][1] = c.w[1]; w[i][2] = c.w[2];
      const float2* __restrict__ tl = table + ((size_t)level << grid.log2_table_size);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[i][k] = tl[corner_index(c, k, mask)];
    }
    v4f z[4], s[4], o16[1], ge[2];
    load_bias<4>(lds + kNrmB0, z, g);
    chain_gemm<4, 2>(lds + kNrmW0, x, z, lane);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const v4f w1 = *reinterpret_cast<const v4f*>(lds + kNrmW1Row0 + 16 * n + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[n][r] = z[n][r] > 0.0f ? w1[r] : 0.0f;
        z[n][r] = fmaxf(z[n][r], 0.0f);
      }
    }
    load_bias<1>(lds + kNrmB1, o16, g);
    chain_gemm<1, 4>(lds + kNrmW1, z, o16, lane);
    zero_tiles<2>(ge);
    chain_gemm<2, 4>(lds + kNrmW0T, s, ge, lane);
    if (geo != nullptr && live) {  // neuron 4 g + r of the base output; neuron 0 is the density pre-activation
      float* o = geo + p * geo_stride + geo_offset + (4 * g - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * g + r > 0) o[r] = o16[0][r];
    }
    // position gradient of the lane's four levels (trilinear_blend_grad: the derivative of the x -> y -> z blend)
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float lx = 0.0f, ly = 0.0f, lz = 0.0f;
#pragma unroll
      for (int f = 0; f < 2; ++f)
        trilinear_blend_grad([&](int k) { return f == 0 ? v[i][k].x : v[i][k].y; }, ge[i >> 1][2 * (i & 1) + f], w[i][0],
                             w[i][1], w[i][2], lx, ly, lz);
      gx += lx * scale[i];
      gy += ly * scale[i];
      gz += lz * scale[i];
    }
    // the sample's four lanes (g = 0 .. 3): (g0 + g1) + (g2 + g3) in every one of them
    gx += __shfl_xor(gx, 16); gy += __shfl_xor(gy, 16); gz += __shfl_xor(gz, 16);
    gx += __shfl_xor(gx, 32); gy += __shfl_xor(gy, 32); gz += __shfl_xor(gz, 32);
    if (g == 0 && live) {
      if (gradient != nullptr) {
        gradient[3 * p + 0] = gx;
        gradient[3 * p + 1] = gy;
        gradient[3 * p + 2] = gz;
      }
      if (normals != nullptr) {  // -F.normalize(g): g / max(|g|, 1e-12)
        const float nrm = fmaxf(sqrtf((gx * gx + gy * gy) + gz * gz), 1e-12f);
        normals[3 * p + 0] = -(gx / nrm);
        normals[3 * p + 1] = -(gy / nrm);
        normals[3 * p + 2] = -(gz / nrm);
      }
    }
  }
}

constexpr int kNrmRays = 4;  // rays (wavefronts) per workgroup of the composite

__global__ __launch_bounds__(64 * kNrmRays) void normals_composite_kernel(
    const float* __restrict__ weights, const float* __restrict__ normals, const float* __restrict__ pred_pre, int64_t num_rays,
    int S, float* __restrict__ normals_out, float* __restrict__ pred_out) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * kNrmRays + wave_index();
  if (ray >= num_rays) return;  // (wave-uniform)
  double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
  for (int smp = lane; smp < S; smp += 64) {
    const int64_t i = ray * S + smp;
    const float w = weights[i];
    if (normals != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a[c] += (double)(w * normals[3 * i + c]);
    }
    if (pred_pre != nullptr) {  // PredNormalsFieldHead: normalize(tanh(x))
      const float t0 = tanhf(pred_pre[3 * i]), t1 = tanhf(pred_pre[3 * i + 1]), t2 = tanhf(pred_pre[3 * i + 2]);
      const float nrm = fmaxf(sqrtf((t0 * t0 + t1 * t1) + t2 * t2), 1e-12f);
      b[0] += (double)(w * (t0 / nrm));
      b[1] += (double)(w * (t1 / nrm));
      b[2] += (double)(w * (t2 / nrm));
    }
  }
  float sa[3], sb[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sa[c] = (float)wave_read_f64<63>(wave_scan_inclusive_f64(a[c]));
    sb[c] = (float)wave_read_f64<63>(wave_scan_inclusive_f64(b[c]));
  }
  if (lane == 0) {  // NormalsRenderer: n / (|n| + 1e-10); NormalsShader: (n + 1) / 2
    if (normals_out != nullptr) {
      const float nrm = sqrtf((sa[0] * sa[0] + sa[1] * sa[1]) + sa[2] * sa[2]) + 1e-10f;
#pragma unroll
      for (int c = 0; c < 3; ++c) normals_out[3 * ray + c] = (sa[c] / nrm + 1.0f) / 2.0f;
    }
    if (pred_out != nullptr) {
      const float nrm = sqrtf((sb[0] * sb[0] + sb[1] * sb[1]) + sb[2] * sb[2]) + 1e-10f;
#pragma unroll
      for (int c = 0; c < 3; ++c) pred_out[3 * ray + c] = (sb[c] / nrm + 1.0f) / 2.0f;
    }
  }
}

__global__ __launch_bounds__(64 * kNrmRays) void normals_losses_kernel(
    const float* __restrict__ weights, const float* __restrict__ normals, const float* __restrict__ pred_pre,
    const float* __restrict__ directions, int64_t num_rays, int S, float orientation_scale, float pred_scale,
    float* __restrict__ orientation_per_ray, float* __restrict__ pred_per_ray, float* __restrict__ d_pred_pre,
    float* __restrict__ d_directions, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * kNrmRays + wave_index();
  if (ray >= num_rays) return;  // (wave-uniform)
  float v[3] = {0.0f, 0.0f, 0.0f};
  if (directions != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = directions[3 * ray + c];
  }
  double so = 0.0, sp = 0.0, sd[3] = {0.0, 0.0, 0.0};
  for (int smp = lane; smp < S; smp += 64) {
    const int64_t i = ray * S + smp;
    const float w = weights[i];
    const float n[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    if (pred_pre != nullptr) {
      const float x[3] = {pred_pre[3 * i], pred_pre[3 * i + 1], pred_pre[3 * i + 2]};
      float term, dx[3];
      pred_normal_sample(w, n, x, pred_scale, &term, d_pred_pre != nullptr ? dx : nullptr);
      sp += (double)term;
      if (d_pred_pre != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d_pred_pre[3 * i + c] = dx[c];
      }
    }
    if (directions != nullptr) {
      float term, dv[3];
      orientation_sample(w, n, v, &term, dv);
      so += (double)term;
#pragma unroll
      for (int c = 0; c < 3; ++c) sd[c] += (double)dv[c];
    }
  }
  const float to = (float)wave_read_f64<63>(wave_scan_inclusive_f64(so));
  const float tp = (float)wave_read_f64<63>(wave_scan_inclusive_f64(sp));
  float td[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) td[c] = (float)wave_read_f64<63>(wave_scan_inclusive_f64(sd[c]));
  if (lane == 0) {
    if (orientation_per_ray != nullptr) orientation_per_ray[ray] = to;
    if (pred_per_ray != nullptr) pred_per_ray[ray] = tp;
    if (d_directions != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float g = orientation_scale * td[c];
        d_directions[3 * ray + c] = accumulate ? d_directions[3 * ray + c] + g : g;
      }
    }
  }
}

}  // namespace nsamd

using namespace nsamd;

extern "C" int nsamd_field_normals(nsamd_points pts, int64_t M, int transform, nsamd_aabb aabb, const float* table,
                                   nsamd_grid grid, const float* enc, const float* base_W0, const float* base_b0,
                                   const float* base_W1, const float* base_b1, float* normals, float* gradient, float* geo,
                                   int64_t geo_stride, int64_t geo_offset, nsamd_stream_t stream) {
  NSAMD_REQUIRE(M >= 0);
  if (grid.num_levels != 16 || check_grid(grid) != NSAMD_OK) return NSAMD_ERR_UNSUPPORTED;  // 32 features = the K of layer 0
  if (M > ((int64_t)1 << 31)) return NSAMD_ERR_UNSUPPORTED;
  if (M == 0) return NSAMD_OK;
  if (const int st = check_points(pts, M)) return st;
  NSAMD_REQUIRE(transform >= 0 && transform <= 2);
  NSAMD_REQUIRE(table != nullptr && enc != nullptr && base_W0 != nullptr && base_b0 != nullptr && base_W1 != nullptr &&
                base_b1 != nullptr);
  NSAMD_REQUIRE(geo == nullptr || (geo_offset >= 0 && geo_stride >= geo_offset + 15));
  if (normals == nullptr && gradient == nullptr && geo == nullptr) return NSAMD_OK;
  const int64_t tiles = (M + 15) / 16;
  const int64_t want = (tiles + kNrmWaves - 1) / kNrmWaves;
  const unsigned blocks = (unsigned)(want < kNrmMaxBlocks ? want : kNrmMaxBlocks);
  field_normals_kernel<<<blocks, kNrmThreads, 0, (hipStream_t)stream>>>(
      pts, M, transform, aabb, reinterpret_cast<const float2*>(table), grid, enc, base_W0, base_b0, base_W1, base_b1, normals,
      gradient, geo, geo_stride, geo_offset);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int nsamd_normals_composite(const float* weights, const float* normals, const float* pred_pre, int64_t num_rays,
                                       int32_t S, float* normals_out, float* pred_out, nsamd_stream_t stream) {
  NSAMD_REQUIRE(num_rays >= 0 && S > 0);
  if (S > 4096) return NSAMD_ERR_UNSUPPORTED;
  unsigned blocks;
  if (grid_blocks((num_rays + kNrmRays - 1) / kNrmRays, &blocks)) return NSAMD_ERR_UNSUPPORTED;
  if (num_rays == 0) return NSAMD_OK;
  NSAMD_REQUIRE(weights != nullptr);
  NSAMD_REQUIRE((normals_out == nullptr || normals != nullptr) && (pred_out == nullptr || pred_pre != nullptr));
  if (normals_out == nullptr && pred_out == nullptr) return NSAMD_OK;
  normals_composite_kernel<<<blocks, 64 * kNrmRays, 0, (hipStream_t)stream>>>(
      weights, normals_out ? normals : nullptr, pred_out ? pred_pre : nullptr, num_rays, S, normals_out, pred_out);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int nsamd_normals_losses(const float* weights, const float* normals, const float* pred_pre, const float* directions,
                                    int64_t num_rays, int32_t S, float orientation_scale, float pred_scale,
                                    float* orientation_per_ray, float* pred_per_ray, float* d_pred_pre, float* d_directions,
                                    int32_t accumulate_directions, nsamd_stream_t stream) {
  NSAMD_REQUIRE(num_rays >= 0);
  if (S < 1 || S > 4096) return NSAMD_ERR_UNSUPPORTED;
  unsigned blocks;
  if (grid_blocks((num_rays + kNrmRays - 1) / kNrmRays, &blocks)) return NSAMD_ERR_UNSUPPORTED;
  if (num_rays == 0) return NSAMD_OK;
  const bool want_pred = pred_per_ray != nullptr || d_pred_pre != nullptr;
  const bool want_orientation = orientation_per_ray != nullptr || d_directions != nullptr;
  if (!want_pred && !want_orientation) return NSAMD_OK;
  NSAMD_REQUIRE(weights != nullptr && normals != nullptr);
  NSAMD_REQUIRE((!want_pred || pred_pre != nullptr) && (!want_orientation || directions != nullptr));
  normals_losses_kernel<<<blocks, 64 * kNrmRays, 0, (hipStream_t)stream>>>(
      weights, normals, want_pred ? pred_pre : nullptr, want_orientation ? directions : nullptr, num_rays, S, orientation_scale,
      pred_scale, orientation_per_ray, pred_per_ray, d_pred_pre, d_directions, accumulate_directions ? 1 : 0);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}
