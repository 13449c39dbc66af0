// The chain layout of the f32 matrix-core kernels (v_mfma_f32_16x16x4_f32), once: field_mlp.hip, normals.hip, linear.hip;
// density_mlp.hip and field_reduce.h take the vector type and the MFMA wrapper. Device code only.
//
// Chain layout. One wavefront owns a tile of 16 sample points. A vector of F features of those points lives in
// registers as X[t][r] (t < F/16, r < 4): lane (j = lane & 15, g = lane >> 4) holds feature 16t + 4g + r of point
// j. With Y^T = W X^T, MFMA step (t, r) takes  A = W[16n + j][16t + 4g + r]  and  B = X[t][r]; the C/D fragment of
// output tile n is then neuron 16n + 4g + r' of point j — the SAME layout, so a layer's accumulators are the
// next layer's B operands with no shuffle or LDS round trip. The K-order permutation this implies is folded into
// the weight fragments when a workgroup stages them in LDS (once; workgroups are persistent over tiles):
//   Wf[n][t][lane][r] = W[16n + j][16t + 4g + r]   -> one conflict-free ds_read_b128 per lane feeds 4 MFMAs.
#pragma once

#include "common.h"

namespace nsamd {

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4f mfma16(float a, float b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// out[n] (+)= sum over input tiles; frag = Wf-style block for this layer: [NT][KT][64][4]
template <int NT, int KT>
__device__ __forceinline__ void chain_gemm(const float* frag, const v4f* in, v4f* out, int lane) {
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    v4f a[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) a[n] = *reinterpret_cast<const v4f*>(frag + ((n * KT + t) * 64 + lane) * 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int n = 0; n < NT; ++n) out[n] = mfma16(a[n][r], in[t][r], out[n]);
    }
  }
}

// one input tile `t` of a [NT][KT] fragment block: out[n] += W[16n + j][16t ..] . in
template <int NT, int KT>
__device__ __forceinline__ void chain_gemm_tile(const float* frag, int t, const v4f& in, v4f* out, int lane) {
  v4f a[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) a[n] = *reinterpret_cast<const v4f*>(frag + ((n * KT + t) * 64 + lane) * 4);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int n = 0; n < NT; ++n) out[n] = mfma16(a[n][r], in[r], out[n]);
  }
}

// out[n] = the lane's four biases of output tile n (neurons 16n + 4g ..)
template <int NT>
__device__ __forceinline__ void load_bias(const float* bias, v4f* out, int g) {
#pragma unroll
  for (int n = 0; n < NT; ++n) out[n] = *reinterpret_cast<const v4f*>(bias + 16 * n + 4 * g);
}

template <int NT>
__device__ __forceinline__ void relu_tiles(v4f* x) {
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) x[n][r] = fmaxf(x[n][r], 0.0f);
}

template <int N>
__device__ __forceinline__ void zero_tiles(v4f* x) {
#pragma unroll
  for (int n = 0; n < N; ++n) x[n] = v4f{0.f, 0.f, 0.f, 0.f};
}

}  // namespace nsamd
