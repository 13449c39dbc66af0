// Internal interface of the proposal-level backward's stages (proposal_chain.hip: nsamd_proposal_levels_bwd, and the per-level
// entry points of sampler.hip and density_mlp.hip). Each `*_launch` takes n = 1 or 2 calls: one call is the per-level launch;
// two calls share ONE launch per kernel where they can, and otherwise run one after the other. The scatter stage is
// scatter.h's scatter_launch, of the same shape. Not part of the C ABI.
// The weights stage has ONE kernel for both cases (two calls as arguments, one slice of the grid per call; one call = one
// slice, the second call zeroed and unread). The density and scatter stages keep a single-call kernel beside their two-call
// kernel around the same body: launched with one slice, the two-call kernels cost the eager per-level entry points about
// 1 us (1 - 3 %) at the benchmark's shapes (profiles/one_kernel_per_stage_ab.txt).
#pragma once

#include "common.h"

namespace nsamd {

// RaySamples.get_weights backward (sampler.hip: weights_bwd_kernel); `gate` (nullable, cleared by the caller) and `ray_mask`
// (nullable) are its zero-gradient outputs
struct WeightsBwdCall {
  const float* t_bins;
  const float* density;
  const float* dweights;
  int64_t num_rays;
  int32_t S;
  float* ddensity;
  uint32_t* gate;
  uint8_t* ray_mask;
};
int weights_bwd_launch(const WeightsBwdCall* calls, int n, hipStream_t stream);

// density MLP backward + the fixed-order reduce of its weight-gradient partials (density_mlp.hip)
struct DensityBwdCall {
  const float* enc;
  const float* selector;
  const float* pre;
  const float* ddensity;
  int64_t M;
  nsamd_density_mlp mlp;
  float* denc;
  float* dW0;
  float* db0;
  float* dW1;
  float* db1;
  float* workspace;
  int64_t workspace_floats;
  const uint32_t* gate;
  const uint8_t* ray_mask;
  int spr;  // samples per ray (read with `ray_mask` only)
};
int density_bwd_launch(const DensityBwdCall* calls, int n, hipStream_t stream);

}  // namespace nsamd
