// Proposal-network losses for gfx950 (reference: /root/reference/nerfstudio/model_components/losses.py —
// outer :53-82, lossfun_outer :85-102, interlevel_loss :113-131, lossfun_distortion :135-146).
//
// Both are per-ray independent with tens to hundreds of samples: one wavefront per ray, rows staged in LDS, value
// and gradient in one pass (the losses are scalars whose upstream gradient is a known constant). The eager
// reference spends ~20 launches and several [N,S,S] temporaries on this; here it is two launches and O(N*S) bytes.
#include "ray_bodies.h"
#include "depth_loss.h"

namespace nsamd {


__global__ __launch_bounds__(kRayThreads) void interlevel_kernel(
    const float* __restrict__ c_in, const float* __restrict__ w_in, int Sf, const float* __restrict__ cp_in,
    const float* __restrict__ wp_in, int Sp, int64_t num_rays, float grad_scale, float* __restrict__ per_ray,
    float* __restrict__ dwp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  interlevel_body(lds + (size_t)wave_index() * interlevel_row_floats(Sf, Sp), c_in, w_in, Sf, cp_in, wp_in, Sp, num_rays,
                  grad_scale, per_ray, dwp);
}

__global__ __launch_bounds__(kRayThreads) void distortion_kernel(const float* __restrict__ s_bins,
                                                                 const float* __restrict__ weights, int S,
                                                                 int64_t num_rays, float grad_scale,
                                                                 float* __restrict__ per_ray,
                                                                 float* __restrict__ dw) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  distortion_body(lds + (size_t)wave_index() * 2 * S, s_bins, weights, S, num_rays, grad_scale, per_ray, dw);
}

// All proposal losses of one training step in one launch: blockIdx.y < levels = interlevel loss of that proposal level,
// blockIdx.y == levels = distortion loss of the fine samples (models/nerfacto.py:367-375).
constexpr int kMaxPropLevels = 4;
struct PropLossArgs {
  const float* s_bins[kMaxPropLevels];
  const float* weights[kMaxPropLevels];
  float* per_ray[kMaxPropLevels];
  float* dw[kMaxPropLevels];
  int S[kMaxPropLevels];
  int levels;
};

__global__ __launch_bounds__(kRayThreads) void proposal_losses_kernel(
    const float* __restrict__ s_fine, const float* __restrict__ w_fine, int Sf, PropLossArgs a, int64_t num_rays,
    float inter_scale, float dist_scale, float* __restrict__ dist_per_ray, float* __restrict__ dw_dist) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int job = blockIdx.y;
  if (job < a.levels) {
    interlevel_body(lds + (size_t)wave_index() * interlevel_row_floats(Sf, a.S[job]), s_fine, w_fine, Sf, a.s_bins[job],
                    a.weights[job], a.S[job], num_rays, inter_scale, a.per_ray[job], a.dw[job]);
  } else {
    distortion_body(lds + (size_t)wave_index() * 2 * Sf, s_fine, w_fine, Sf, num_rays, dist_scale, dist_per_ray, dw_dist);
  }
}

// Depth supervision of depth-nerfacto (models/depth_nerfacto.py:90-104; the arithmetic is depth_loss.h): one wavefront per
// (ray, level), blockIdx.y = level, lanes striding over the level's samples. Each lane adds its terms in sample order in double,
// the lanes meet through the DPP scan of wave.h: a fixed order, so the per-ray value is the same bits run to run. Gradients are
// plain stores; `accumulate` adds them to what the buffer holds (the explicit schedule: behind the proposal losses' own
// gradients) — for a masked ray too, whose `old + 0` is what an addition of the zero gradient gives (-0 becomes +0).
constexpr int kMaxDepthLevels = 8;
constexpr int kMaxDepthSamples = 4096;
struct DepthLossArgs {
  const float* t_bins[kMaxDepthLevels];
  const float* weights[kMaxDepthLevels];
  float* dw[kMaxDepthLevels];
  int S[kMaxDepthLevels];
  int levels;
};

__global__ __launch_bounds__(kRayThreads) void depth_loss_kernel(
    DepthLossArgs a, int64_t num_rays, const float* __restrict__ termination_depth,
    const float* __restrict__ directions_norm, const float* __restrict__ predicted_depth, float sigma, float log_scale,
    int loss_type, float scale, int accumulate, float* __restrict__ per_ray, float* __restrict__ d_predicted) {
  const int lane = threadIdx.x & 63, wave = wave_index();
  const int64_t ray = (int64_t)blockIdx.x * kRaysPerBlock + wave;
  if (ray >= num_rays) return;  // wave-uniform
  const int lvl = blockIdx.y;
  const int S = a.S[lvl];
  const float target = depth_target(termination_depth[ray], directions_norm != nullptr ? directions_norm[ray] : 1.0f,
                                    directions_norm == nullptr);
  const bool supervised = target > 0.0f;  // depth_mask; wave-uniform
  const float* __restrict__ tb = a.t_bins[lvl] + ray * (S + 1);
  const float* __restrict__ w = a.weights[lvl] + ray * S;
  float* __restrict__ dw = a.dw[lvl] != nullptr ? a.dw[lvl] + ray * S : nullptr;
  const bool urf = loss_type == kDepthLossUrf;
  double sum0 = 0.0, sum1 = 0.0;  // DS_NERF: the terms; URF: the near and the empty terms
  for (int i = lane; i < S; i += 64) {
    float g = 0.0f;
    if (supervised) {
      float t0 = 0.0f, t1 = 0.0f, d = 0.0f;
      if (urf) urf_sample(tb[i], tb[i + 1], w[i], target, sigma, log_scale, &t0, &t1, &d);
      else ds_nerf_sample(tb[i], tb[i + 1], w[i], target, sigma, &t0, &d);
      sum0 += (double)t0;
      sum1 += (double)t1;
      g = d * scale;
    }
    if (dw != nullptr) dw[i] = accumulate ? dw[i] + g : g;
  }
  // (every lane is back here: the DPP moves need the whole wave)
  const float tot0 = (float)wave_read_f64<63>(wave_scan_inclusive_f64(sum0));
  const float tot1 = urf ? (float)wave_read_f64<63>(wave_scan_inclusive_f64(sum1)) : 0.0f;  // (wave-uniform branch)
  if (lane != 0) return;
  float loss = tot0, dpred = 0.0f;
  if (urf) {
    float expected = 0.0f;
    urf_ray(target, predicted_depth[ray], &expected, &dpred);
    loss = expected + (tot0 + tot1);  // expected_depth_loss + (near + empty), losses.py:283-285
  }
  if (per_ray != nullptr) per_ray[(int64_t)lvl * num_rays + ray] = supervised ? loss : 0.0f;
  if (urf && lvl == 0 && d_predicted != nullptr) {
    // every level's call of the reference adds the same term to predicted_depth's gradient: the sum of `levels` equal summands
    const float g = supervised ? dpred * scale : 0.0f;
    float total = 0.0f;
    for (int l = 0; l < a.levels; ++l) total += g;
    d_predicted[ray] = accumulate ? d_predicted[ray] + total : total;
  }
}

}  // namespace nsamd

using namespace nsamd;

extern "C" int nsamd_proposal_losses(const float* s_bins_fine, const float* w_fine, int32_t S_fine, int32_t levels,
                                     const float* const* s_bins_prop, const float* const* w_prop,
                                     const int32_t* S_prop, int64_t num_rays, float interlevel_grad_scale,
                                     float distortion_grad_scale, float* const* interlevel_per_ray,
                                     float* const* dw_prop, float* distortion_per_ray, float* dw_distortion,
                                     nsamd_stream_t stream) {
  NSAMD_REQUIRE(num_rays >= 0 && S_fine > 0 && levels >= 0 && levels <= kMaxPropLevels);
  if (num_rays == 0) return NSAMD_OK;
  NSAMD_REQUIRE(s_bins_fine && w_fine && distortion_per_ray);
  NSAMD_REQUIRE(levels == 0 || (s_bins_prop && w_prop && S_prop && interlevel_per_ray));
  if (S_fine > 2048) return NSAMD_ERR_UNSUPPORTED;
  PropLossArgs a{};
  a.levels = levels;
  size_t lds = sizeof(float) * 2 * S_fine * kRaysPerBlock;
  for (int i = 0; i < levels; ++i) {
    NSAMD_REQUIRE(s_bins_prop[i] && w_prop[i] && interlevel_per_ray[i] && S_prop[i] > 0);
    a.s_bins[i] = s_bins_prop[i];
    a.weights[i] = w_prop[i];
    a.per_ray[i] = interlevel_per_ray[i];
    a.dw[i] = dw_prop ? dw_prop[i] : nullptr;
    a.S[i] = S_prop[i];
    const size_t per_wave =
        sizeof(float) * ((2 * (S_fine + 2) + 2 * (S_prop[i] + 1) + (S_fine + 1) + 4 * S_fine + 1) & ~1);
    if (per_wave * kRaysPerBlock > lds) lds = per_wave * kRaysPerBlock;
  }
  if (lds > 64 * 1024) return NSAMD_ERR_UNSUPPORTED;
  dim3 g((unsigned)((num_rays + kRaysPerBlock - 1) / kRaysPerBlock), (unsigned)(levels + 1));
  proposal_losses_kernel<<<g, kRayThreads, lds, (hipStream_t)stream>>>(
      s_bins_fine, w_fine, S_fine, a, num_rays, interlevel_grad_scale, distortion_grad_scale, distortion_per_ray,
      dw_distortion);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int nsamd_interlevel_loss(const float* s_bins_fine, const float* w_fine, int32_t S_fine,
                                     const float* s_bins_prop, const float* w_prop, int32_t S_prop,
                                     int64_t num_rays, float grad_scale, float* per_ray_loss, float* dw_prop,
                                     nsamd_stream_t stream) {
  NSAMD_REQUIRE(num_rays >= 0 && S_fine > 0 && S_prop > 0);
  if (num_rays == 0) return NSAMD_OK;
  NSAMD_REQUIRE(s_bins_fine && w_fine && s_bins_prop && w_prop && per_ray_loss);
  const size_t per_wave = sizeof(float) * ((2 * (S_fine + 2) + 2 * (S_prop + 1) + (S_fine + 1) + 4 * S_fine + 1) & ~1);
  if (per_wave * kRaysPerBlock > 64 * 1024) return NSAMD_ERR_UNSUPPORTED;
  const unsigned blocks = (unsigned)((num_rays + kRaysPerBlock - 1) / kRaysPerBlock);
  interlevel_kernel<<<blocks, kRayThreads, per_wave * kRaysPerBlock, (hipStream_t)stream>>>(
      s_bins_fine, w_fine, S_fine, s_bins_prop, w_prop, S_prop, num_rays, grad_scale, per_ray_loss, dw_prop);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int nsamd_distortion_loss(const float* s_bins, const float* weights, int32_t S, int64_t num_rays,
                                     float grad_scale, float* per_ray_loss, float* dweights,
                                     nsamd_stream_t stream) {
  NSAMD_REQUIRE(num_rays >= 0 && S > 0);
  if (num_rays == 0) return NSAMD_OK;
  NSAMD_REQUIRE(s_bins && weights && per_ray_loss);
  if (S > 2048) return NSAMD_ERR_UNSUPPORTED;
  const unsigned blocks = (unsigned)((num_rays + kRaysPerBlock - 1) / kRaysPerBlock);
  distortion_kernel<<<blocks, kRayThreads, sizeof(float) * 2 * S * kRaysPerBlock, (hipStream_t)stream>>>(
      s_bins, weights, S, num_rays, grad_scale, per_ray_loss, dweights);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int nsamd_depth_loss(int32_t levels, const float* const* t_bins, const float* const* weights, const int32_t* S,
                                int64_t num_rays, const float* termination_depth, const float* directions_norm,
                                const float* predicted_depth, float sigma, int32_t loss_type, float scale,
                                int32_t accumulate, float* per_ray, float* const* d_weights, float* d_predicted,
                                nsamd_stream_t stream) {
  NSAMD_REQUIRE(num_rays >= 0 && levels >= 1 && t_bins && weights && S);
  if (!depth_loss_type_supported(loss_type) || levels > kMaxDepthLevels) return NSAMD_ERR_UNSUPPORTED;
  for (int i = 0; i < levels; ++i)
    if (S[i] < 1 || S[i] > kMaxDepthSamples) return NSAMD_ERR_UNSUPPORTED;
  if (num_rays > (int64_t)kRaysPerBlock * 0x7fffffff) return NSAMD_ERR_UNSUPPORTED;
  if (num_rays == 0) return NSAMD_OK;
  NSAMD_REQUIRE(termination_depth && (loss_type != kDepthLossUrf || predicted_depth));
  DepthLossArgs a{};
  a.levels = levels;
  for (int i = 0; i < levels; ++i) {
    NSAMD_REQUIRE(t_bins[i] && weights[i]);
    a.t_bins[i] = t_bins[i];
    a.weights[i] = weights[i];
    a.dw[i] = d_weights ? d_weights[i] : nullptr;
    a.S[i] = S[i];
  }
  const float log_scale = loss_type == kDepthLossUrf ? urf_log_scale(sigma) : 0.0f;  // host, once per launch
  dim3 g((unsigned)((num_rays + kRaysPerBlock - 1) / kRaysPerBlock), (unsigned)levels);
  depth_loss_kernel<<<g, kRayThreads, 0, (hipStream_t)stream>>>(a, num_rays, termination_depth, directions_norm,
                                                                predicted_depth, sigma, log_scale, loss_type, scale, accumulate,
                                                                per_ray, d_predicted);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}
