// Per-sample arithmetic of the depth-supervision losses of depth-nerfacto (gfx950; the host compiler sees it only through
// tests/hostcheck). Reference: nerfstudio/model_components/losses.py — ds_nerf_depth_loss :225-247,
// urban_radiance_field_depth_loss :250-286, depth_loss :289-325 — and torch.distributions.Normal.log_prob. fp32 with the
// reference's operations in the reference's order; the library is built with -ffp-contract=off.
#pragma once

#include "common.h"

namespace nsamd {

constexpr int kDepthLossDsNerf = 1;  // DepthLossType.DS_NERF (losses.py:41-46)
constexpr int kDepthLossUrf = 2;     // DepthLossType.URF
constexpr float kDepthEps = 1.0e-7f;           // losses.py:35
constexpr float kUrfSigmaScaleFactor = 3.0f;   // losses.py:38
constexpr float kLogSqrt2Pi = 0.9189385332046727f;  // math.log(math.sqrt(2 * math.pi)), Normal.log_prob

NSAMD_HD bool depth_loss_type_supported(int type) { return type == kDepthLossDsNerf || type == kDepthLossUrf; }

// The ray's target (losses.py:314-315): z-depth times the norm of the ray's direction in the camera frame, unless the depth
// already is a Euclidean distance. The ray is supervised where target > 0 (depth_mask, :243 / :268).
NSAMD_HD float depth_target(float termination_depth, float directions_norm, bool is_euclidean) {
  return is_euclidean ? termination_depth : termination_depth * directions_norm;
}

// DS-NeRF (losses.py:245): term = -log(w + EPS) * exp(-(steps - target)^2 / (2 * sigma)) * len — `2 * sigma`, not
// `2 * sigma^2`, as the reference has it — and d term / d w = -exp(...) * len / (w + EPS).
NSAMD_HD void ds_nerf_sample(float t0, float t1, float w, float target, float sigma, float* term, float* dw) {
  const float steps = (t0 + t1) / 2.0f;  // (starts + ends) / 2, :316
  const float len = t1 - t0;             // ends - starts, :319
  const float d = steps - target;
  const float e = expf(-(d * d) / (2.0f * sigma));
  const float u = w + kDepthEps;
  *term = (-logf(u) * e) * len;
  *dw = -(e * len) / u;
}

// log(scale) of the Normal of the URF near term, scale = sigma / 3 in fp32 as the reference divides. It is the same number for
// every sample of a launch, so it is taken once — in double, rounded once — instead of once per sample by logf, whose last bit,
// times every density of the launch, is a systematic 2e-7 of the whole loss (profiles/depth_loss_float64_ratios.txt).
NSAMD_HD float urf_log_scale(float sigma) { return (float)log((double)(sigma / kUrfSigmaScaleFactor)); }

// Urban Radiance Fields line-of-sight terms (losses.py:274-283): near = (w - N(steps - target; 0, sigma / 3))^2 where
// target - sigma <= steps <= target + sigma, empty = w^2 where steps < target - sigma; the density as exp(log_prob), log_prob
// composed as Normal.log_prob does: -(x^2) / (2 var) - log(scale) - log(sqrt(2 pi)), log_scale = urf_log_scale(sigma).
// d(near + empty) / d w.
NSAMD_HD void urf_sample(float t0, float t1, float w, float target, float sigma, float log_scale, float* near_term,
                         float* empty_term, float* dw) {
  const float steps = (t0 + t1) / 2.0f;
  const float x = steps - target;
  const float s = sigma / kUrfSigmaScaleFactor;
  const float var = s * s;
  const float log_prob = (-(x * x) / (2.0f * var) - log_scale) - kLogSqrt2Pi;
  const float pdf = expf(log_prob);
  const bool in_near = (steps <= target + sigma) && (steps >= target - sigma);
  const bool in_empty = steps < target - sigma;
  const float r = w - pdf;
  *near_term = in_near ? r * r : 0.0f;
  *empty_term = in_empty ? w * w : 0.0f;
  *dw = (in_near ? 2.0f * r : 0.0f) + (in_empty ? 2.0f * w : 0.0f);
}

// Expected-depth term of URF, once per ray and level (losses.py:271): (target - predicted)^2, derivative in `predicted`.
NSAMD_HD void urf_ray(float target, float predicted, float* term, float* dpredicted) {
  const float d = target - predicted;
  *term = d * d;
  *dpredicted = -(2.0f * d);
}

}  // namespace nsamd
