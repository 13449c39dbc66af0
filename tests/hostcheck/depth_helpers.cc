// Host build of nerfstudio_amd/csrc/depth_loss.h for tests/test_depth_cpu.py: the per-sample arithmetic nsamd_depth_loss runs per
// lane, looped over one level's rays and samples the way the kernel composes it (terms added in double, rounded once; masked
// rays exactly 0). Test infrastructure: the product never loads it.
#include "../../nerfstudio_amd/csrc/depth_loss.h"

using namespace nsamd;

// One level: per_ray [n], dw [n, S] = d term / d w * scale, dpred [n] = one level's share of predicted_depth's gradient * scale
// (URF; nullable). dn: null for a Euclidean depth.
extern "C" int hc_depth_level(const float* t_bins, const float* w, int S, int64_t n, const float* td, const float* dn,
                              const float* pred, float sigma, int loss_type, float scale, float* per_ray, float* dw,
                              float* dpred) {
  if (!depth_loss_type_supported(loss_type)) return -2;
  const float log_scale = loss_type == kDepthLossUrf ? urf_log_scale(sigma) : 0.0f;
  for (int64_t r = 0; r < n; ++r) {
    const float target = depth_target(td[r], dn ? dn[r] : 1.0f, dn == nullptr);
    const bool supervised = target > 0.0f;
    const float* tb = t_bins + r * (S + 1);
    double sum0 = 0.0, sum1 = 0.0;
    for (int i = 0; i < S; ++i) {
      float t0 = 0.0f, t1 = 0.0f, d = 0.0f, g = 0.0f;
      if (supervised) {
        if (loss_type == kDepthLossUrf) urf_sample(tb[i], tb[i + 1], w[r * S + i], target, sigma, log_scale, &t0, &t1, &d);
        else ds_nerf_sample(tb[i], tb[i + 1], w[r * S + i], target, sigma, &t0, &d);
        sum0 += (double)t0;
        sum1 += (double)t1;
        g = d * scale;
      }
      dw[r * S + i] = g;
    }
    float loss = (float)sum0, dp = 0.0f;
    if (loss_type == kDepthLossUrf) {
      float expected = 0.0f;
      urf_ray(target, pred[r], &expected, &dp);
      loss = expected + ((float)sum0 + (float)sum1);
    }
    per_ray[r] = supervised ? loss : 0.0f;
    if (dpred) dpred[r] = supervised ? dp * scale : 0.0f;
  }
  return 0;
}
