// Host build of nerfstudio_amd/csrc/normals_loss.h for tests/test_normals_loss_cpu.py: the per-sample arithmetic
// nsamd_normals_losses runs per lane, looped over the rays and samples the way the kernel composes it (terms added in double,
// rounded once, then the scale). Test infrastructure: the product never loads it.
#include <cstdint>

#include "../../nerfstudio_amd/csrc/normals_loss.h"

using namespace nsamd;

// weights [n, S], normals / pred_pre / d_pred_pre [n * S, 3], directions / d_directions [n, 3], per-ray terms [n]
extern "C" int hc_normals_losses(const float* weights, const float* normals, const float* pred_pre, const float* directions,
                                 int64_t n, int S, float orientation_scale, float pred_scale, float* orientation_per_ray,
                                 float* pred_per_ray, float* d_pred_pre, float* d_directions) {
  for (int64_t r = 0; r < n; ++r) {
    double so = 0.0, sp = 0.0, sd[3] = {0.0, 0.0, 0.0};
    for (int s = 0; s < S; ++s) {
      const int64_t i = r * S + s;
      float term, dv[3];
      pred_normal_sample(weights[i], normals + 3 * i, pred_pre + 3 * i, pred_scale, &term, d_pred_pre + 3 * i);
      sp += (double)term;
      orientation_sample(weights[i], normals + 3 * i, directions + 3 * r, &term, dv);
      so += (double)term;
      for (int c = 0; c < 3; ++c) sd[c] += (double)dv[c];
    }
    orientation_per_ray[r] = (float)so;
    pred_per_ray[r] = (float)sp;
    for (int c = 0; c < 3; ++c) d_directions[3 * r + c] = orientation_scale * (float)sd[c];
  }
  return 0;
}
