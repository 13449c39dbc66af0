// Per-sample arithmetic of the two normals losses of a `predict_normals` nerfacto model and their gradients (gfx950; the host
// compiler sees it only through tests/hostcheck). Reference: nerfstudio/model_components/losses.py — orientation_loss :201-213,
// pred_normal_loss :216-222 —, PredNormalsFieldHead (field_components/field_heads.py: tanh, then torch.nn.functional.normalize)
// and the call site models/nerfacto.py:335-344: weights and analytic normals are detached, so the predicted-normal term has
// gradient only through the head's pre-activation and the orientation term only through the view direction. fp32 with the
// reference's operations in the reference's order; the library is built with -ffp-contract=off.
#pragma once

#include "common.h"

namespace nsamd {

constexpr float kNormalizeEps = 1.0e-12f;  // torch.nn.functional.normalize's eps

// (a . b) as torch sums a three-wide last dimension: (a0 b0 + a1 b1) + a2 b2
NSAMD_HD float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Predicted normal p = normalize(tanh(x)) of the head's pre-activation x, its loss term w (1 - n . p) (losses.py:216-222) and,
// unless dx is null, dx = scale * d term / d x: with g_p = -w n, normalize's backward g_t = (g_p - p (p . g_p)) / q where the
// norm was not clamped (|t| >= eps) and g_p / eps where it was — what autograd gives —, then tanh's, g_t (1 - t^2).
NSAMD_HD void pred_normal_sample(float w, const float* n, const float* x, float scale, float* term, float* dx) {
  float t[3], p[3], gp[3];
  for (int c = 0; c < 3; ++c) t[c] = tanhf(x[c]);
  const float nrm = sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  const float q = fmaxf(nrm, kNormalizeEps);
  for (int c = 0; c < 3; ++c) p[c] = t[c] / q;
  *term = w * (1.0f - dot3(n, p));
  if (dx == nullptr) return;
  for (int c = 0; c < 3; ++c) gp[c] = -(w * n[c]);
  const bool clamped = !(nrm >= kNormalizeEps);
  const float along = clamped ? 0.0f : dot3(p, gp);
  for (int c = 0; c < 3; ++c) {
    const float gt = clamped ? gp[c] / kNormalizeEps : (gp[c] - p[c] * along) / q;
    dx[c] = scale * (gt * (1.0f - t[c] * t[c]));
  }
}

// Orientation term w min(0, n . (-v))^2 of a sample under the ray's view direction v (losses.py:201-213; torch.fmin: a NaN
// product counts as 0) and dv = d term / d v = 2 w m (-n), unscaled (the caller sums it over the ray first).
NSAMD_HD void orientation_sample(float w, const float* n, const float* v, float* term, float* dv) {
  const float c = -dot3(n, v);
  const float m = fminf(0.0f, c);
  *term = w * (m * m);
  const float k = (2.0f * w) * m;
  for (int i = 0; i < 3; ++i) dv[i] = k * -n[i];
}

}  // namespace nsamd
