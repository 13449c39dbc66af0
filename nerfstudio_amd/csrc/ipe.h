// Per-sample arithmetic of mip-NeRF's integrated positional encoding (gfx950; the host compiler sees it only through
// tests/hostcheck). Reference: nerfstudio/cameras/rays.py:73-90 (Frustums.get_gaussian_blob), utils/math.py:42-67
// (compute_3d_gaussian), :95-121 (conical_frustum_to_gaussian), :124-134 (expected_sin) and
// field_components/encodings.py:162-186 (NeRFEncoding.pytorch_fwd with covariances). fp32 with the reference's operations in
// the reference's order; the library is built with -ffp-contract=off.
#pragma once

#include "common.h"

namespace nsamd {

constexpr int kIpeMaxFrequencies = 64;  // what the kernel keeps of `freqs` in LDS

// Conical frustum [t0, t1] of the ray o + t d whose pixel has area `pixel_area` at distance 1 -> mean and the DIAGONAL of the
// covariance of its Gaussian (the encoding reads nothing else of the 3 x 3 matrix). c = interval centre, h = half width
// (eq. 7 of arXiv:2103.13415 in its stable form). The along-ray projector is the raw d d^T, only the across-ray one is
// normalised (math.py:60-63): a direction of length != 1 comes out as the reference's. c = h = 0 is 0 / 0 there too.
NSAMD_HD void frustum_gaussian_diag(const float o[3], const float d[3], float t0, float t1, float pixel_area, float mean[3],
                                    float var[3]) {
  const float radius = sqrtf(pixel_area) / 1.7724538509055159f;  // sqrt(area / pi), rays.py:80
  const float c = (t0 + t1) / 2.0f, h = (t1 - t0) / 2.0f;
  const float c2 = c * c, h2 = h * h, h4 = h2 * h2;
  const float q = 3.0f * c2 + h2;
  const float t_mean = c + (2.0f * c * h2) / q;
  const float var_along = h2 / 3.0f - (float)(4.0 / 15.0) * ((h4 * (12.0f * c2 - h2)) / (q * q));
  const float var_across = (radius * radius) * ((c2 / 4.0f + (float)(5.0 / 12.0) * h2) - ((float)(4.0 / 15.0) * h4) / q);
  const float mag_sq = fmaxf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], 1.0e-10f);
  for (int k = 0; k < 3; ++k) {
    mean[k] = o[k] + d[k] * t_mean;
    var[k] = var_along * (d[k] * d[k]) + var_across * (1.0f - d[k] * (d[k] / mag_sq));
  }
}

// One entry of the encoding: E[sin(y)], y ~ N(s, var freq^2), s = (2 pi mean) freq (+ pi / 2 for the second half of the row).
// The variance is NOT multiplied by (2 pi)^2 — the reference's behaviour. Where the damping factor is exactly 0 the entry is 0
// and the sine is not evaluated: mip-NeRF's top frequencies (up to 2^16) are damped to zero for most samples, and those are the
// arguments that take sinf's slow range reduction.
NSAMD_HD float ipe_entry(float mean, float var, float freq, bool shifted) {
  const float damp = expf(-0.5f * (var * (freq * freq)));
  if (damp == 0.0f) return 0.0f;
  const float s = (6.283185307179586f * mean) * freq;
  return damp * sinf(shifted ? s + 1.5707963267948966f : s);
}

// Column `col` of a row [6 F (+3)]: k = axis * F + f in the first 3 F columns, the same shifted by pi / 2 in the next 3 F,
// the mean itself (`raw`) in the last three (include_input).
struct IpeColumn {
  int axis, f;
  bool shifted, raw;
};

NSAMD_HD IpeColumn ipe_column(int F, int col) {
  const int per = 3 * F;
  IpeColumn c;
  c.raw = col >= 2 * per;
  c.shifted = !c.raw && col >= per;
  const int k = c.raw ? 0 : (c.shifted ? col - per : col);
  c.axis = c.raw ? col - 2 * per : (k >= F ? 1 : 0) + (k >= 2 * F ? 1 : 0);
  c.f = c.raw ? 0 : k - c.axis * F;
  return c;
}

}  // namespace nsamd
