// Per-ray arithmetic of ray generation for perspective (with OpenCV distortion), fisheye and equirectangular cameras (gfx950;
// the host compiler sees it only through tests/hostcheck). Reference: Cameras._generate_rays_from_coords,
// nerfstudio/cameras/cameras.py:598-656 (coords, undistortion, y flip), :781-817 (local directions by camera type), :887-909
// (rotate, normalise, pixel area); camera_utils.py:375-478 (radial_and_tangential_undistort). fp32 with the reference's
// operations in the reference's order; the library is built with -ffp-contract=off.
#pragma once

#include "common.h"

namespace nsamd {

constexpr int kLensPerspective = 1;      // CameraType.PERSPECTIVE (cameras.py:41-52)
constexpr int kLensFisheye = 2;          // CameraType.FISHEYE
constexpr int kLensEquirectangular = 3;  // CameraType.EQUIRECTANGULAR

NSAMD_HD bool lens_type_supported(int type) { return type >= kLensPerspective && type <= kLensEquirectangular; }

// k = (k1, k2, k3, k4, p1, p2). The reference undistorts when ANY parameter of the batch is non-zero
// (`(distortion_params != 0).any()`, cameras.py:649); here the test is per camera. That changes no result: with all six zero
// d = 1, the residual is (1 * x + 0 + 0) - xd = 0 at x = xd, the denominator is 0 * 0 - 1 * 1 = -1, so every step is 0 / -1 and
// x + (-0) = x bit for bit, in all ten iterations (tests/test_lens_cpu.py runs lens_undistort on zeros to check it).
NSAMD_HD bool lens_has_distortion(const float* k) {
  return k != nullptr && (k[0] != 0.0f || k[1] != 0.0f || k[2] != 0.0f || k[3] != 0.0f || k[4] != 0.0f || k[5] != 0.0f);
}

// radial_and_tangential_undistort (camera_utils.py:441-478) of ONE coordinate: Newton's method on the OpenCV distortion model
// from the distorted point, exactly 10 iterations, a step skipped where |denominator| <= 1e-3 (the reference's torch.where).
NSAMD_HD void lens_undistort(float xd, float yd, const float* k, float* xo, float* yo) {
  const float k1 = k[0], k2 = k[1], k3 = k[2], k4 = k[3], p1 = k[4], p2 = k[5];
  float x = xd, y = yd;
  for (int it = 0; it < 10; ++it) {
    // _compute_residual_and_jacobian (camera_utils.py:375-437)
    const float r = x * x + y * y;
    const float d = 1.0f + r * (k1 + r * (k2 + r * (k3 + r * k4)));
    const float fx = ((d * x + ((2.0f * p1) * x) * y) + p2 * (r + (2.0f * x) * x)) - xd;
    const float fy = ((d * y + ((2.0f * p2) * x) * y) + p1 * (r + (2.0f * y) * y)) - yd;
    const float d_r = k1 + r * (2.0f * k2 + r * (3.0f * k3 + (r * 4.0f) * k4));
    const float d_x = (2.0f * x) * d_r;
    const float d_y = (2.0f * y) * d_r;
    const float fx_x = ((d + d_x * x) + (2.0f * p1) * y) + (6.0f * p2) * x;
    const float fx_y = (d_y * x + (2.0f * p1) * x) + (2.0f * p2) * y;
    const float fy_x = (d_x * y + (2.0f * p2) * y) + (2.0f * p1) * x;
    const float fy_y = ((d + d_y * y) + (2.0f * p2) * x) + (6.0f * p1) * y;
    const float den = fy_x * fx_y - fx_x * fy_y;
    const float x_num = fx * fy_y - fy * fx_y;
    const float y_num = fy * fx_x - fx * fy_x;
    const bool step = fabsf(den) > 1e-3f;
    x = x + (step ? x_num / den : 0.0f);
    y = y + (step ? y_num / den : 0.0f);
  }
  *xo = x;
  *yo = y;
}

// Direction in camera coordinates (OpenGL: +y up, looking down -z) of the image coordinate (u, v), v already flipped
// (cameras.py:655-656). cameras.py:781-817. Fisheye at u = v = 0 is 0 / 0 as in the reference.
NSAMD_HD void lens_local_direction(int type, float u, float v, float* out) {
  const float pi = 3.14159265358979323846f;
  if (type == kLensFisheye) {
    const float theta = fminf(fmaxf(sqrtf(u * u + v * v), 0.0f), pi);
    const float s = sinf(theta);
    out[0] = u * s / theta;
    out[1] = v * s / theta;
    out[2] = -cosf(theta);
  } else if (type == kLensEquirectangular) {
    const float theta = -pi * u;  // minus sign for right-handed
    const float phi = pi * (0.5f - v);
    const float sp = sinf(phi);
    out[0] = -sinf(theta) * sp;
    out[1] = cosf(phi);
    out[2] = -cosf(theta) * sp;
  } else {
    out[0] = u;
    out[1] = v;
    out[2] = -1.0f;
  }
}

// The shared tail (cameras.py:887-909): the three local directions l[k] — centre, +1 pixel in x, +1 pixel in y — rotated by the
// pose m [3,4], normalize_with_norm, the ray's origin, direction, pixel area dx * dy and the centre's norm.
NSAMD_HD void raygen_finish(const float (&l)[3][3], const float* __restrict__ m, float* __restrict__ origin,
                            float* __restrict__ direction, float* __restrict__ pixel_area, float* __restrict__ direction_norm) {
  const float eps = 8.881784197001252e-16f;  // camera_utils._EPS = 4 * float64 eps, cast to fp32
  float d[3][3];
  float n0 = 0.0f;
  for (int k = 0; k < 3; ++k) {
    const float lx = l[k][0], ly = l[k][1], lz = l[k][2];
    float v[3];
    for (int r = 0; r < 3; ++r) v[r] = (lx * m[4 * r + 0] + ly * m[4 * r + 1]) + lz * m[4 * r + 2];
    const float nrm = fmaxf(sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), eps);
    if (k == 0) n0 = nrm;
    for (int r = 0; r < 3; ++r) d[k][r] = v[r] / nrm;
  }
  float dx = 0.0f, dy = 0.0f;
  for (int r = 0; r < 3; ++r) {
    const float a = d[0][r] - d[1][r], b = d[0][r] - d[2][r];
    dx += a * a;
    dy += b * b;
  }
  dx = sqrtf(dx);
  dy = sqrtf(dy);
  for (int r = 0; r < 3; ++r) {
    origin[r] = m[4 * r + 3];
    direction[r] = d[0][r];
  }
  if (pixel_area) *pixel_area = dx * dy;
  if (direction_norm) *direction_norm = n0;
}

// One ray of a camera of type 1 - 3 at pixel-centre coordinates (x, y): image coordinates of the centre and of its two
// neighbours (cameras.py:622-634), undistorted unless the camera is equirectangular (:645-653) or has no distortion, flipped to
// OpenGL, turned into local directions by lens type, then the shared tail. k: the camera's six parameters, or null.
NSAMD_HD void raygen_lens_one(float x, float y, float fxr, float fyr, float cxr, float cyr, int type, const float* k,
                              const float* __restrict__ m, float* __restrict__ origin, float* __restrict__ direction,
                              float* __restrict__ pixel_area, float* __restrict__ direction_norm) {
  float px[3] = {(x - cxr) / fxr, (x - cxr + 1.0f) / fxr, (x - cxr) / fxr};
  float py[3] = {(y - cyr) / fyr, (y - cyr) / fyr, (y - cyr + 1.0f) / fyr};
  if (type != kLensEquirectangular && lens_has_distortion(k)) {
    const float kk[6] = {k[0], k[1], k[2], k[3], k[4], k[5]};
    for (int c = 0; c < 3; ++c) lens_undistort(px[c], py[c], kk, &px[c], &py[c]);
  }
  float l[3][3];
  for (int c = 0; c < 3; ++c) lens_local_direction(type, px[c], -py[c], l[c]);
  raygen_finish(l, m, origin, direction, pixel_area, direction_norm);
}

}  // namespace nsamd
