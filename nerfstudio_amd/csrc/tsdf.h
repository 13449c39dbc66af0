// Per-voxel arithmetic of TSDF fusion (gfx950; the host compiler sees it only through tests/hostcheck). Reference:
// nerfstudio/exporter/tsdf_utils.py — TSDF.from_aabb :88-113, TSDF.integrate_tsdf :172-274 — and the nearest-neighbour,
// zero-padded, align_corners=False form of torch.nn.functional.grid_sample that it samples the images with. fp32 with the
// reference's operations in the reference's order where the order decides something; the library is built with
// -ffp-contract=off.
//
// Two properties of the reference are KEPT, not repaired — parity is with the reference:
//  * the weight is clamped to 1 (:267), so from the second valid view on a voxel's value is the mean of its old value and the
//    new one, not the running mean over all views;
//  * a voxel BEHIND a camera (z < 0 after the flips of :213-215) still projects through the pinhole (:221 divides by the signed
//    z) and is integrated when it lands inside the image and passes the validity test of :245.
#pragma once

#include "common.h"
#include "../../include/nsamd_export.h"

namespace nsamd {

// one view's record, 18 floats, indexed by the view alone (uniform across a wave): w2c [3,4] and the first two rows of K [2,3]
constexpr int kTsdfPoseFloats = 12;
constexpr int kTsdfIntrinsicFloats = 6;

// Coordinate of voxel i along one axis (:100-104): origin + i * voxel_size, a multiply and then an add — the voxel's CORNER,
// not its centre, as in the reference.
NSAMD_HD float tsdf_voxel_coord(float origin, int32_t i, float voxel_size) { return origin + (float)i * voxel_size; }

// cam = w2c · (p, 1), then y = -y, z = -z (:210-215). w2c: [3,4] row-major.
NSAMD_HD void tsdf_camera_point(const float* w2c, float px, float py, float pz, float* x, float* y, float* z) {
  *x = ((w2c[0] * px + w2c[1] * py) + w2c[2] * pz) + w2c[3];
  *y = -(((w2c[4] * px + w2c[5] * py) + w2c[6] * pz) + w2c[7]);
  *z = -(((w2c[8] * px + w2c[9] * py) + w2c[10] * pz) + w2c[11]);
}

// The distance of the voxel from the camera, not its z (:218).
NSAMD_HD float tsdf_voxel_depth(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// Pixel coordinates (:220-222): K · (x / z, y / z, 1) with the first two rows of K [2,3]. z == 0 gives non-finite coordinates.
NSAMD_HD void tsdf_project(const float* K, float x, float y, float z, float* u, float* v) {
  const float a = x / z, b = y / z;
  *u = (K[0] * a + K[1] * b) + K[2];
  *v = (K[3] * a + K[4] * b) + K[5];
}

// Nearest pixel along one axis of `size` pixels: the reference's normalisation g = 2 u / size - 1 (:228), grid_sample's own
// unnormalisation for align_corners=False, ((g + 1) size - 1) / 2, ties to even. The bounds test 0 <= index <= size - 1 is made
// IN FLOAT, before any conversion to an integer: a non-finite coordinate (z == 0) fails both comparisons and lies outside.
NSAMD_HD bool tsdf_pixel_index(float coord, int32_t size, int32_t* index) {
  const float fs = (float)size;
  const float g = 2.0f * coord / fs - 1.0f;
  const float r = nearbyintf(((g + 1.0f) * fs - 1.0f) / 2.0f);
  const bool inside = r >= 0.0f && r <= (float)(size - 1);
  *index = inside ? (int32_t)r : 0;
  return inside;
}

// dist = sampled_depth - voxel_depth, the new value clamp(dist / truncation, -1, 1) (:243-244) and the validity test of :245;
// sampled_depth is 0 outside the image (padding_mode="zeros"), which fails `sampled_depth > 0`.
NSAMD_HD bool tsdf_observe(float sampled_depth, float voxel_depth, float truncation, float* new_value) {
  const float dist = sampled_depth - voxel_depth;
  *new_value = fminf(fmaxf(dist / truncation, -1.0f), 1.0f);
  return voxel_depth > 0.0f && sampled_depth > 0.0f && dist > -truncation;
}

// Running average of a valid voxel with new weight 1 (:254-274): total = weight + 1, value = (value * weight + new) / total,
// colour likewise, weight = min(total, 1). `colour`: the voxel's three channels; `sampled`: the pixel's, or NULL — no colour
// images, the colour stays as it is.
NSAMD_HD void tsdf_update(float* value, float* weight, float* colour, float new_value, const float* sampled) {
  const float w = *weight;
  const float total = w + 1.0f;
  *value = (*value * w + new_value) / total;
  if (sampled != nullptr)
    for (int c = 0; c < 3; ++c) colour[c] = (colour[c] * w + sampled[c]) / total;
  *weight = fminf(total, 1.0f);
}

// One view of one voxel at world position (px, py, pz): project, fetch the nearest depth (and colour) pixel of the view's
// image [H, W] (/ [H, W, 3]; `color` NULL: `colour` [3] is left alone), update the state in place. Returns whether the view
// was valid for the voxel.
NSAMD_HD bool tsdf_integrate_view(const float* w2c, const float* K, const float* depth, const float* color, int32_t H, int32_t W,
                                  float truncation, float px, float py, float pz, float* value, float* weight, float* colour) {
  float x, y, z, u, v;
  tsdf_camera_point(w2c, px, py, pz, &x, &y, &z);
  const float voxel_depth = tsdf_voxel_depth(x, y, z);
  tsdf_project(K, x, y, z, &u, &v);
  int32_t ix, iy;
  const bool in_x = tsdf_pixel_index(u, W, &ix);
  const bool in_y = tsdf_pixel_index(v, H, &iy);
  if (!(in_x && in_y)) return false;  // sample 0: never valid
  const int64_t pixel = (int64_t)iy * W + ix;
  float new_value;
  if (!tsdf_observe(depth[pixel], voxel_depth, truncation, &new_value)) return false;
  tsdf_update(value, weight, colour, new_value, color != nullptr ? color + 3 * pixel : nullptr);
  return true;
}

}  // namespace nsamd
