/*
 * nsamd_export.h — the part of libnsamd.so's C ABI that serves mesh export (ns-export tsdf), apart from the training and
 * rendering core of nsamd.h. Conventions as there: device pointers, fp32, dense row-major tensors, a small POD struct passed by
 * value, a hipStream_t; 0 (NSAMD_OK) or a negative nsamd_status, nothing launched on error, no synchronisation.
 * Paths are relative to /root/reference/nerfstudio/.
 */
#ifndef NSAMD_EXPORT_H
#define NSAMD_EXPORT_H

#include "nsamd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------
 * Mesh export: fusion of B rendered frames into a TSDF volume — TSDF.integrate_tsdf (exporter/tsdf_utils.py:172-274), which
 * builds [B, voxels] temporaries with ~40 torch launches, as ONE pass: one lane per voxel (z fastest), the voxel's state
 * loaded once, updated by the views in view order, stored once and only when some view was valid for it: 20 B of state per
 * voxel read, 20 B written for a touched voxel, per launch whatever B is. values, weights [X,Y,Z], colors [X,Y,Z,3]
 * (nullable) are updated in place. Per view b:
 * w2c [B,3,4] = the inverse of the camera-to-world pose, K [B,2,3] = the first two rows of the intrinsics, depth [B,H,W],
 * color [B,H,W,3] (nullable; colours are left as they are when either is NULL). A voxel's coordinate is origin + i *
 * voxel_size per axis — its corner (:100-104); it is projected as :210-222 (camera y and z flipped, depth = the DISTANCE),
 * sampled as grid_sample(mode="nearest", padding_mode="zeros", align_corners=False) (:228-241), valid when voxel_depth > 0,
 * sampled_depth > 0 and sampled_depth - voxel_depth > -truncation (:243-245), and averaged with its clamped weight as
 * :254-274: total = weight + 1, value = (value * weight + clamp(dist / truncation, -1, 1)) / total, weight = min(total, 1).
 * Kept as the reference has them: the weight clamp (a voxel's value is the mean of its old value and the new one from the
 * second valid view on) and voxels behind a camera, which project through the pinhole and are integrated when they land
 * inside the image. truncation = voxel_size[0] * truncation_margin (:80-85) is the caller's. No allocation, no
 * synchronisation, no atomics: capturable, and the same bits run to run. B == 0 or a volume without voxels is a no-op; more
 * than 256 * (2^31 - 1) voxels: NSAMD_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct nsamd_tsdf_volume {
  float origin[3];     /* aabb minimum                          */
  float voxel_size[3]; /* (aabb maximum - aabb minimum) / dims  */
  int32_t dims[3];     /* X, Y, Z                               */
  float truncation;    /* > 0                                   */
} nsamd_tsdf_volume;
int nsamd_tsdf_integrate(nsamd_tsdf_volume vol, float* values, float* weights, float* colors, const float* w2c,
                         const float* K, int32_t B, const float* depth, const float* color, int32_t H, int32_t W,
                         nsamd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NSAMD_EXPORT_H */
