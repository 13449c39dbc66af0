// Host build of nerfstudio_amd/csrc/tsdf.h for tests/test_tsdf_cpu.py: the per-voxel arithmetic nsamd_tsdf_integrate runs per
// lane, looped over the voxels the way the kernel composes it (z fastest; the state loaded once, the views in view order, stored
// once and only when some view was valid). Test infrastructure: the product never loads it.
#include "../../nerfstudio_amd/csrc/tsdf.h"

using namespace nsamd;

// The entry point's arguments on host memory. stores (nullable): the number of voxels whose state was written back.
extern "C" int hc_tsdf_integrate(nsamd_tsdf_volume vol, float* values, float* weights, float* colors, const float* w2c,
                                 const float* K, int32_t B, const float* depth, const float* color, int32_t H, int32_t W,
                                 int64_t* stores) {
  if (B < 0 || vol.dims[0] < 0 || vol.dims[1] < 0 || vol.dims[2] < 0) return -1;
  const int64_t plane = (int64_t)vol.dims[1] * vol.dims[2], num_voxels = plane * vol.dims[0];
  if (stores) *stores = 0;
  if (B == 0 || num_voxels == 0) return 0;
  if (!values || !weights || !w2c || !K || !depth || H <= 0 || W <= 0 || !(vol.truncation > 0.0f)) return -1;
  const bool coloured = colors != nullptr && color != nullptr;
  const int64_t image = (int64_t)H * W;
  for (int64_t voxel = 0; voxel < num_voxels; ++voxel) {
    const int64_t i = point_ray(voxel, plane);
    const int64_t rest = voxel - i * plane;
    const int64_t j = point_ray(rest, vol.dims[2]);
    const int64_t k = rest - j * vol.dims[2];
    const float px = tsdf_voxel_coord(vol.origin[0], (int32_t)i, vol.voxel_size[0]);
    const float py = tsdf_voxel_coord(vol.origin[1], (int32_t)j, vol.voxel_size[1]);
    const float pz = tsdf_voxel_coord(vol.origin[2], (int32_t)k, vol.voxel_size[2]);
    float value = values[voxel], weight = weights[voxel];
    float colour[3] = {0.0f, 0.0f, 0.0f};
    if (coloured)
      for (int c = 0; c < 3; ++c) colour[c] = colors[3 * voxel + c];
    bool touched = false;
    for (int32_t b = 0; b < B; ++b)
      touched |= tsdf_integrate_view(w2c + kTsdfPoseFloats * (int64_t)b, K + kTsdfIntrinsicFloats * (int64_t)b,
                                     depth + b * image, coloured ? color + 3 * b * image : nullptr, H, W, vol.truncation, px, py, pz,
                                     &value, &weight, colour);
    if (!touched) continue;
    if (stores) ++*stores;
    values[voxel] = value;
    weights[voxel] = weight;
    if (coloured)
      for (int c = 0; c < 3; ++c) colors[3 * voxel + c] = colour[c];
  }
  return 0;
}
