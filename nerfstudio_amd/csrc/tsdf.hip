// TSDF fusion of rendered depth (and colour) frames into a voxel volume: nsamd_tsdf_integrate. What the reference's
// TSDF.integrate_tsdf (exporter/tsdf_utils.py:172-274) does with ~40 eager torch launches over [batch, voxels] temporaries is
// one memory-bound pass here: 20 B of state per voxel (value, weight, colour) read once per launch and written once for the voxels
// a view was valid for, whatever the number of views.
// The per-voxel arithmetic is tsdf.h.
#include "launch.h"
#include "tsdf.h"

using namespace nsamd;

namespace {

constexpr int kTsdfThreads = 256;  // four wavefronts

// One lane per voxel, z fastest: a wavefront's 64 lanes touch 256 contiguous bytes of `values` and `weights` and 768 of
// `colors`. The voxel's state is loaded once, carried in registers across the views IN VIEW ORDER (the reference updates
// sequentially, :249-274) and stored once, only when some view was valid for the voxel. The views' records are indexed by the
// loop counter alone: uniform across the wave. No atomics, no traffic between workgroups: the same bits run to run.
__global__ __launch_bounds__(kTsdfThreads) void tsdf_integrate_kernel(
    nsamd_tsdf_volume vol, int64_t num_voxels, float* __restrict__ values, float* __restrict__ weights,
    float* __restrict__ colors, const float* __restrict__ w2c, const float* __restrict__ K, int32_t B,
    const float* __restrict__ depth, const float* __restrict__ color, int32_t H, int32_t W) {
  const int64_t voxel = (int64_t)blockIdx.x * kTsdfThreads + threadIdx.x;
  if (voxel >= num_voxels) return;
  const int64_t plane = (int64_t)vol.dims[1] * vol.dims[2];
  const int64_t i = point_ray(voxel, plane);
  const int64_t rest = voxel - i * plane;
  const int64_t j = point_ray(rest, vol.dims[2]);
  const int64_t k = rest - j * vol.dims[2];
  const float px = tsdf_voxel_coord(vol.origin[0], (int32_t)i, vol.voxel_size[0]);
  const float py = tsdf_voxel_coord(vol.origin[1], (int32_t)j, vol.voxel_size[1]);
  const float pz = tsdf_voxel_coord(vol.origin[2], (int32_t)k, vol.voxel_size[2]);

  const bool coloured = colors != nullptr && color != nullptr;
  float value = values[voxel], weight = weights[voxel];
  float colour[3] = {0.0f, 0.0f, 0.0f};
  if (coloured)
    for (int c = 0; c < 3; ++c) colour[c] = colors[3 * voxel + c];

  const int64_t image = (int64_t)H * W;
  bool touched = false;
  for (int32_t b = 0; b < B; ++b)
    touched |= tsdf_integrate_view(w2c + kTsdfPoseFloats * (int64_t)b, K + kTsdfIntrinsicFloats * (int64_t)b, depth + b * image,
                                   coloured ? color + 3 * b * image : nullptr, H, W, vol.truncation, px, py, pz, &value, &weight,
                                   colour);
  if (!touched) return;
  values[voxel] = value;
  weights[voxel] = weight;
  if (coloured)
    for (int c = 0; c < 3; ++c) colors[3 * voxel + c] = colour[c];
}

}  // namespace

extern "C" int nsamd_tsdf_integrate(nsamd_tsdf_volume vol, float* values, float* weights, float* colors, const float* w2c,
                                    const float* K, int32_t B, const float* depth, const float* color, int32_t H, int32_t W,
                                    nsamd_stream_t stream) {
  NSAMD_REQUIRE(B >= 0 && vol.dims[0] >= 0 && vol.dims[1] >= 0 && vol.dims[2] >= 0);
  const int64_t plane = (int64_t)vol.dims[1] * vol.dims[2];  // < 2^62
  if (B == 0 || vol.dims[0] == 0 || plane == 0) return NSAMD_OK;
  if (plane > (int64_t)kTsdfThreads * 0x7fffffffLL / vol.dims[0]) return NSAMD_ERR_UNSUPPORTED;  // more voxels than a grid covers
  const int64_t num_voxels = plane * vol.dims[0];
  NSAMD_REQUIRE(values && weights && w2c && K && depth && H > 0 && W > 0 && vol.truncation > 0.0f);
  unsigned blocks = 0;
  const int status = grid_blocks((num_voxels + kTsdfThreads - 1) / kTsdfThreads, &blocks);
  if (status != NSAMD_OK) return status;
  tsdf_integrate_kernel<<<blocks, kTsdfThreads, 0, (hipStream_t)stream>>>(vol, num_voxels, values, weights, colors, w2c, K, B, depth,
                                                                          color, H, W);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}
