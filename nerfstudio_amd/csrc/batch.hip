// A training batch sampled on the device for gfx950: pixel draw, colour gather from an image store in HBM and ray generation
// in one launch — what VanillaDataManager.next_train does on the host every iteration
// (nerfstudio/data/datamanagers/base_datamanager.py:506-515: PixelSampler.sample, data/pixel_samplers.py:137-174
// and :265-330, then RayGenerator, model_components/ray_generators.py:41-56).
#include "batch_sample.h"
#include "common.h"
#include "launch.h"
#include "lens.h"

namespace nsamd {

// One ray per lane. Latency-bound: per lane one Philox block (or one per rejected draw), a dependent chain of gathers (mask
// byte -> three colour bytes; the camera's record through L2) and raygen_lens_one. The draw counter is only READ: the grid has
// many workgroups, so whoever owns the counter advances it in a launch of its own (the step prologue, or a torch op).
// Nothing in the arguments changes from step to step, so the launch replays as a node of a captured iteration.
__global__ __launch_bounds__(256) void sample_batch_kernel(
    const uint8_t* __restrict__ images, const uint8_t* __restrict__ mask, int32_t num_images, int32_t height, int32_t width,
    const float* __restrict__ c2w, const float* __restrict__ fx, const float* __restrict__ fy, const float* __restrict__ cx,
    const float* __restrict__ cy, const int32_t* __restrict__ camera_type, const float* __restrict__ distortion,
    const int64_t* __restrict__ draw_counter, int64_t draw_offset, uint64_t key, int32_t max_attempts, int64_t n,
    float* __restrict__ origins, float* __restrict__ directions, float* __restrict__ pixel_area,
    float* __restrict__ directions_norm, int64_t* __restrict__ camera_indices, float* __restrict__ target,
    int64_t* __restrict__ indices, int32_t* __restrict__ failed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t draw = draw_counter[0] + draw_offset;
  int32_t c, y, x;
  batch_draw_pixel((uint32_t)i, 0u, draw, key, num_images, height, width, &c, &y, &x);
  int64_t pixel = ((int64_t)c * height + y) * width + x;  // (the indices are clamped to the store: batch_pixel_index)
  if (mask != nullptr) {
    // rejection_sample_mask (pixel_samplers.py:82-119), lane-local: redraw while the pixel is masked out, at most
    // max_attempts times; a lane that runs out keeps its last draw and is counted
    int32_t attempt = 0;
    while (mask[pixel] == 0 && attempt < max_attempts) {
      ++attempt;
      batch_draw_pixel((uint32_t)i, (uint32_t)attempt, draw, key, num_images, height, width, &c, &y, &x);
      pixel = ((int64_t)c * height + y) * width + x;
    }
    if (mask[pixel] == 0) atomicAdd(failed, 1);
  }
  const uint8_t* rgb = images + 3 * pixel;
  target[3 * i + 0] = batch_pixel_float(rgb[0]);
  target[3 * i + 1] = batch_pixel_float(rgb[1]);
  target[3 * i + 2] = batch_pixel_float(rgb[2]);
  camera_indices[i] = c;
  if (indices != nullptr) {
    indices[3 * i + 0] = c;
    indices[3 * i + 1] = y;
    indices[3 * i + 2] = x;
  }
  // the call of raygen_lens_kernel (misc.hip): the same bits as nsamd_raygen_lens over `indices`
  raygen_lens_one((float)x + 0.5f, (float)y + 0.5f, fx[c], fy[c], cx[c], cy[c], camera_type[c],
                  distortion ? distortion + 6 * c : nullptr, c2w + (int64_t)c * 12, origins + 3 * i, directions + 3 * i,
                  pixel_area ? pixel_area + i : nullptr, directions_norm ? directions_norm + i : nullptr);
}

}  // namespace nsamd

using namespace nsamd;

extern "C" int nsamd_sample_batch(const uint8_t* images, const uint8_t* mask, int32_t num_images, int32_t height,
                                  int32_t width, const float* c2w, const float* fx, const float* fy, const float* cx,
                                  const float* cy, const int32_t* camera_type, const float* distortion,
                                  const int64_t* draw_counter, int64_t draw_offset, uint64_t seed, int32_t max_attempts,
                                  int64_t num_rays, float* origins, float* directions, float* pixel_area,
                                  float* directions_norm, int64_t* camera_indices, float* target, int64_t* indices,
                                  int32_t* failed, nsamd_stream_t stream) {
  NSAMD_REQUIRE(num_rays >= 0 && num_images > 0 && height > 0 && width > 0 && max_attempts >= 0);
  NSAMD_REQUIRE(images && c2w && fx && fy && cx && cy && camera_type && draw_counter);
  NSAMD_REQUIRE(mask == nullptr || failed != nullptr);
  // the pixel index recipe is exact for dimensions a float holds (batch_sample.h); the ray index is one Philox counter word
  if (num_images >= (1 << 24) || height >= (1 << 24) || width >= (1 << 24) || num_rays > 0xffffffffLL) return NSAMD_ERR_UNSUPPORTED;
  if (num_rays == 0) return NSAMD_OK;
  NSAMD_REQUIRE(origins && directions && camera_indices && target);
  unsigned blocks;
  const int status = grid_blocks((num_rays + 255) / 256, &blocks);
  if (status != NSAMD_OK) return status;
  sample_batch_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(
      images, mask, num_images, height, width, c2w, fx, fy, cx, cy, camera_type, distortion, draw_counter, draw_offset,
      seed ^ kBatchSeedXor, max_attempts, num_rays, origins, directions, pixel_area, directions_norm, camera_indices, target,
      indices, failed);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}
