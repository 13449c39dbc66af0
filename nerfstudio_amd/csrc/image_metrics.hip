// Eval image metrics and colormaps (include/nsamd_image.h): nsamd_image_range / nsamd_image_metrics / nsamd_colormap. Where the
// library path reflect-pads, concatenates five images, runs a 121-tap depth-wise convolution and a dozen elementwise launches,
// and reads minima and maxima back to the host, a workgroup here holds a tile's pixels of both images in LDS, runs the 11-tap
// pass along rows and along columns over the five moment planes and leaves two fp64 partial sums; a second one-workgroup launch
// adds them in index order. The per-window and per-pixel arithmetic is image_metrics.h.
#include "launch.h"
#include "image_metrics.h"
#include "wave.h"

using namespace nsamd;

namespace {

constexpr int kImgThreads = NSAMD_IMAGE_BLOCK;  // four wavefronts
constexpr int kImgWaves = kImgThreads / 64;
constexpr int kTile = NSAMD_SSIM_TILE;
constexpr int kPixelStride = kSsimRegion + 1;  // 43 words per row of the pixel planes, 33 per row of the moment planes: odd, so
constexpr int kMomentStride = kTile + 1;       // the column pass (a wavefront = two rows of 32 windows) stays conflict-free

// Workgroup (ty, tx) of the (H - 10) x (W - 10) windows' tiling. Per channel: the tile's (T + 10)^2 pixels of both images minus
// their pivots into LDS (a wavefront reads consecutive pixels of a row; the C channels of a pixel share their cache lines
// across the channel loop), the squared error of the pixels the tile owns on the way; the row pass over (T + 10) x T
// positions; the column pass and the window's value over T x T. Positions past the image hold zeros and are never summed.
// The loops' trip counts do not depend on the lane: every barrier is reached by all 256.
__global__ __launch_bounds__(kImgThreads) void image_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                    int H, int W, int C, const float* __restrict__ range_pred,
                                                                    const float* __restrict__ range_target, float data_range,
                                                                    double* __restrict__ partials, float* __restrict__ ssim_map) {
  __shared__ float dx[kSsimRegion * kPixelStride];
  __shared__ float dy[kSsimRegion * kPixelStride];
  __shared__ float rows[kSsimMoments][kSsimRegion * kMomentStride];
  const int tiles_x = (int)ssim_tiles(W);
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const SsimSpan sy = ssim_span(H, ty), sx = ssim_span(W, tx);
  const float R = range_pred != nullptr ? ssim_data_range(range_pred, range_target) : data_range;
  float c1, c2;
  ssim_constants(R, &c1, &c2);
  double ssim_acc = 0.0, se_acc = 0.0;
  for (int c = 0; c < C; ++c) {
    const int64_t centre = ((int64_t)(sy.first + sy.pixels / 2) * W + (sx.first + sx.pixels / 2)) * C + c;
    const float px = ssim_pivot(pred[centre]), py = ssim_pivot(target[centre]);
    for (int i = threadIdx.x; i < kSsimRegion * kSsimRegion; i += kImgThreads) {
      const int r = i / kSsimRegion, q = i - r * kSsimRegion;
      float ex = 0.0f, ey = 0.0f;
      if (r < sy.pixels && q < sx.pixels) {
        const int64_t g = ((int64_t)(sy.first + r) * W + (sx.first + q)) * C + c;
        const float x = pred[g], y = target[g];
        if (r < sy.owned && q < sx.owned) se_acc += squared_error(x, y);
        ex = x - px;
        ey = y - py;
      }
      dx[r * kPixelStride + q] = ex;
      dy[r * kPixelStride + q] = ey;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSsimRegion * kTile; i += kImgThreads) {
      const int r = i / kTile, q = i - r * kTile;
      float m[kSsimMoments];
      ssim_row_moments(&dx[r * kPixelStride + q], &dy[r * kPixelStride + q], m);
      for (int k = 0; k < kSsimMoments; ++k) rows[k][r * kMomentStride + q] = m[k];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTile * kTile; i += kImgThreads) {
      const int wy = i / kTile, wx = i - wy * kTile;
      float M[kSsimMoments];
      for (int k = 0; k < kSsimMoments; ++k) M[k] = ssim_tap(&rows[k][wy * kMomentStride + wx], kMomentStride);
      if (wy < sy.windows && wx < sx.windows) {
        const float v = ssim_window(M, px, py, c1, c2);
        ssim_acc += (double)v;
        if (ssim_map != nullptr) ssim_map[((int64_t)(sy.first + wy) * (W - kSsimHalo) + (sx.first + wx)) * C + c] = v;
      }
    }
    // the next channel's loads write dx, dy: every lane is past the row pass that read them; its row pass writes rows[] behind
    // the barrier that follows the loads, which no lane reaches before it has left this column pass
  }
  const double ssim_total = block_sum_f64<kImgWaves>(ssim_acc);
  const double se_total = block_sum_f64<kImgWaves>(se_acc);
  if (threadIdx.x == 0) {
    partials[2 * (int64_t)blockIdx.x] = ssim_total;
    partials[2 * (int64_t)blockIdx.x + 1] = se_total;
  }
}

// ONE workgroup: the tiles' partial sums in the same fixed order, then the one rounding of each result
__global__ __launch_bounds__(kImgThreads) void image_metrics_finish_kernel(const double* __restrict__ partials, int tiles, int H,
                                                                           int W, int C, const float* __restrict__ range_pred,
                                                                           const float* __restrict__ range_target,
                                                                           float data_range, float psnr_range,
                                                                           float* __restrict__ out4) {
  double ssim_acc = 0.0, se_acc = 0.0;
  for (int t = threadIdx.x; t < tiles; t += kImgThreads) ssim_acc += partials[2 * t], se_acc += partials[2 * t + 1];
  const double ssim_total = block_sum_f64<kImgWaves>(ssim_acc);
  const double se_total = block_sum_f64<kImgWaves>(se_acc);
  if (threadIdx.x == 0) {
    const float R = range_pred != nullptr ? ssim_data_range(range_pred, range_target) : data_range;
    image_metrics_finish(ssim_total, se_total, H, W, C, R, psnr_range, out4);
  }
}

// minimum, maximum and NaN flag over the workgroup: a butterfly per wavefront, the wavefronts in index order (the operations
// are order-free). Every thread calls it; valid in every thread.
__device__ __forceinline__ RangeAcc block_range(RangeAcc a) {
  __shared__ float wave_lo[kImgWaves], wave_hi[kImgWaves];
  __shared__ int wave_nan[kImgWaves];
  for (int m = 1; m < 64; m <<= 1) range_merge(a, __shfl_xor(a.lo, m), __shfl_xor(a.hi, m), __shfl_xor(a.nan, m));
  if ((threadIdx.x & 63) == 0) wave_lo[threadIdx.x >> 6] = a.lo, wave_hi[threadIdx.x >> 6] = a.hi, wave_nan[threadIdx.x >> 6] = a.nan;
  __syncthreads();
  RangeAcc total = range_empty();
  for (int w = 0; w < kImgWaves; ++w) range_merge(total, wave_lo[w], wave_hi[w], wave_nan[w]);
  return total;
}

// workgroup b: values b * 256 + lane, then every gridDim.x * 256 further
__global__ __launch_bounds__(kImgThreads) void image_range_partial_kernel(const float* __restrict__ x, int64_t n,
                                                                          float* __restrict__ partials) {
  RangeAcc a = range_empty();
  for (int64_t i = (int64_t)blockIdx.x * kImgThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kImgThreads) range_fold(a, x[i]);
  const RangeAcc total = block_range(a);
  if (threadIdx.x == 0) range_store(total, partials + 2 * (int64_t)blockIdx.x);
}

// ONE workgroup: the pairs of the partial launch (a NaN pair carries its workgroup's flag)
__global__ __launch_bounds__(kImgThreads) void image_range_finish_kernel(const float* __restrict__ partials, int blocks,
                                                                         float* __restrict__ range2) {
  RangeAcc a = range_empty();
  for (int b = threadIdx.x; b < blocks; b += kImgThreads) range_merge(a, partials[2 * b], partials[2 * b + 1], 0);
  const RangeAcc total = block_range(a);
  if (threadIdx.x == 0) range_store(total, range2);
}

// One lane per pixel; the 3 KiB table is read once per workgroup into LDS, where 64 lanes' scattered rows cost no cache lines.
template <bool kGray>
__global__ __launch_bounds__(kImgThreads) void colormap_kernel(const float* __restrict__ values, int64_t n,
                                                               const float* __restrict__ lut, const float* __restrict__ range2,
                                                               const float* __restrict__ accumulation, nsamd_colormap_params params,
                                                               float* __restrict__ out_rgb, uint8_t* __restrict__ out_u8) {
  __shared__ float table[kGray ? 1 : 256 * 3];
  if (!kGray) {
    for (int i = threadIdx.x; i < 256 * 3; i += kImgThreads) table[i] = lut[i];
    __syncthreads();
  }
  const int64_t i = (int64_t)blockIdx.x * kImgThreads + threadIdx.x;
  if (i >= n) return;
  const ColormapConsts k = colormap_consts(params, range2);
  const bool has_acc = accumulation != nullptr;
  float rgb[3];
  if (kGray)
    colormap_pixel(k, nullptr, values[i], has_acc, has_acc ? accumulation[i] : 0.0f, rgb);
  else
    colormap_pixel(k, table, values[i], has_acc, has_acc ? accumulation[i] : 0.0f, rgb);
  for (int c = 0; c < 3; ++c) {
    if (out_rgb != nullptr) out_rgb[3 * i + c] = rgb[c];
    if (out_u8 != nullptr) out_u8[3 * i + c] = (uint8_t)texture_level(rgb[c]);
  }
}

}  // namespace

extern "C" int nsamd_image_range(const float* x, int64_t n, void* scratch, float* range2_dev, nsamd_stream_t stream) {
  const int sizes = image_range_check(n);
  if (sizes != NSAMD_OK) return sizes;
  NSAMD_REQUIRE(x && scratch && range2_dev);
  const int blocks = (int)image_range_blocks(n);
  hipStream_t s = (hipStream_t)stream;
  image_range_partial_kernel<<<blocks, kImgThreads, 0, s>>>(x, n, reinterpret_cast<float*>(scratch));
  NSAMD_CHECK_LAUNCH();
  image_range_finish_kernel<<<1, kImgThreads, 0, s>>>(reinterpret_cast<const float*>(scratch), blocks, range2_dev);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int64_t nsamd_image_metrics_scratch_bytes(int64_t H, int64_t W, int32_t C) {
  if (image_metrics_check(H, W, C) != NSAMD_OK) return 0;
  return 16 * ssim_tiles(H) * ssim_tiles(W);
}

extern "C" int nsamd_image_metrics(const float* pred, const float* target, int64_t H, int64_t W, int32_t C,
                                   const float* range_pred2_dev, const float* range_target2_dev, float data_range, float psnr_range,
                                   void* scratch, float* out4_dev, float* ssim_map, nsamd_stream_t stream) {
  const int sizes = image_metrics_check(H, W, C);
  if (sizes != NSAMD_OK) return sizes;
  NSAMD_REQUIRE(pred && target && scratch && out4_dev && psnr_range > 0.0f);
  NSAMD_REQUIRE((range_pred2_dev == nullptr) == (range_target2_dev == nullptr));
  NSAMD_REQUIRE(range_pred2_dev != nullptr || data_range > 0.0f);
  const int64_t tiles = ssim_tiles(H) * ssim_tiles(W);
  unsigned blocks = 0;
  const int status = grid_blocks(tiles, &blocks);
  if (status != NSAMD_OK) return status;
  hipStream_t s = (hipStream_t)stream;
  double* partials = reinterpret_cast<double*>(scratch);
  image_metrics_kernel<<<blocks, kImgThreads, 0, s>>>(pred, target, (int)H, (int)W, (int)C, range_pred2_dev, range_target2_dev,
                                                      data_range, partials, ssim_map);
  NSAMD_CHECK_LAUNCH();
  image_metrics_finish_kernel<<<1, kImgThreads, 0, s>>>(partials, (int)tiles, (int)H, (int)W, (int)C, range_pred2_dev,
                                                        range_target2_dev, data_range, psnr_range, out4_dev);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int nsamd_colormap(const float* values, int64_t n, const float* lut, const float* range2_dev, const float* accumulation,
                              nsamd_colormap_params params, float* out_rgb, uint8_t* out_u8, nsamd_stream_t stream) {
  const int args = colormap_check(n, params, values, range2_dev, accumulation, out_rgb, out_u8);
  if (args != NSAMD_OK) return args;
  unsigned blocks = 0;
  const int status = grid_blocks((n + kImgThreads - 1) / kImgThreads, &blocks);
  if (status != NSAMD_OK) return status;
  hipStream_t s = (hipStream_t)stream;
  if (lut == nullptr)
    colormap_kernel<true><<<blocks, kImgThreads, 0, s>>>(values, n, lut, range2_dev, accumulation, params, out_rgb, out_u8);
  else
    colormap_kernel<false><<<blocks, kImgThreads, 0, s>>>(values, n, lut, range2_dev, accumulation, params, out_rgb, out_u8);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}
