// Host build of nerfstudio_amd/csrc/image_metrics.h for tests/test_image_metrics_cpu.py and tests/test_colormaps_cpu.py (and
// tests/hostcheck/image_main.cc): the arithmetic of the image entry points, looped the way the kernels compose it — a tile's
// pixels minus their pivots in exactly-sized planes, the row pass, the column pass, each lane's fp64 sums over its stride, a
// butterfly per wavefront, the wavefronts and then the tiles in index order; the minimum and maximum in the two levels of the
// range kernel; one pixel of the colormap per lane. Host memory in place of device memory; the argument checks are the entry
// points' own (image_metrics.h). Test infrastructure: the product never loads it.
#include <vector>

#include "../../nerfstudio_amd/csrc/image_metrics.h"

using namespace nsamd;

namespace {

constexpr int kLanes = NSAMD_IMAGE_BLOCK;
constexpr int kTile = NSAMD_SSIM_TILE;

// the sum of one workgroup's 256 lane values as block_sum_f64 forms it: a butterfly per wavefront, the wavefronts in order
double block_sum(const double* lanes) {
  double total = 0.0;
  for (int w = 0; w < kLanes / 64; ++w) {
    double v[64];
    for (int l = 0; l < 64; ++l) v[l] = lanes[64 * w + l];
    for (int m = 1; m < 64; m <<= 1) {
      double next[64];
      for (int l = 0; l < 64; ++l) next[l] = v[l] + v[l ^ m];
      for (int l = 0; l < 64; ++l) v[l] = next[l];
    }
    total += v[0];
  }
  return total;
}

}  // namespace

extern "C" int hc_image_range(const float* x, int64_t n, void* scratch, float* range2) {
  const int sizes = image_range_check(n);
  if (sizes != NSAMD_OK) return sizes;
  if (!(x && scratch && range2)) return NSAMD_ERR_INVALID_ARG;
  const int64_t blocks = image_range_blocks(n);
  float* partials = reinterpret_cast<float*>(scratch);
  for (int64_t b = 0; b < blocks; ++b) {
    RangeAcc total = range_empty();
    for (int l = 0; l < kLanes; ++l) {
      RangeAcc a = range_empty();
      for (int64_t i = b * kLanes + l; i < n; i += blocks * kLanes) range_fold(a, x[i]);
      range_merge(total, a.lo, a.hi, a.nan);
    }
    range_store(total, partials + 2 * b);
  }
  RangeAcc total = range_empty();
  for (int64_t b = 0; b < blocks; ++b) range_merge(total, partials[2 * b], partials[2 * b + 1], 0);
  range_store(total, range2);
  return NSAMD_OK;
}

extern "C" int64_t hc_image_metrics_scratch_bytes(int64_t H, int64_t W, int32_t C) {
  if (image_metrics_check(H, W, C) != NSAMD_OK) return 0;
  return 16 * ssim_tiles(H) * ssim_tiles(W);
}

extern "C" int hc_image_metrics(const float* pred, const float* target, int64_t H, int64_t W, int32_t C, const float* range_pred,
                                const float* range_target, float data_range, float psnr_range, void* scratch, float* out4,
                                float* ssim_map) {
  const int sizes = image_metrics_check(H, W, C);
  if (sizes != NSAMD_OK) return sizes;
  if (!(pred && target && scratch && out4 && psnr_range > 0.0f)) return NSAMD_ERR_INVALID_ARG;
  if ((range_pred == nullptr) != (range_target == nullptr)) return NSAMD_ERR_INVALID_ARG;
  if (!(range_pred != nullptr || data_range > 0.0f)) return NSAMD_ERR_INVALID_ARG;
  const int64_t tiles_y = ssim_tiles(H), tiles_x = ssim_tiles(W);
  double* partials = reinterpret_cast<double*>(scratch);
  const float R = range_pred != nullptr ? ssim_data_range(range_pred, range_target) : data_range;
  float c1, c2;
  ssim_constants(R, &c1, &c2);
  for (int64_t tile = 0; tile < tiles_y * tiles_x; ++tile) {
    const SsimSpan sy = ssim_span(H, tile / tiles_x), sx = ssim_span(W, tile % tiles_x);
    // exactly-sized planes: what a tile at the image's edge does not read does not exist here
    std::vector<float> dx((size_t)sy.pixels * sx.pixels), dy(dx.size());
    std::vector<float> rows((size_t)kSsimMoments * sy.pixels * sx.windows);
    std::vector<double> ssim_acc(kLanes, 0.0), se_acc(kLanes, 0.0);
    for (int c = 0; c < C; ++c) {
      const int64_t centre = ((int64_t)(sy.first + sy.pixels / 2) * W + (sx.first + sx.pixels / 2)) * C + c;
      const float px = ssim_pivot(pred[centre]), py = ssim_pivot(target[centre]);
      for (int i = 0; i < kSsimRegion * kSsimRegion; ++i) {
        const int r = i / kSsimRegion, q = i - r * kSsimRegion;
        if (!(r < sy.pixels && q < sx.pixels)) continue;
        const int64_t g = ((int64_t)(sy.first + r) * W + (sx.first + q)) * C + c;
        if (r < sy.owned && q < sx.owned) se_acc[(size_t)(i % kLanes)] += squared_error(pred[g], target[g]);
        dx[(size_t)r * sx.pixels + q] = pred[g] - px;
        dy[(size_t)r * sx.pixels + q] = target[g] - py;
      }
      for (int r = 0; r < sy.pixels; ++r)
        for (int q = 0; q < sx.windows; ++q) {
          float m[kSsimMoments];
          ssim_row_moments(&dx[(size_t)r * sx.pixels + q], &dy[(size_t)r * sx.pixels + q], m);
          for (int k = 0; k < kSsimMoments; ++k) rows[((size_t)k * sy.pixels + r) * sx.windows + q] = m[k];
        }
      for (int i = 0; i < kTile * kTile; ++i) {
        const int wy = i / kTile, wx = i - wy * kTile;
        if (!(wy < sy.windows && wx < sx.windows)) continue;
        float M[kSsimMoments];
        for (int k = 0; k < kSsimMoments; ++k) M[k] = ssim_tap(&rows[((size_t)k * sy.pixels + wy) * sx.windows + wx], sx.windows);
        const float v = ssim_window(M, px, py, c1, c2);
        ssim_acc[(size_t)(i % kLanes)] += (double)v;
        if (ssim_map != nullptr) ssim_map[((int64_t)(sy.first + wy) * (W - kSsimHalo) + (sx.first + wx)) * C + c] = v;
      }
    }
    partials[2 * tile] = block_sum(ssim_acc.data());
    partials[2 * tile + 1] = block_sum(se_acc.data());
  }
  std::vector<double> ssim_acc(kLanes, 0.0), se_acc(kLanes, 0.0);
  for (int64_t t = 0; t < tiles_y * tiles_x; ++t) {
    ssim_acc[(size_t)(t % kLanes)] += partials[2 * t];
    se_acc[(size_t)(t % kLanes)] += partials[2 * t + 1];
  }
  image_metrics_finish(block_sum(ssim_acc.data()), block_sum(se_acc.data()), H, W, C, R, psnr_range, out4);
  return NSAMD_OK;
}

extern "C" int hc_colormap(const float* values, int64_t n, const float* lut, const float* range2, const float* accumulation,
                           nsamd_colormap_params params, float* out_rgb, uint8_t* out_u8) {
  const int args = colormap_check(n, params, values, range2, accumulation, out_rgb, out_u8);
  if (args != NSAMD_OK) return args;
  const ColormapConsts k = colormap_consts(params, range2);
  for (int64_t i = 0; i < n; ++i) {
    float rgb[3];
    colormap_pixel(k, lut, values[i], accumulation != nullptr, accumulation != nullptr ? accumulation[i] : 0.0f, rgb);
    for (int c = 0; c < 3; ++c) {
      if (out_rgb != nullptr) out_rgb[3 * i + c] = rgb[c];
      if (out_u8 != nullptr) out_u8[3 * i + c] = (uint8_t)texture_level(rgb[c]);
    }
  }
  return NSAMD_OK;
}
