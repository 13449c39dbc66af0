// Per-window and per-pixel arithmetic of the eval image metrics and colormaps (gfx950; the host compiler sees it only through
// tests/hostcheck): the 11-tap Gaussian sums, a window's SSIM from its five moments about the tile's pivot, the tile geometry,
// the results' one rounding, the min / max fold and a pixel's colour, as include/nsamd_image.h defines them. The fp32 operation
// order is stated HERE, once, for the kernels and the host build of the tests; the library is built with -ffp-contract=off.
#pragma once

#include "common.h"
#include "texture.h"
#include "../../include/nsamd_image.h"

namespace nsamd {

constexpr int kSsimTaps = NSAMD_SSIM_WINDOW;
constexpr int kSsimHalo = kSsimTaps - 1;                  // 10: a tile of T windows reads T + 10 pixels per axis
constexpr int kSsimRegion = NSAMD_SSIM_TILE + kSsimHalo;  // 42
constexpr int kSsimMoments = 5;                           // E[dx], E[dy], E[dx dx], E[dy dy], E[dx dy]

// exp(-(d / 1.5)^2 / 2), d = -5 .. 5, over their sum: formed in fp64, rounded once to fp32
#define NSAMD_SSIM_WEIGHTS                                                                                                     \
  {0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f, 0.213005543f, 0.109360687f, \
   0.0360007733f, 0.00759875821f, 0.00102838012f}

// ---- argument limits and geometry, shared by the entry points and the host build of the tests (no HIP runtime call) -------------
NSAMD_HD int image_metrics_check(int64_t H, int64_t W, int32_t C) {
  if (C < 1 || C > 4 || H < kSsimTaps || W < kSsimTaps) return NSAMD_ERR_INVALID_ARG;
  return (H > 0x7fffffffLL / W || H * W > 0x7fffffffLL / C) ? NSAMD_ERR_INVALID_ARG : NSAMD_OK;
}

NSAMD_HD int64_t ssim_tiles(int64_t side) { return (side - kSsimHalo + NSAMD_SSIM_TILE - 1) / NSAMD_SSIM_TILE; }  // side >= 11

NSAMD_HD int image_range_check(int64_t n) { return n < 1 ? NSAMD_ERR_INVALID_ARG : NSAMD_OK; }

NSAMD_HD int64_t image_range_blocks(int64_t n) {
  const int64_t b = (n + NSAMD_IMAGE_BLOCK - 1) / NSAMD_IMAGE_BLOCK;
  return b < NSAMD_RANGE_MAX_BLOCKS ? b : NSAMD_RANGE_MAX_BLOCKS;
}

// One tile along one axis: its first pixel / window, the windows it holds, the pixels it reads and the pixels it OWNS for the
// squared error — its T, and for the last tile everything up to the image's edge (inside what it reads): every pixel once.
struct SsimSpan {
  int first, windows, pixels, owned;
};
NSAMD_HD SsimSpan ssim_span(int64_t side, int64_t tile) {
  SsimSpan s;
  s.first = (int)(tile * NSAMD_SSIM_TILE);
  const int64_t left = side - kSsimHalo - s.first;
  s.windows = left < NSAMD_SSIM_TILE ? (int)left : NSAMD_SSIM_TILE;
  s.pixels = s.windows + kSsimHalo;
  s.owned = tile == ssim_tiles(side) - 1 ? s.pixels : NSAMD_SSIM_TILE;
  return s;
}

// the pivot of a tile: the pixel in the middle of what it reads, 0 where that is not finite (a pivot only has to be tile-constant)
NSAMD_HD float ssim_pivot(float centre) { return (centre - centre == 0.0f) ? centre : 0.0f; }

// ---- the two passes -------------------------------------------------------------------------------------------------------------
// sum_j g[j] v[j stride], j ascending
NSAMD_HD float ssim_tap(const float* v, int stride) {
  const float g[kSsimTaps] = NSAMD_SSIM_WEIGHTS;
  float acc = g[0] * v[0];
  for (int j = 1; j < kSsimTaps; ++j) acc = acc + g[j] * v[j * stride];
  return acc;
}

// the five row sums at one pixel from 11 consecutive dx = x - p_x and dy = y - p_y
NSAMD_HD void ssim_row_moments(const float* dx, const float* dy, float* m) {
  const float g[kSsimTaps] = NSAMD_SSIM_WEIGHTS;
  float a[kSsimMoments] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int j = 0; j < kSsimTaps; ++j) {
    const float x = dx[j], y = dy[j];
    const float t[kSsimMoments] = {x, y, x * x, y * y, x * y};
    for (int k = 0; k < kSsimMoments; ++k) a[k] = j == 0 ? g[0] * t[k] : a[k] + g[j] * t[k];
  }
  for (int k = 0; k < kSsimMoments; ++k) m[k] = a[k];
}

NSAMD_HD void ssim_constants(float R, float* c1, float* c2) {
  const double a = 0.01 * (double)R, b = 0.03 * (double)R;
  *c1 = (float)(a * a);
  *c2 = (float)(b * b);
}

// R of two {min, max} pairs, as the library forms it in fp32
NSAMD_HD float ssim_data_range(const float* range_pred, const float* range_target) {
  const float a = range_pred[1] - range_pred[0], b = range_target[1] - range_target[0];
  return (a != a || b != b) ? a + b : fmaxf(a, b);
}

// a window's value from its five moments about (px, py)
NSAMD_HD float ssim_window(const float* M, float px, float py, float c1, float c2) {
  const float mu_x = px + M[0], mu_y = py + M[1];
  const float s_xx = fmaxf(M[2] - M[0] * M[0], 0.0f), s_yy = fmaxf(M[3] - M[1] * M[1], 0.0f);
  const float s_xy = M[4] - M[0] * M[1];
  const float upper = (2.0f * mu_x * mu_y + c1) * (2.0f * s_xy + c2);
  const float lower = ((mu_x * mu_x + mu_y * mu_y) + c1) * ((s_xx + s_yy) + c2);
  const float v = upper / lower;
  // fmaxf drops a NaN moment: a window over a NaN pixel is NaN whatever the clamp did
  return (M[2] != M[2] || M[3] != M[3]) ? M[2] + M[3] : v;
}

// (x - y)^2 in fp64: the difference of two fp32 values is exact there
NSAMD_HD double squared_error(float x, float y) {
  const double d = (double)x - (double)y;
  return d * d;
}

// out4 = {mse, psnr, ssim, R}: the one rounding of each
NSAMD_HD void image_metrics_finish(double ssim_sum, double se_sum, int64_t H, int64_t W, int32_t C, float R, float psnr_range,
                                   float* out4) {
  const double mse = se_sum / (double)(H * W * C);
  out4[0] = (float)mse;
  out4[1] = (float)(10.0 * log10((double)psnr_range * (double)psnr_range / mse));
  out4[2] = (float)(ssim_sum / (double)((H - kSsimHalo) * (W - kSsimHalo) * C));
  out4[3] = R;
}

// ---- minimum and maximum --------------------------------------------------------------------------------------------------------
struct RangeAcc {
  float lo, hi;
  int nan;
};
NSAMD_HD RangeAcc range_empty() { return RangeAcc{INFINITY, -INFINITY, 0}; }
NSAMD_HD void range_fold(RangeAcc& a, float v) {
  a.lo = fminf(a.lo, v);  // fminf / fmaxf drop a NaN: the flag carries it
  a.hi = fmaxf(a.hi, v);
  a.nan |= (v != v) ? 1 : 0;
}
NSAMD_HD void range_merge(RangeAcc& a, float lo, float hi, int nan) {
  a.lo = fminf(a.lo, lo);
  a.hi = fmaxf(a.hi, hi);
  a.nan |= nan | ((lo != lo || hi != hi) ? 1 : 0);
}
NSAMD_HD void range_store(const RangeAcc& a, float* out2) {
  out2[0] = a.nan ? NAN : a.lo;
  out2[1] = a.nan ? NAN : a.hi;
}

// ---- the colormap ---------------------------------------------------------------------------------------------------------------
NSAMD_HD int colormap_check(int64_t n, const nsamd_colormap_params& p, const void* values, const void* range2,
                            const void* accumulation, const void* out_rgb, const void* out_u8) {
  if (n < 1 || n > 0x7fffffffLL || values == nullptr || (out_rgb == nullptr && out_u8 == nullptr)) return NSAMD_ERR_INVALID_ARG;
  if (p.mode != NSAMD_COLORMAP_PLAIN && p.mode != NSAMD_COLORMAP_DEPTH) return NSAMD_ERR_INVALID_ARG;
  if (p.mode == NSAMD_COLORMAP_PLAIN && accumulation != nullptr) return NSAMD_ERR_INVALID_ARG;
  const bool both = (p.fixed & NSAMD_COLORMAP_FIXED_NEAR) && (p.fixed & NSAMD_COLORMAP_FIXED_FAR);
  const bool needs_range = p.normalize != 0 || (p.mode == NSAMD_COLORMAP_DEPTH && !both);
  return (needs_range && range2 == nullptr) ? NSAMD_ERR_INVALID_ARG : NSAMD_OK;
}

// torch.clip(t, 0, 1) on the CPU: min(max(t, 0), 1) by comparisons — a NaN and -0.0 pass through
NSAMD_HD float clip_unit(float t) { return t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t); }

// the constants of one launch: everything of THE COLORMAP that does not depend on the pixel
struct ColormapConsts {
  int depth, normalize, invert;
  float near_plane, width;  // depth mode: t = (v - near_plane) / width
  float lo, den;            // normalize: t = (t - lo) / den
  float scale, offset;
};
NSAMD_HD float colormap_depth_unit(const ColormapConsts& k, float v) { return clip_unit((v - k.near_plane) / k.width); }

// range2: the {min, max} of the values (read only where colormap_check asks for it)
NSAMD_HD ColormapConsts colormap_consts(const nsamd_colormap_params& p, const float* range2) {
  ColormapConsts k;
  k.depth = p.mode == NSAMD_COLORMAP_DEPTH;
  k.normalize = p.normalize != 0;
  k.invert = p.invert != 0;
  k.near_plane = 0.0f, k.width = 1.0f, k.lo = 0.0f, k.den = 1.0f;
  const bool fixed_near = (p.fixed & NSAMD_COLORMAP_FIXED_NEAR) != 0, fixed_far = (p.fixed & NSAMD_COLORMAP_FIXED_FAR) != 0;
  const bool reads = k.normalize || (k.depth && !(fixed_near && fixed_far));
  const float vmin = reads ? range2[0] : 0.0f, vmax = reads ? range2[1] : 0.0f;
  if (k.depth) {
    const double near_d = fixed_near ? p.near_plane : (double)vmin, far_d = fixed_far ? p.far_plane : (double)vmax;
    k.near_plane = (float)near_d;
    k.width = (float)(far_d - near_d + 1e-10);
  }
  if (k.normalize) {
    const float hi = k.depth ? colormap_depth_unit(k, vmax) : vmax;
    k.lo = k.depth ? colormap_depth_unit(k, vmin) : vmin;
    k.den = (hi - k.lo) + 1e-9f;
  }
  k.scale = (float)(p.colormap_max - p.colormap_min);
  k.offset = (float)p.colormap_min;
  return k;
}

// the value in [0, 1] that indexes the table
NSAMD_HD float colormap_unit(const ColormapConsts& k, float v) {
  float t = k.depth ? colormap_depth_unit(k, v) : v;
  if (k.normalize) t = (t - k.lo) / k.den;
  t = t * k.scale + k.offset;
  t = clip_unit(t);
  if (k.invert) t = 1.0f - t;
  return t != t ? 0.0f : t;
}

// rgb[3] of one pixel; lut NULL = "gray"; acc: the pixel's accumulation (has_acc) for depth mode's white blend
NSAMD_HD void colormap_pixel(const ColormapConsts& k, const float* lut, float v, bool has_acc, float acc, float* rgb) {
  const float t = colormap_unit(k, v);
  const int row = (int)(t * 255.0f);  // truncation; t in [0, 1]
  for (int c = 0; c < 3; ++c) {
    const float colour = lut != nullptr ? lut[3 * row + c] : t;
    rgb[c] = has_acc ? colour * acc + (1.0f - acc) : colour;
  }
}

}  // namespace nsamd
