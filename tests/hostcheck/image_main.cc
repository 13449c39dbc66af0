// Stand-alone program over tests/hostcheck/image_helpers.cc, built by tests/test_image_metrics_cpu.py with
// -fsanitize=address,undefined and run once per image size: memory and arithmetic of the host build of csrc/image_metrics.h
// under the sanitizers, with exactly-sized heap buffers so that a halo pixel, a window or a partial sum past an end is caught.
//   image_main <images.bin> <H> <W> <C>
// reads H * W * C floats of the prediction and as many of the target, takes both ranges, measures the pair with the ranges and
// with data_range = 1, with and without the per-window map, requires the same bits, colours channel 0 in every mode into
// exactly-sized outputs, and prints "windows <n> mse <%.9g> psnr <%.9g> ssim <%.9g> range <%.9g>". Exit status 0 when
// everything agreed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/nsamd_image.h"

extern "C" {
int hc_image_range(const float*, int64_t, void*, float*);
int64_t hc_image_metrics_scratch_bytes(int64_t, int64_t, int32_t);
int hc_image_metrics(const float*, const float*, int64_t, int64_t, int32_t, const float*, const float*, float, float, void*, float*,
                     float*);
int hc_colormap(const float*, int64_t, const float*, const float*, const float*, nsamd_colormap_params, float*, uint8_t*);
}

#define REQUIRE(cond)                                                 \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main(int argc, char** argv) {
  REQUIRE(argc == 5);
  const int64_t H = std::atoll(argv[2]), W = std::atoll(argv[3]);
  const int32_t C = std::atoi(argv[4]);
  REQUIRE(H >= NSAMD_SSIM_WINDOW && W >= NSAMD_SSIM_WINDOW && C >= 1 && C <= 4);
  const size_t n = (size_t)(H * W * C);
  std::vector<float> pred(n), target(n);
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f != nullptr);
  REQUIRE(std::fread(pred.data(), sizeof(float), n, f) == n);
  REQUIRE(std::fread(target.data(), sizeof(float), n, f) == n);
  std::fclose(f);

  std::vector<float> range_scratch(NSAMD_RANGE_SCRATCH_BYTES / 4);
  std::vector<float> range_pred(2), range_target(2);
  REQUIRE(hc_image_range(pred.data(), (int64_t)n, range_scratch.data(), range_pred.data()) == 0);
  REQUIRE(hc_image_range(target.data(), (int64_t)n, range_scratch.data(), range_target.data()) == 0);
  REQUIRE(range_pred[0] <= range_pred[1] && range_target[0] <= range_target[1]);
  REQUIRE(hc_image_range(pred.data(), 0, range_scratch.data(), range_pred.data()) == NSAMD_ERR_INVALID_ARG);

  const int64_t bytes = hc_image_metrics_scratch_bytes(H, W, C);
  REQUIRE(bytes >= 16 && bytes % 16 == 0);
  REQUIRE(hc_image_metrics_scratch_bytes(H, NSAMD_SSIM_WINDOW - 1, C) == 0 && hc_image_metrics_scratch_bytes(H, W, 5) == 0);
  std::vector<double> scratch((size_t)bytes / 8);
  const int64_t windows = (H - 10) * (W - 10) * C;
  std::vector<float> map((size_t)windows, -7.0f), out(4), again(4);
  REQUIRE(hc_image_metrics(pred.data(), target.data(), H, W, C, range_pred.data(), range_target.data(), 0.0f, 1.0f, scratch.data(),
                           out.data(), map.data()) == 0);
  REQUIRE(hc_image_metrics(pred.data(), target.data(), H, W, C, range_pred.data(), range_target.data(), 0.0f, 1.0f, scratch.data(),
                           again.data(), nullptr) == 0);
  REQUIRE(std::memcmp(out.data(), again.data(), 4 * sizeof(float)) == 0);
  double sum = 0.0;
  for (int64_t i = 0; i < windows; ++i) {
    REQUIRE(map[(size_t)i] >= -1.0001f && map[(size_t)i] <= 1.0001f);
    sum += map[(size_t)i];
  }
  REQUIRE(std::fabs(sum / (double)windows - (double)out[2]) < 1e-6);
  REQUIRE(hc_image_metrics(pred.data(), target.data(), H, W, C, nullptr, nullptr, 1.0f, 1.0f, scratch.data(), again.data(), nullptr) == 0);
  REQUIRE(again[3] == 1.0f && std::memcmp(again.data(), out.data(), 2 * sizeof(float)) == 0);  // mse and psnr do not depend on R
  REQUIRE(hc_image_metrics(pred.data(), target.data(), H, W, C, nullptr, nullptr, 0.0f, 1.0f, scratch.data(), again.data(), nullptr) ==
          NSAMD_ERR_INVALID_ARG);
  REQUIRE(hc_image_metrics(pred.data(), target.data(), 10, W, C, nullptr, nullptr, 1.0f, 1.0f, scratch.data(), again.data(), nullptr) ==
          NSAMD_ERR_INVALID_ARG);

  // the colormaps of channel 0 of the prediction, every mode, exactly-sized outputs
  const int64_t pixels = H * W;
  std::vector<float> depth((size_t)pixels), acc((size_t)pixels), lut(256 * 3), rgb((size_t)pixels * 3), range(2);
  std::vector<uint8_t> u8((size_t)pixels * 3);
  for (int64_t i = 0; i < pixels; ++i) depth[(size_t)i] = 4.0f * pred[(size_t)(i * C)] - 1.0f, acc[(size_t)i] = (float)(i % 11) / 10.0f;
  depth[0] = NAN;  // a NaN depth colours as row 0; the range is NaN, so it is taken from the finite rest
  for (int i = 0; i < 256 * 3; ++i) lut[(size_t)i] = (float)(i / 3) / 255.0f;
  REQUIRE(hc_image_range(depth.data() + 1, pixels - 1, range_scratch.data(), range.data()) == 0);
  for (int mode = 0; mode < 2; ++mode)
    for (int variant = 0; variant < 8; ++variant) {
      nsamd_colormap_params p = {mode, variant & 1, (variant >> 1) & 1, (variant >> 2) ? 3 : 0, 0.1, 0.9, 0.25, 2.5};
      const bool with_acc = mode == NSAMD_COLORMAP_DEPTH && (variant & 2);
      REQUIRE(hc_colormap(depth.data(), pixels, (variant & 4) ? nullptr : lut.data(), range.data(), with_acc ? acc.data() : nullptr, p,
                          rgb.data(), u8.data()) == 0);
      for (size_t i = 0; i < rgb.size(); ++i) REQUIRE(rgb[i] >= 0.0f && rgb[i] <= 1.0f && u8[i] == (uint8_t)(rgb[i] * 255.0f + 0.5f));
    }
  nsamd_colormap_params plain = {NSAMD_COLORMAP_PLAIN, 0, 0, 0, 0.0, 1.0, 0.0, 0.0};
  REQUIRE(hc_colormap(depth.data(), pixels, lut.data(), nullptr, nullptr, plain, nullptr, nullptr) == NSAMD_ERR_INVALID_ARG);
  REQUIRE(hc_colormap(depth.data(), 0, lut.data(), nullptr, nullptr, plain, rgb.data(), nullptr) == NSAMD_ERR_INVALID_ARG);
  REQUIRE(hc_colormap(depth.data(), pixels, lut.data(), nullptr, nullptr, plain, rgb.data(), nullptr) == 0);
  plain.normalize = 1;
  REQUIRE(hc_colormap(depth.data(), pixels, lut.data(), nullptr, nullptr, plain, rgb.data(), nullptr) == NSAMD_ERR_INVALID_ARG);
  std::printf("windows %lld mse %.9g psnr %.9g ssim %.9g range %.9g\n", (long long)windows, (double)out[0], (double)out[1],
              (double)out[2], (double)out[3]);
  return 0;
}
