// Host build of nerfstudio_amd/csrc/ipe.h for tests/test_mipnerf_cpu.py: the per-sample arithmetic nsamd_ipe_encode runs per lane,
// looped over rays, samples and columns the way the kernel composes it (one Gaussian per point, then every column of its row).
// Test infrastructure: the product never loads it.
#include "../../nerfstudio_amd/csrc/ipe.h"

using namespace nsamd;

static void write_row(const float mean[3], const float var[3], const float* freqs, int F, int width, float* row) {
  for (int col = 0; col < width; ++col) {
    const IpeColumn c = ipe_column(F, col);
    row[col] = c.raw ? mean[c.axis] : ipe_entry(mean[c.axis], var[c.axis], freqs[c.f], c.shifted);
  }
}

// Ray mode: out [n * S, 6 F (+3)]; means / variances [n * S, 3] (nullable) = the Gaussians the rows were formed from.
extern "C" int hc_ipe_rays(const float* origins, const float* directions, const float* t_bins, const float* pixel_area, int64_t n,
                           int S, const float* freqs, int F, int include_input, float* out, float* means, float* variances) {
  if (F <= 0 || F > kIpeMaxFrequencies) return -2;
  const int width = 6 * F + (include_input ? 3 : 0);
  for (int64_t r = 0; r < n; ++r)
    for (int s = 0; s < S; ++s) {
      const int64_t p = r * S + s;
      const float* tb = t_bins + r * (S + 1) + s;
      float mean[3], var[3];
      frustum_gaussian_diag(origins + 3 * r, directions + 3 * r, tb[0], tb[1], pixel_area[r], mean, var);
      for (int k = 0; k < 3; ++k) {
        if (means) means[3 * p + k] = mean[k];
        if (variances) variances[3 * p + k] = var[k];
      }
      write_row(mean, var, freqs, F, width, out + p * width);
    }
  return 0;
}

// Explicit mode: means / variances [M, 3] -> out [M, 6 F (+3)].
extern "C" int hc_ipe_explicit(const float* means, const float* variances, int64_t M, const float* freqs, int F, int include_input,
                               float* out) {
  if (F <= 0 || F > kIpeMaxFrequencies) return -2;
  const int width = 6 * F + (include_input ? 3 : 0);
  for (int64_t p = 0; p < M; ++p) write_row(means + 3 * p, variances + 3 * p, freqs, F, width, out + p * width);
  return 0;
}
