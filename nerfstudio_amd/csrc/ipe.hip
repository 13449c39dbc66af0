// mip-NeRF's integrated positional encoding for gfx950: conical frustum -> Gaussian -> E[sin] rows, from rays and bin edges
// (means and covariances never touch HBM) or from explicit means and covariance diagonals. Arithmetic: ipe.h.
//
// Mapping: one workgroup = a tile of kIpeTile consecutive points. Its first lanes form one Gaussian each (mean and variance
// per axis, 24 B in LDS); after the barrier all 256 lanes walk the tile's output — kIpeTile rows of 6 F (+3) floats, one
// contiguous span of HBM — element by element, so every store instruction of a wave is 256 contiguous bytes whatever the row
// width, and a Gaussian is formed once per point instead of once per entry. The (row, column) of a lane advances by 256
// elements per step without a division. What bounds it (profiles/mipnerf_ipe.txt, 4096 x 128 samples at F = 16: 88 us, 396 B
// per sample stored and nothing read back = 2.3 TB/s): not the store stream alone. With every entry damped to zero — no sine
// evaluated, one expf and one store per entry left — the same launch takes 54 us (3.9 TB/s); the sinf of the entries the damping
// leaves alive, three quarters of a row at exponents 0 .. 16 and a pinhole's pixel area, is the rest. Forming the Gaussians is
// not measurable (explicit mode: 86 us).
#include "ipe.h"
#include "launch.h"

namespace nsamd {

constexpr int kIpeTile = 64;
constexpr int kIpeThreads = 256;

__global__ __launch_bounds__(kIpeThreads) void ipe_encode_kernel(nsamd_points P, int64_t M, const float* __restrict__ pixel_area,
                                                                const float* __restrict__ variances,
                                                                const float* __restrict__ freqs, int F, int width,
                                                                float* __restrict__ out) {
  __shared__ float g_mean[kIpeTile][3];
  __shared__ float g_var[kIpeTile][3];
  __shared__ float fr[kIpeMaxFrequencies];
  const int tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * kIpeTile;
  const int64_t left = M - p0;
  const int count = left < kIpeTile ? (int)left : kIpeTile;
  if (tid < F) fr[tid] = freqs[tid];
  if (tid < count) {
    const int64_t p = p0 + tid;
    float mean[3], var[3];
    if (P.positions != nullptr) {
      for (int k = 0; k < 3; ++k) {
        mean[k] = P.positions[3 * p + k];
        var[k] = variances[3 * p + k];
      }
    } else {
      const int64_t S = P.samples_per_ray;
      const int64_t ray = point_ray(p, S);
      const float* tb = P.t_bins + ray * (S + 1) + (p - ray * S);
      const float o[3] = {P.origins[3 * ray], P.origins[3 * ray + 1], P.origins[3 * ray + 2]};
      const float d[3] = {P.directions[3 * ray], P.directions[3 * ray + 1], P.directions[3 * ray + 2]};
      frustum_gaussian_diag(o, d, tb[0], tb[1], pixel_area[ray], mean, var);
    }
    for (int k = 0; k < 3; ++k) {
      g_mean[tid][k] = mean[k];
      g_var[tid][k] = var[k];
    }
  }
  __syncthreads();
  const int total = count * width;
  const int step_r = kIpeThreads / width, step_c = kIpeThreads - step_r * width;
  int row = tid / width, col = tid - row * width;
  float* __restrict__ o = out + p0 * width;
  for (int e = tid; e < total; e += kIpeThreads) {
    const IpeColumn c = ipe_column(F, col);
    const float m = g_mean[row][c.axis];
    o[e] = c.raw ? m : ipe_entry(m, g_var[row][c.axis], fr[c.f], c.shifted);
    row += step_r;
    col += step_c;
    if (col >= width) {
      col -= width;
      ++row;
    }
  }
}

}  // namespace nsamd

using namespace nsamd;

extern "C" int nsamd_ipe_encode(nsamd_points pts, int64_t M, const float* pixel_area, const float* variances, const float* freqs,
                                int32_t num_frequencies, int32_t include_input, float* out, nsamd_stream_t stream) {
  if (const int st = check_points(pts, M)) return st;
  if (num_frequencies <= 0 || num_frequencies > kIpeMaxFrequencies) return NSAMD_ERR_UNSUPPORTED;
  if (M == 0) return NSAMD_OK;
  NSAMD_REQUIRE(freqs != nullptr && out != nullptr);
  NSAMD_REQUIRE(pts.positions != nullptr ? variances != nullptr : pixel_area != nullptr);
  unsigned blocks;
  if (grid_blocks((M + kIpeTile - 1) / kIpeTile, &blocks)) return NSAMD_ERR_UNSUPPORTED;
  const int width = 6 * num_frequencies + (include_input ? 3 : 0);
  ipe_encode_kernel<<<blocks, kIpeThreads, 0, (hipStream_t)stream>>>(pts, M, pixel_area, variances, freqs, num_frequencies, width,
                                                                   out);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}
