// Host build of nerfstudio_amd/csrc/texture.h for tests/test_texture_cpu.py (and tests/hostcheck/texture_main.cc): the per-texel
// arithmetic of the texture entry points, looped the way the kernels compose it — one row per lane, rows past `count` repeating
// the last texel; the edge lengths summed per lane, per wavefront butterfly, per workgroup and by the finishing workgroup in
// the kernels' order; the destination bytes of the image word by word. Host memory in place of device memory; the argument
// checks are the entry points' own (texture.h). Test infrastructure: the product never loads it.
#include <vector>

#include "../../nerfstudio_amd/csrc/texture.h"

using namespace nsamd;

namespace {

// the sum of one workgroup's 256 lane values as block_sum_f64 forms it: a butterfly per wavefront, the wavefronts in order
double block_sum(const double* lanes) {
  double total = 0.0;
  for (int w = 0; w < NSAMD_TEXTURE_BLOCK / 64; ++w) {
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

extern "C" int hc_texel_rays(nsamd_texel_atlas atlas, const float* vertices, const float* normals, const int32_t* faces, int64_t V,
                             const float* raylen_dev, int64_t first, int64_t count, int64_t rows, float* origins,
                             float* directions, float* nears, float* fars) {
  int64_t width = 0, height = 0;
  const int sizes = texel_atlas_check(atlas, &width, &height);
  if (sizes != NSAMD_OK) return sizes;
  const int range = texel_range_check(width * height, first, count, rows);
  if (range != NSAMD_OK) return range;
  if (rows == 0) return NSAMD_OK;
  if (!(V >= 1 && vertices && normals && faces && raylen_dev && origins && directions && nears && fars)) return NSAMD_ERR_INVALID_ARG;
  const float raylen = raylen_dev[0];
  for (int64_t row = 0; row < rows; ++row) {
    texel_ray(atlas, width, vertices, normals, faces, V, raylen, first + (row < count ? row : count - 1), origins + 3 * row,
              directions + 3 * row);
    nears[row] = 0.0f;
    fars[row] = raylen;
  }
  return NSAMD_OK;
}

extern "C" int hc_mesh_raylen(const float* vertices, int64_t V, const int32_t* faces, int64_t T, void* scratch, float* raylen_dev) {
  const int sizes = raylen_check(V, T);
  if (sizes != NSAMD_OK) return sizes;
  if (!(vertices && faces && scratch && raylen_dev)) return NSAMD_ERR_INVALID_ARG;
  const int64_t blocks = raylen_blocks(T);
  double* partials = reinterpret_cast<double*>(scratch);
  std::vector<double> lanes(NSAMD_TEXTURE_BLOCK);
  for (int64_t b = 0; b < blocks; ++b) {
    for (int l = 0; l < NSAMD_TEXTURE_BLOCK; ++l) {
      double acc = 0.0;
      for (int64_t t = b * NSAMD_TEXTURE_BLOCK + l; t < T; t += blocks * NSAMD_TEXTURE_BLOCK) acc += raylen_edge(vertices, V, faces, t);
      lanes[(size_t)l] = acc;
    }
    partials[b] = block_sum(lanes.data());
  }
  for (int l = 0; l < NSAMD_TEXTURE_BLOCK; ++l) {
    double acc = 0.0;
    for (int64_t b = l; b < blocks; b += NSAMD_TEXTURE_BLOCK) acc += partials[b];
    lanes[(size_t)l] = acc;
  }
  raylen_dev[0] = raylen_finish(block_sum(lanes.data()), T);
  return NSAMD_OK;
}

extern "C" int hc_texture_store(const float* rgb, int64_t count, int64_t first, uint8_t* atlas_u8) {
  if (!(count >= 0 && count <= 0x7fffffffLL && first >= 0 && first <= (int64_t)0x7fffffffffffffffLL / 4)) return NSAMD_ERR_INVALID_ARG;
  if (count == 0) return NSAMD_OK;
  if (!(rgb && atlas_u8)) return NSAMD_ERR_INVALID_ARG;
  uint8_t* const begin = atlas_u8 + 3 * first;
  const int head = (int)(reinterpret_cast<uintptr_t>(begin) & 3u);
  const int64_t bytes = 3 * count, words = (bytes + head + 3) / 4;
  for (int64_t word = 0; word < words; ++word)
    for (int b = 0; b < 4; ++b) {
      const int64_t j = 4 * word - head + b;
      if (j >= 0 && j < bytes) begin[j] = (uint8_t)texture_level(rgb[j]);
    }
  return NSAMD_OK;
}
