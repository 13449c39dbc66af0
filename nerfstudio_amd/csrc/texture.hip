// Texture export (include/nsamd_texture.h): nsamd_texel_rays / nsamd_mesh_raylen / nsamd_texture_store. Where the reference
// gathers [H,W,3,3] vertices and normals and [H,W,3,2] texture coordinates to form one ray per texel
// (exporter/texture_utils.py:170-206, more than 100 B per texel), a lane here finds its triangle and its weights from the
// texel's index and writes the ray straight into the eval loop's input buffers: 32 B written per texel, the mesh read through
// the cache (the texels of a square share two faces). The per-texel arithmetic is texture.h.
#include "launch.h"
#include "texture.h"
#include "wave.h"

using namespace nsamd;

namespace {

constexpr int kTexThreads = NSAMD_TEXTURE_BLOCK;  // four wavefronts
constexpr int kTexWaves = kTexThreads / 64;

// One lane per row of the outputs; row i holds texel first + min(i, count - 1). The workgroup's 256 x 3 floats of origins and of
// directions meet in LDS (a lane's three words at stride 3: no bank conflict) and leave as three sweeps of consecutive words,
// 256 contiguous bytes per wavefront and store instruction. No lane returns before the barrier.
__global__ __launch_bounds__(kTexThreads) void texel_rays_kernel(nsamd_texel_atlas atlas, int64_t width,
                                                                 const float* __restrict__ vertices,
                                                                 const float* __restrict__ normals,
                                                                 const int32_t* __restrict__ faces, int64_t V,
                                                                 const float* __restrict__ raylen_dev, int64_t first, int64_t count,
                                                                 int64_t rows, float* __restrict__ origins,
                                                                 float* __restrict__ directions, float* __restrict__ nears,
                                                                 float* __restrict__ fars) {
  __shared__ float stage[2][3 * kTexThreads];
  const int64_t base = (int64_t)blockIdx.x * kTexThreads;
  const int64_t row = base + threadIdx.x;
  const float raylen = raylen_dev[0];
  if (row < rows) {
    float o[3], d[3];
    texel_ray(atlas, width, vertices, normals, faces, V, raylen, first + (row < count ? row : count - 1), o, d);
    for (int c = 0; c < 3; ++c) stage[0][3 * threadIdx.x + c] = o[c], stage[1][3 * threadIdx.x + c] = d[c];
    nears[row] = 0.0f;
    fars[row] = raylen;
  }
  __syncthreads();
  const int64_t words = 3 * (rows - base < kTexThreads ? rows - base : (int64_t)kTexThreads);
  for (int k = 0; k < 3; ++k) {
    const int i = k * kTexThreads + threadIdx.x;
    if (i < words) origins[3 * base + i] = stage[0][i], directions[3 * base + i] = stage[1][i];
  }
}

// workgroup b: faces b * 256 + lane, then every gridDim.x * 256 further, per lane in ascending order
__global__ __launch_bounds__(kTexThreads) void raylen_partial_kernel(const float* __restrict__ vertices, int64_t V,
                                                                     const int32_t* __restrict__ faces, int64_t T,
                                                                     double* __restrict__ partials) {
  double acc = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * kTexThreads + threadIdx.x; t < T; t += (int64_t)gridDim.x * kTexThreads)
    acc += raylen_edge(vertices, V, faces, t);
  const double total = block_sum_f64<kTexWaves>(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// ONE workgroup: the partial sums in the same fixed order, then the one rounding
__global__ __launch_bounds__(kTexThreads) void raylen_finish_kernel(const double* __restrict__ partials, int blocks, int64_t T,
                                                                    float* __restrict__ raylen_dev) {
  double acc = 0.0;
  for (int b = threadIdx.x; b < blocks; b += kTexThreads) acc += partials[b];
  const double total = block_sum_f64<kTexWaves>(acc);
  if (threadIdx.x == 0) raylen_dev[0] = raylen_finish(total, T);
}

// One lane per aligned 32-bit word of the destination bytes [begin, begin + bytes) of the atlas: byte j of the range is
// channel j mod 3 of row j div 3 of rgb, i.e. rgb[j].
__global__ __launch_bounds__(kTexThreads) void texture_store_kernel(const float* __restrict__ rgb, int64_t bytes, int head,
                                                                    uint8_t* __restrict__ aligned) {
  // `aligned` is the destination rounded down to 4 bytes, `head` (0-3) the bytes of its first word before the range
  const int64_t word = (int64_t)blockIdx.x * kTexThreads + threadIdx.x;
  const int64_t j0 = 4 * word - head;  // index into rgb of the word's first byte
  if (j0 >= bytes) return;
  if (j0 >= 0 && j0 + 4 <= bytes) {
    const uint32_t packed = texture_level(rgb[j0]) | (texture_level(rgb[j0 + 1]) << 8) | (texture_level(rgb[j0 + 2]) << 16) |
                            (texture_level(rgb[j0 + 3]) << 24);
    reinterpret_cast<uint32_t*>(aligned)[word] = packed;
    return;
  }
  for (int b = 0; b < 4; ++b) {
    const int64_t j = j0 + b;
    if (j >= 0 && j < bytes) aligned[4 * word + b] = (uint8_t)texture_level(rgb[j]);
  }
}

}  // namespace

extern "C" int nsamd_texel_rays(nsamd_texel_atlas atlas, const float* vertices, const float* normals, const int32_t* faces,
                                int64_t V, const float* raylen_dev, int64_t first, int64_t count, int64_t rows, float* origins,
                                float* directions, float* nears, float* fars, nsamd_stream_t stream) {
  int64_t width = 0, height = 0;
  const int sizes = texel_atlas_check(atlas, &width, &height);
  if (sizes != NSAMD_OK) return sizes;
  const int range = texel_range_check(width * height, first, count, rows);
  if (range != NSAMD_OK) return range;
  if (rows == 0) return NSAMD_OK;
  NSAMD_REQUIRE(V >= 1 && vertices && normals && faces && raylen_dev && origins && directions && nears && fars);
  unsigned blocks = 0;
  const int status = grid_blocks((rows + kTexThreads - 1) / kTexThreads, &blocks);
  if (status != NSAMD_OK) return status;
  texel_rays_kernel<<<blocks, kTexThreads, 0, (hipStream_t)stream>>>(atlas, width, vertices, normals, faces, V, raylen_dev, first,
                                                                     count, rows, origins, directions, nears, fars);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int nsamd_mesh_raylen(const float* vertices, int64_t V, const int32_t* faces, int64_t T, void* scratch,
                                 float* raylen_dev, nsamd_stream_t stream) {
  const int sizes = raylen_check(V, T);
  if (sizes != NSAMD_OK) return sizes;
  NSAMD_REQUIRE(vertices && faces && scratch && raylen_dev);
  const int blocks = (int)raylen_blocks(T);
  hipStream_t s = (hipStream_t)stream;
  raylen_partial_kernel<<<blocks, kTexThreads, 0, s>>>(vertices, V, faces, T, reinterpret_cast<double*>(scratch));
  NSAMD_CHECK_LAUNCH();
  raylen_finish_kernel<<<1, kTexThreads, 0, s>>>(reinterpret_cast<const double*>(scratch), blocks, T, raylen_dev);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int nsamd_texture_store(const float* rgb, int64_t count, int64_t first, uint8_t* atlas_u8, nsamd_stream_t stream) {
  NSAMD_REQUIRE(count >= 0 && count <= 0x7fffffffLL && first >= 0 && first <= (int64_t)0x7fffffffffffffffLL / 4);
  if (count == 0) return NSAMD_OK;
  NSAMD_REQUIRE(rgb && atlas_u8);
  uint8_t* const begin = atlas_u8 + 3 * first;
  const int head = (int)(reinterpret_cast<uintptr_t>(begin) & 3u);
  const int64_t bytes = 3 * count, words = (bytes + head + 3) / 4;
  unsigned blocks = 0;
  const int status = grid_blocks((words + kTexThreads - 1) / kTexThreads, &blocks);
  if (status != NSAMD_OK) return status;
  texture_store_kernel<<<blocks, kTexThreads, 0, (hipStream_t)stream>>>(rgb, bytes, head, begin - head);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}
