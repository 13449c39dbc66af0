// Stand-alone program over tests/hostcheck/texture_helpers.cc, built by tests/test_texture_cpu.py with
// -fsanitize=address,undefined and run once per mesh: memory and arithmetic of the host build of csrc/texture.h under the
// sanitizers, with exactly-sized heap buffers so that a row, a face or a byte past an end is caught.
//   texture_main <mesh.bin> <V> <F> <P> <sw> <sh>
// reads V * 3 floats of vertices, V * 3 of normals and F * 3 int32 of faces (some of which may lie outside [0, V): they are
// clamped), renders every texel in one call and again in chunks of 37 rows padded to 64, requires the same bytes, the padding
// rows to repeat the last texel, every direction to be a unit vector or zero, sums the ray length twice, stores an image at an
// odd row offset between guard bytes, and prints "texels <W H> raylen <%.9g>". Exit status 0 when everything agreed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/nsamd_texture.h"

extern "C" {
int hc_texel_rays(nsamd_texel_atlas, const float*, const float*, const int32_t*, int64_t, const float*, int64_t, int64_t, int64_t,
                  float*, float*, float*, float*);
int hc_mesh_raylen(const float*, int64_t, const int32_t*, int64_t, void*, float*);
int hc_texture_store(const float*, int64_t, int64_t, uint8_t*);
}

#define REQUIRE(cond)                                                 \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main(int argc, char** argv) {
  REQUIRE(argc == 7);
  const int64_t V = std::atoll(argv[2]), F = std::atoll(argv[3]);
  const nsamd_texel_atlas atlas = {(int32_t)F, std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6])};
  REQUIRE(V > 0 && F > 0);
  std::vector<float> vertices((size_t)V * 3), normals((size_t)V * 3);
  std::vector<int32_t> faces((size_t)F * 3);
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f != nullptr);
  REQUIRE(std::fread(vertices.data(), sizeof(float), vertices.size(), f) == vertices.size());
  REQUIRE(std::fread(normals.data(), sizeof(float), normals.size(), f) == normals.size());
  REQUIRE(std::fread(faces.data(), sizeof(int32_t), faces.size(), f) == faces.size());
  std::fclose(f);

  std::vector<double> scratch(NSAMD_RAYLEN_SCRATCH_BYTES / 8);
  float raylen = -1.0f, again = -2.0f;
  REQUIRE(hc_mesh_raylen(vertices.data(), V, faces.data(), F, scratch.data(), &raylen) == 0);
  REQUIRE(hc_mesh_raylen(vertices.data(), V, faces.data(), F, scratch.data(), &again) == 0);
  REQUIRE(std::memcmp(&raylen, &again, sizeof(float)) == 0 && raylen >= 0.0f);
  REQUIRE(hc_mesh_raylen(vertices.data(), V, faces.data(), 0, scratch.data(), &again) == NSAMD_ERR_INVALID_ARG);

  const int64_t texels = (int64_t)atlas.squares_w * (atlas.px + 3) * atlas.squares_h * atlas.px;
  std::vector<float> o((size_t)texels * 3), d((size_t)texels * 3), nr((size_t)texels), fr((size_t)texels);
  REQUIRE(hc_texel_rays(atlas, vertices.data(), normals.data(), faces.data(), V, &raylen, 0, texels, texels, o.data(), d.data(),
                        nr.data(), fr.data()) == 0);
  for (int64_t i = 0; i < texels; ++i) {
    const double n = std::sqrt((double)d[3 * i] * d[3 * i] + (double)d[3 * i + 1] * d[3 * i + 1] + (double)d[3 * i + 2] * d[3 * i + 2]);
    REQUIRE(n == 0.0 || std::fabs(n - 1.0) < 1e-5);
    REQUIRE(nr[(size_t)i] == 0.0f && fr[(size_t)i] == raylen);
  }
  const int64_t chunk = 37, rows = 64;
  for (int64_t a = 0; a < texels; a += chunk) {
    const int64_t k = texels - a < chunk ? texels - a : chunk;
    std::vector<float> co((size_t)rows * 3), cd((size_t)rows * 3), cn((size_t)rows), cf((size_t)rows);
    REQUIRE(hc_texel_rays(atlas, vertices.data(), normals.data(), faces.data(), V, &raylen, a, k, rows, co.data(), cd.data(),
                          cn.data(), cf.data()) == 0);
    REQUIRE(std::memcmp(co.data(), o.data() + 3 * a, sizeof(float) * 3 * (size_t)k) == 0);
    REQUIRE(std::memcmp(cd.data(), d.data() + 3 * a, sizeof(float) * 3 * (size_t)k) == 0);
    for (int64_t r = k; r < rows; ++r) {
      REQUIRE(std::memcmp(co.data() + 3 * r, co.data() + 3 * (k - 1), sizeof(float) * 3) == 0);
      REQUIRE(std::memcmp(cd.data() + 3 * r, cd.data() + 3 * (k - 1), sizeof(float) * 3) == 0);
    }
  }
  REQUIRE(hc_texel_rays(atlas, vertices.data(), normals.data(), faces.data(), V, &raylen, texels - 1, 2, 2, o.data(), d.data(),
                        nr.data(), fr.data()) == NSAMD_ERR_INVALID_ARG);  // past the atlas

  // the image: rows 1 .. texels - 2 of an exactly-sized atlas, so that the destination starts at an odd byte
  std::vector<uint8_t> image((size_t)texels * 3, 7);
  std::vector<float> rgb((size_t)texels * 3);
  for (size_t i = 0; i < rgb.size(); ++i) rgb[i] = (float)((int)(i % 300) - 20) / 255.0f;
  if (texels > 2) {
    REQUIRE(hc_texture_store(rgb.data(), texels - 2, 1, image.data()) == 0);
    for (int c = 0; c < 3; ++c) REQUIRE(image[(size_t)c] == 7 && image[(size_t)(3 * (texels - 1) + c)] == 7);
    for (int64_t j = 0; j < 3 * (texels - 2); ++j) {
      const int v = (int)(j % 300) - 20;
      REQUIRE(image[(size_t)(3 + j)] == (v < 0 ? 0 : (v > 255 ? 255 : v)));
    }
  }
  std::printf("texels %lld raylen %.9g\n", (long long)texels, (double)raylen);
  return 0;
}
