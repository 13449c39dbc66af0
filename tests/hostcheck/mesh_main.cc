// Stand-alone program over tests/hostcheck/mesh_helpers.cc, built by tests/test_mesh_cpu.py with -fsanitize=address,undefined
// and run once per volume: memory and arithmetic of the host build of csrc/mesh.h under the sanitizers, with exactly-sized heap
// buffers so that a row, a word or a scratch byte past an end is caught.
//   mesh_main <values.f32> <X> <Y> <Z>
// reads X * Y * Z raw little-endian floats, counts, emits into buffers of exactly the counted sizes, requires every face index
// to name a vertex, every vertex to lie on its volume, a second run to give the same bytes, a wrong V to write nothing, and
// prints "vertices <V> triangles <T>". Exit status 0 when everything agreed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/nsamd_mesh.h"

extern "C" {
int hc_mesh_count(nsamd_mesh_volume, const float*, void*, int64_t*);
int hc_mesh_emit(nsamd_mesh_volume, const float*, const float*, const void*, int64_t, int64_t, float*, float*, float*, int32_t*);
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
  const nsamd_mesh_volume vol = {{-0.5f, 0.25f, 1.0f}, {0.1f, 0.2f, 0.15f}, {std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])}};
  const int64_t n = (int64_t)vol.dims[0] * vol.dims[1] * vol.dims[2];
  REQUIRE(n > 0);
  std::vector<float> values((size_t)n), colors((size_t)n * 3);
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f != nullptr);
  REQUIRE(std::fread(values.data(), sizeof(float), values.size(), f) == values.size());
  std::fclose(f);
  for (int64_t i = 0; i < 3 * n; ++i) colors[(size_t)i] = (float)(i % 251) / 250.0f;

  std::vector<int64_t> scratch((size_t)(NSAMD_MESH_SCRATCH_BYTES(n) + 7) / 8);  // 8-byte aligned, no slack beyond the rounding
  int64_t totals[2] = {-1, -1};
  REQUIRE(hc_mesh_count(vol, values.data(), scratch.data(), totals) == 0);
  const int64_t V = totals[0], T = totals[1];
  REQUIRE(V >= 0 && T >= 0);
  std::vector<float> vertices((size_t)V * 3, -7.0f), normals((size_t)V * 3, -7.0f), vcolors((size_t)V * 3, -7.0f);
  std::vector<int32_t> faces((size_t)T * 3, -7);
  if (V > 0) {  // a wrong pair of totals writes nothing
    REQUIRE(hc_mesh_emit(vol, values.data(), colors.data(), scratch.data(), V - 1, T, vertices.data(), normals.data(), vcolors.data(),
                         faces.data()) == 0);
    for (float x : vertices) REQUIRE(x == -7.0f);
    for (int32_t i : faces) REQUIRE(i == -7);
  }
  REQUIRE(hc_mesh_emit(vol, values.data(), colors.data(), scratch.data(), V, T, vertices.data(), normals.data(), vcolors.data(),
                       faces.data()) == 0);
  for (int32_t i : faces) REQUIRE(i >= 0 && i < V);
  for (int64_t i = 0; i < V; ++i)
    for (int a = 0; a < 3; ++a) {
      const float lo = vol.origin[a], hi = vol.origin[a] + (float)(vol.dims[a] - 1) * vol.voxel_size[a];
      REQUIRE(vertices[(size_t)(3 * i + a)] >= lo - 1e-5f && vertices[(size_t)(3 * i + a)] <= hi + 1e-5f);
      REQUIRE(vcolors[(size_t)(3 * i + a)] >= 0.0f && vcolors[(size_t)(3 * i + a)] <= 1.0f);
      REQUIRE(normals[(size_t)(3 * i + a)] >= -1.0f - 1e-6f && normals[(size_t)(3 * i + a)] <= 1.0f + 1e-6f);
    }
  std::vector<float> again((size_t)V * 3, 9.0f), again_n((size_t)V * 3), again_c((size_t)V * 3);
  std::vector<int32_t> again_f((size_t)T * 3, 9);
  std::vector<int64_t> scratch2(scratch.size());
  int64_t totals2[2] = {0, 0};
  REQUIRE(hc_mesh_count(vol, values.data(), scratch2.data(), totals2) == 0 && totals2[0] == V && totals2[1] == T);
  REQUIRE(hc_mesh_emit(vol, values.data(), colors.data(), scratch2.data(), V, T, again.data(), again_n.data(), again_c.data(),
                       again_f.data()) == 0);
  REQUIRE(V == 0 || std::memcmp(again.data(), vertices.data(), sizeof(float) * 3 * (size_t)V) == 0);
  REQUIRE(T == 0 || std::memcmp(again_f.data(), faces.data(), sizeof(int32_t) * 3 * (size_t)T) == 0);
  std::printf("vertices %lld triangles %lld\n", (long long)V, (long long)T);
  return 0;
}
