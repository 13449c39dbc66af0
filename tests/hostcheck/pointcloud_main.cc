// Stand-alone program over tests/hostcheck/pointcloud_helpers.cc, built by tests/test_pointcloud_cpu.py with
// -fsanitize=address,undefined and run once per cloud: memory and arithmetic of the host build of csrc/pointcloud.h under the
// sanitizers, with exactly-sized heap buffers so that a row or slot past an end is caught.
//   pointcloud_main <points.f32> <n> <k> <std_ratio>
// reads n * 3 raw little-endian floats, runs the neighbour search through the rings and through the brute-force phase over
// three grids (a default-like one, one cell, a fine one whose box leaves the far points out), requires the same bits from all of
// them, applies the outlier rule, pushes the points through the selection as rays (appends, then an overflow), and prints
// "kept <m> of <n>". Exit status 0 when everything agreed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/nsamd_pointcloud.h"

extern "C" {
int hc_points_select(const float*, const float*, const float*, const float*, const float*, const float*, int64_t, nsamd_crop_box,
                     float*, float*, float*, float*, int64_t, int64_t*, int64_t*);
int hc_select_below(const double*, int64_t, const double*, int64_t*, int64_t*, int64_t*);
int hc_point_cell_keys(const float*, int64_t, nsamd_point_grid, int64_t*);
int hc_knn_mean_distance(const float*, int64_t, const int32_t*, const int32_t*, nsamd_point_grid, int32_t, int32_t, double*,
                         int32_t*);
}

#define REQUIRE(cond)                                              \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                    \
    }                                                              \
  } while (0)

static int knn(const std::vector<float>& pts, int64_t n, nsamd_point_grid grid, int k, int max_rings, std::vector<double>& avg,
               int32_t* brute) {
  const int64_t cells = (int64_t)grid.dims[0] * grid.dims[1] * grid.dims[2];
  std::vector<int64_t> keys((size_t)n);
  REQUIRE(hc_point_cell_keys(pts.data(), n, grid, keys.data()) == 0);
  std::vector<int32_t> order((size_t)n), cell_start((size_t)cells + 1, 0), unfinished((size_t)n + 1);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return keys[a] < keys[b]; });
  for (int64_t i = 0; i < n; ++i) ++cell_start[(size_t)keys[i] + 1];
  for (int64_t c = 0; c < cells; ++c) cell_start[c + 1] += cell_start[c];
  avg.assign((size_t)n, -1.0);
  REQUIRE(hc_knn_mean_distance(pts.data(), n, order.data(), cell_start.data(), grid, k, max_rings, avg.data(),
                               unfinished.data()) == 0);
  *brute = unfinished[0];
  return 0;
}

int main(int argc, char** argv) {
  REQUIRE(argc == 5);
  const int64_t n = std::atoll(argv[2]);
  const int k = std::atoi(argv[3]);
  const double std_ratio = std::atof(argv[4]);
  REQUIRE(n > 0);
  std::vector<float> pts((size_t)n * 3);
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f != nullptr);
  REQUIRE(std::fread(pts.data(), sizeof(float), pts.size(), f) == pts.size());
  std::fclose(f);

  const nsamd_point_grid grids[3] = {{{-0.6f, -0.6f, -0.6f}, 0.1f, {12, 12, 12}},
                                     {{-0.6f, -0.6f, -0.6f}, 1.2f, {1, 1, 1}},
                                     {{-0.55f, -0.5f, -0.45f}, 0.02f, {55, 50, 45}}};
  std::vector<double> first, avg;
  for (int g = 0; g < 3; ++g)
    for (int max_rings : {0, 1, 3, 100}) {
      int32_t brute = 0;
      if (knn(pts, n, grids[g], k, max_rings, avg, &brute) != 0) return 1;
      REQUIRE(max_rings != 0 || brute == n);
      REQUIRE(max_rings != 100 || brute == 0);
      if (first.empty()) first = avg;
      REQUIRE(std::memcmp(first.data(), avg.data(), sizeof(double) * (size_t)n) == 0);
    }

  double sum = 0.0, dev2 = 0.0;
  int64_t valid = 0;
  for (double a : avg)
    if (a > 0.0) sum += a, ++valid;
  const double mean = sum / (double)valid;
  for (double a : avg)
    if (a > 0.0) dev2 += (a - mean) * (a - mean);
  const double threshold = mean + std_ratio * std::sqrt(dev2 / (double)(valid - 1));
  const int64_t words = NSAMD_SELECT_SCRATCH_WORDS(n);
  std::vector<int64_t> kept((size_t)n), scratch((size_t)words);
  int64_t count = -1;
  REQUIRE(hc_select_below(avg.data(), n, &threshold, kept.data(), &count, scratch.data()) == 0);
  REQUIRE(count >= 0 && count <= n);
  for (int64_t i = 1; i < count; ++i) REQUIRE(kept[i - 1] < kept[i]);

  // the points as rays from the origin along themselves at depth 1, cropped to the unit box: two appends, then an overflow
  std::vector<float> origins((size_t)n * 3, 0.0f), depth((size_t)n, 1.0f), alpha((size_t)n);
  for (int64_t i = 0; i < n; ++i) alpha[i] = (i % 3 == 0) ? 0.25f : 0.75f;
  nsamd_crop_box box = {1, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {1.0f, 1.0f, 1.0f}};
  int64_t expected = 0;
  for (int64_t i = 0; i < n; ++i)
    expected += alpha[i] > 0.5f && std::fabs(pts[3 * i]) < 1 && std::fabs(pts[3 * i + 1]) < 1 && std::fabs(pts[3 * i + 2]) < 1;
  const int64_t cap = 2 * expected;
  std::vector<float> out_p((size_t)cap * 3), out_c((size_t)cap * 3), out_v((size_t)cap * 3), out_n((size_t)cap * 3);
  int64_t cursor[2] = {0, 0};
  for (int pass = 0; pass < 3; ++pass) {
    REQUIRE(hc_points_select(origins.data(), pts.data(), depth.data(), pts.data(), alpha.data(), pts.data(), n, box, out_p.data(),
                             out_c.data(), out_v.data(), out_n.data(), cap, cursor, scratch.data()) == 0);
    REQUIRE(cursor[0] == (pass == 0 ? expected : 2 * expected));
    REQUIRE(cursor[1] == (pass == 2 && expected > 0 ? 1 : 0));
  }
  REQUIRE(std::memcmp(out_p.data(), out_p.data() + 3 * expected, sizeof(float) * 3 * (size_t)expected) == 0);
  std::printf("kept %lld of %lld\n", (long long)count, (long long)n);
  return 0;
}
