// TEST INFRASTRUCTURE (tests/test_device_batches_cpu.py): compiles the per-ray arithmetic of the device-side batch sampler
// (nerfstudio_amd/csrc/batch_sample.h: Philox-4x32-10, the uniform -> pixel index recipe, the uint8 -> float colour) with the HOST
// compiler, so that `pytest -m "not gpu"` can pin it to the reference's fixture without a GPU. Nothing in the product loads this
// library; the kernels run these functions on the device.
#include <math.h>
#include <stdint.h>

#include "../../nerfstudio_amd/csrc/batch_sample.h"

using namespace nsamd;

extern "C" {

// counters [n,4], keys [n,2] -> words [n,4]
void hc_philox4x32_10(const uint32_t* counters, const uint32_t* keys, int64_t n, uint32_t* out) {
  for (int64_t i = 0; i < n; ++i) {
    uint32_t c[4] = {counters[4 * i], counters[4 * i + 1], counters[4 * i + 2], counters[4 * i + 3]};
    uint32_t k[2] = {keys[2 * i], keys[2 * i + 1]};
    philox4x32_10(c, k);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = c[j];
  }
}

void hc_batch_uniform(const uint32_t* words, int64_t n, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = batch_uniform(words[i]);
}

void hc_batch_pixel_index(const float* u, int64_t n, int32_t dim, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = batch_pixel_index(u[i], dim);
}

// the unclamped recipe next to it: how often the clamp of batch_pixel_index changes a result
int64_t hc_batch_pixel_index_clamped(const float* u, int64_t n, int32_t dim) {
  int64_t fired = 0;
  for (int64_t i = 0; i < n; ++i) fired += ((int32_t)(u[i] * (float)dim) != batch_pixel_index(u[i], dim)) ? 1 : 0;
  return fired;
}

void hc_batch_pixel_float(const uint8_t* b, int64_t n, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = batch_pixel_float(b[i]);
}

// the draw of one lane of the kernel: ray, attempt, draw counter, key (the seed already XORed) -> (image, row, col)
void hc_batch_draw_pixel(const uint32_t* rays, const uint32_t* attempts, int64_t n, int64_t draw, uint64_t key, int32_t num_images,
                         int32_t height, int32_t width, int32_t* out /* [n,3] */) {
  for (int64_t i = 0; i < n; ++i)
    batch_draw_pixel(rays[i], attempts[i], draw, key, num_images, height, width, out + 3 * i, out + 3 * i + 1, out + 3 * i + 2);
}

uint64_t hc_batch_seed_xor(void) { return kBatchSeedXor; }

}  // extern "C"
