// Per-ray arithmetic of a training batch sampled on the device (gfx950; the host compiler sees it only through
// tests/hostcheck): the counter-based generator the step prologue and the batch sampler share, the uniform -> pixel index
// recipe of the reference's PixelSampler.sample_method (nerfstudio/data/pixel_samplers.py:137-174:
// `floor(torch.rand(n, 3) * tensor([N, H, W])).long()`) and the uint8 -> float colour of InputDataset.get_image_float32
// (data/datasets/base_dataset.py:107: `image / np.float32(255)`). fp32 with the reference's operations in the reference's
// order; the library is built with -ffp-contract=off.
#pragma once

#include "common.h"

namespace nsamd {

// XORed into the trainer's seed for the pixel stream: the batch sampler and the step prologue (jitter, random background)
// share (seed, draw counter), and a different key makes the two streams of one step independent.
constexpr uint64_t kBatchSeedXor = 0xA0761D6478BD642FULL;

NSAMD_HD void philox_round(uint32_t (&c)[4], uint32_t (&k)[2]) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k[0], n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k[1], n3 = (uint32_t)p0;
  c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3;
  k[0] += 0x9E3779B9u, k[1] += 0xBB67AE85u;
}

// Philox-4x32-10 (Salmon et al., SC'11): counter -> four random words, in place; the key is consumed.
NSAMD_HD void philox4x32_10(uint32_t (&counter)[4], uint32_t (&key)[2]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) philox_round(counter, key);
}

// 24 random bits: uniform on [0, 1), every value exactly representable
NSAMD_HD float batch_uniform(uint32_t word) { return (float)(word >> 8) * 5.9604644775390625e-8f; }

// (u * dim) as an fp32 product, truncated: pixel_samplers.py:169-172. A 24-bit uniform is at most 1 - 2^-24, so the exact
// product lies dim * 2^-24 below dim — more than half an ulp of the floats just below dim (exactly one ulp when dim is a power
// of two) — and never rounds up to dim: the clamp never fires (tests/test_device_batches_cpu.py checks the top of the range).
// It only guarantees that no read leaves the store.
NSAMD_HD int32_t batch_pixel_index(float u, int32_t dim) {
  const int32_t v = (int32_t)(u * (float)dim);
  return v > dim - 1 ? dim - 1 : v;
}

// IEEE division (hipcc's default for `/`, no reciprocal): the bits of numpy's uint8 / np.float32(255)
NSAMD_HD float batch_pixel_float(uint8_t b) { return (float)b / 255.0f; }

// One draw of ray `ray`: (image, row, col) from the first three words of Philox(counter = (ray, attempt, draw), key).
NSAMD_HD void batch_draw_pixel(uint32_t ray, uint32_t attempt, int64_t draw, uint64_t key, int32_t num_images, int32_t height,
                               int32_t width, int32_t* c, int32_t* y, int32_t* x) {
  uint32_t ctr[4] = {ray, attempt, (uint32_t)draw, (uint32_t)((uint64_t)draw >> 32)};
  uint32_t k[2] = {(uint32_t)key, (uint32_t)(key >> 32)};
  philox4x32_10(ctr, k);
  *c = batch_pixel_index(batch_uniform(ctr[0]), num_images);
  *y = batch_pixel_index(batch_uniform(ctr[1]), height);
  *x = batch_pixel_index(batch_uniform(ctr[2]), width);
}

}  // namespace nsamd
