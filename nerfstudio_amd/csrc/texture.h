// Per-texel arithmetic of the texture export (gfx950; the host compiler sees it only through tests/hostcheck): the closed form
// of the reference's per-UV-triangle unwrap (exporter/texture_utils.py:77-208), the texel's ray, an edge's length for the ray
// length and the 8-bit level of a colour, as include/nsamd_texture.h defines them. The fp32 operation order is stated HERE,
// once, for the kernels and the host build of the tests; the library is built with -ffp-contract=off.
#pragma once

#include "common.h"
#include "../../include/nsamd_texture.h"

namespace nsamd {

constexpr int64_t kTextureMaxSide = 0x7fffffffLL;

// ---- argument limits, shared by the entry points and the host build of the tests (no HIP runtime call) --------------------------
// *width, *height: the atlas in texels
NSAMD_HD int texel_atlas_check(const nsamd_texel_atlas& a, int64_t* width, int64_t* height) {
  if (a.faces < 1 || a.px < 2 || a.squares_w < 1 || a.squares_h < 1) return NSAMD_ERR_INVALID_ARG;
  if (2 * (int64_t)a.squares_w * a.squares_h < a.faces) return NSAMD_ERR_INVALID_ARG;
  *width = (int64_t)a.squares_w * ((int64_t)a.px + 3);
  *height = (int64_t)a.squares_h * a.px;
  return (*width > kTextureMaxSide || *height > kTextureMaxSide) ? NSAMD_ERR_UNSUPPORTED : NSAMD_OK;
}

NSAMD_HD int texel_range_check(int64_t texels, int64_t first, int64_t count, int64_t rows) {
  if (count == 0 && rows == 0) return NSAMD_OK;
  if (first < 0 || count < 1 || rows < count || count > texels || first > texels - count) return NSAMD_ERR_INVALID_ARG;
  return rows > 0x7fffffffLL ? NSAMD_ERR_UNSUPPORTED : NSAMD_OK;
}

NSAMD_HD int raylen_check(int64_t V, int64_t T) {
  return (V < 1 || T < 1 || T > 0x7fffffffLL) ? NSAMD_ERR_INVALID_ARG : NSAMD_OK;
}

NSAMD_HD int64_t raylen_blocks(int64_t T) {
  const int64_t b = (T + NSAMD_TEXTURE_BLOCK - 1) / NSAMD_TEXTURE_BLOCK;
  return b < NSAMD_RAYLEN_MAX_BLOCKS ? b : NSAMD_RAYLEN_MAX_BLOCKS;
}

// a face's vertex index as the gathers use it: clamped into [0, V), V >= 1
NSAMD_HD int64_t texel_vertex(int32_t i, int64_t V) { return i < 0 ? 0 : (i >= V ? V - 1 : (int64_t)i); }

// ---- the layout -----------------------------------------------------------------------------------------------------------------
// Texel (x, y) of the atlas (width = sw (P + 3)): its triangle and the three weights, each ONE integer numerator over P - 1.
NSAMD_HD int64_t texel_site(const nsamd_texel_atlas& a, int64_t x, int64_t y, float* w) {
  const int64_t sqw = (int64_t)a.px + 3, P = a.px;
  const int64_t su = point_ray(x, sqw), sv = point_ray(y, P);
  const int64_t uo = x - su * sqw, vo = y - sv * P;
  const int64_t lower = (uo + vo >= P + 1) ? 1 : 0;
  int64_t t = 2 * (sv * a.squares_w + su) + lower;
  t = t < a.faces - 1 ? t : (int64_t)a.faces - 1;
  // the triangle's own square: another one than (su, sv) for the texels past the last face
  const int64_t q = t >> 1, osv = point_ray(q, a.squares_w), osu = q - osv * a.squares_w;
  const int64_t du = x - osu * sqw, dv = y - osv * P;
  const int64_t n1 = (t & 1) ? P + 2 - du : du, n2 = (t & 1) ? P - 1 - dv : dv;
  const float den = (float)(P - 1);
  w[0] = (float)(P - 1 - n1 - n2) / den;
  w[1] = (float)n1 / den;
  w[2] = (float)n2 / den;
  return t;
}

// ---- a ray ----------------------------------------------------------------------------------------------------------------------
// origin o[3] and direction d[3] of linear texel `texel`: texture_utils.py:195-206 and :386, left to right, separately rounded
NSAMD_HD void texel_ray(const nsamd_texel_atlas& a, int64_t width, const float* vertices, const float* normals,
                        const int32_t* faces, int64_t V, float raylen, int64_t texel, float* o, float* d) {
  const int64_t y = point_ray(texel, width), x = texel - y * width;
  float w[3];
  const int64_t t = texel_site(a, x, y, w);
  const int64_t i0 = texel_vertex(faces[3 * t], V), i1 = texel_vertex(faces[3 * t + 1], V), i2 = texel_vertex(faces[3 * t + 2], V);
  float b[3];
  for (int c = 0; c < 3; ++c) {
    o[c] = (vertices[3 * i0 + c] * w[0] + vertices[3 * i1 + c] * w[1]) + vertices[3 * i2 + c] * w[2];
    b[c] = -((normals[3 * i0 + c] * w[0] + normals[3 * i1 + c] * w[1]) + normals[3 * i2 + c] * w[2]);
  }
  const float len = sqrtf((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
  const float div = fmaxf(len, 1e-12f);  // F.normalize's eps
  const float half = 0.5f * raylen;
  for (int c = 0; c < 3; ++c) {
    d[c] = b[c] / div;
    o[c] = o[c] - half * d[c];
  }
}

// ---- the ray length -------------------------------------------------------------------------------------------------------------
// |v[f1] - v[f0]| of face t in fp64: the differences of two fp32 values are exact there
NSAMD_HD double raylen_edge(const float* vertices, int64_t V, const int32_t* faces, int64_t t) {
  const int64_t i0 = texel_vertex(faces[3 * t], V), i1 = texel_vertex(faces[3 * t + 1], V);
  const double dx = (double)vertices[3 * i1] - (double)vertices[3 * i0];
  const double dy = (double)vertices[3 * i1 + 1] - (double)vertices[3 * i0 + 1];
  const double dz = (double)vertices[3 * i1 + 2] - (double)vertices[3 * i0 + 2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

NSAMD_HD float raylen_finish(double sum, int64_t T) { return (float)(2.0 * sum / (double)T); }  // the one rounding to fp32

// ---- the image ------------------------------------------------------------------------------------------------------------------
// floor(clamp(v, 0, 1) * 255 + 0.5): fmaxf / fminf return the other operand for a NaN, so NaN -> 0
NSAMD_HD uint32_t texture_level(float v) {
  const float c = fminf(fmaxf(v, 0.0f), 1.0f);
  return (uint32_t)(c * 255.0f + 0.5f);  // in [0.5, 255.5]: the conversion truncates = floor
}

}  // namespace nsamd
