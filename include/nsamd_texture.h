/*
 * nsamd_texture.h — the part of libnsamd.so's C ABI that textures an exported mesh (ns-export tsdf / poisson with
 * texture_method="nerf"): what exporter/texture_utils.py:export_textured_mesh does around the render of one ray per texel —
 * the per-UV-triangle unwrap (unwrap_mesh_per_uv_triangle, :77-208), the ray length (:374-380) and the 8-bit image.
 * Conventions as in nsamd.h: device pointers, dense row-major tensors, a small POD struct passed by value, a hipStream_t;
 * 0 (NSAMD_OK) or a negative nsamd_status, nothing launched on error, no allocation, no synchronisation — every launch can be
 * captured in a graph. Paths are relative to the reference's nerfstudio/ package.
 *
 * THE ATLAS. F faces, P = px_per_uv_triangle >= 2 (at P = 1 the reference divides by a zero area). Two faces share a square
 * of (P + 3) x P texels; sw x sh squares, sw = ceil(sqrt(ceil(F / 2))), sh = ceil(ceil(F / 2) / sw): W = sw (P + 3) texels
 * wide, H = sh P high, texel (x, y) = linear index y W + x. For texel (x, y):
 *   its square (su, sv) = (x div (P + 3), y div P), its offsets (uo, vo) inside it, lower = (uo + vo >= P + 1),
 *   its triangle t = min(2 (sv sw + su) + lower, F - 1).
 * The corners of triangle t lie on texel centres of ITS OWN square ((t div 2) mod sw, (t div 2) div sw) — for the texels past
 * the last face, clamped to F - 1, that is another square than the texel's, and they extrapolate from it as the reference's
 * do — at the offsets (0,0), (P-1,0), (0,P-1) for an even t (the upper triangle) and (P+2,P-1), (3,P-1), (P+2,0) for an odd
 * one. With (du, dv) the texel's offset from that square's corner the barycentric weights are RATIOS OF SMALL INTEGERS,
 *   upper: w1 = du / (P-1), w2 = dv / (P-1);   lower: w1 = (P+2-du) / (P-1), w2 = (P-1-dv) / (P-1);   w0 = 1 - w1 - w2,
 * each formed here as one integer numerator divided by (P-1) in fp32: one rounding per weight, whatever the atlas size. (The
 * reference forms them in fp32 from differences of texture coordinates 1 / W apart: 1e-3 of error at 50 000 faces.)
 * The texture coordinate of a corner at offset (a, b) of square (su, sv) is ((su (P+3) + a + 0.5) / W, (sv P + b + 0.5) / H).
 *
 * THE RAY of a texel, in fp32, separately rounded, left to right as the reference writes it:
 *   origin    = v0 w0 + v1 w1 + v2 w2                          (v_i, n_i: the vertices and normals of the triangle's corners)
 *   direction = -(n0 w0 + n1 w1 + n2 w2) / max(|.|, 1e-12)      (F.normalize; a zero blend gives a zero direction)
 *   origin   -= (0.5 raylen) direction,   near = 0,   far = raylen.
 *
 * THE IMAGE. The reference writes the PNG with mediapy, which was not available to compare against; this is the project's
 * definition of the 8-bit level of a colour channel v, in fp32: floor(clamp(v, 0, 1) * 255 + 0.5) — a product, then a sum —
 * with clamp = fmin(fmax(v, 0), 1), so that NaN writes 0, -Inf 0 and +Inf 255.
 */
#ifndef NSAMD_TEXTURE_H
#define NSAMD_TEXTURE_H

#include "nsamd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NSAMD_TEXTURE_BLOCK 256       /* lanes per workgroup of every kernel here */
#define NSAMD_RAYLEN_MAX_BLOCKS 1024  /* workgroups of the edge-length sum at most */
/* bytes of `scratch` of nsamd_mesh_raylen: one fp64 partial sum per workgroup (8-byte aligned) */
#define NSAMD_RAYLEN_SCRATCH_BYTES (8 * NSAMD_RAYLEN_MAX_BLOCKS)

typedef struct nsamd_texel_atlas {
  int32_t faces;      /* F >= 1                                   */
  int32_t px;         /* P >= 2                                   */
  int32_t squares_w;  /* sw >= 1                                  */
  int32_t squares_h;  /* sh >= 1, 2 sw sh >= F; W, H <= 2^31 - 1  */
} nsamd_texel_atlas;

/* ------------------------------------------------------------------------------------------------------------
 * The rays of texels first .. first + count - 1 of the atlas' row-major W x H grid, one lane per texel, into the first
 * `rows` >= count rows of origins, directions [rows,3] and nears, fars [rows] fp32; rows count .. rows - 1 are copies of row
 * count - 1 (the padding rule of the eval loop's last chunk: its depth clip range is unchanged). vertices, normals [V,3] fp32,
 * faces [F,3] int32; a face index outside [0, V) is CLAMPED into it before the gather: whatever the mesh holds, nothing is
 * read out of bounds. raylen_dev: one fp32 on the device (nsamd_mesh_raylen's output, or 0 for raylen_method="none").
 * A workgroup's rows go through LDS so that every store instruction of a wavefront writes 256 contiguous bytes.
 * count == 0 and rows == 0 is a no-op; else 1 <= count <= rows, first >= 0, first + count <= W H (NSAMD_ERR_INVALID_ARG).
 * ------------------------------------------------------------------------------------------------------------ */
int nsamd_texel_rays(nsamd_texel_atlas atlas, const float* vertices, const float* normals, const int32_t* faces, int64_t V,
                     const float* raylen_dev, int64_t first, int64_t count, int64_t rows, float* origins, float* directions,
                     float* nears, float* fars, nsamd_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * raylen_dev[0] = 2 mean_f |v[f1] - v[f0]| over the T faces (texture_utils.py:374-380). The differences, the lengths and the
 * sum are formed in fp64 from the fp32 vertices — per lane over a fixed stride, a fixed butterfly per wavefront, the
 * wavefronts and then the workgroups' partial sums (scratch) in index order by one finishing workgroup — and rounded ONCE to
 * fp32: no atomics, the same bits run to run. Face indices are clamped as above. T == 0 is NSAMD_ERR_INVALID_ARG (the
 * reference's mean of nothing is NaN), as are V <= 0 and T > 2^31 - 1.
 * ------------------------------------------------------------------------------------------------------------ */
int nsamd_mesh_raylen(const float* vertices, int64_t V, const int32_t* faces, int64_t T, void* scratch, float* raylen_dev,
                      nsamd_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * rgb [count,3] fp32 as 8-bit levels (the rule above) into rows first .. first + count - 1 of the [H W, 3] uint8 atlas. A
 * lane owns one aligned 32-bit word of the destination and stores it whole; the at most two partial words at the ends are
 * stored byte by byte. first >= 0, 0 <= count <= 2^31 - 1; count == 0 is a no-op. The caller owns the bound first + count <= H W.
 * ------------------------------------------------------------------------------------------------------------ */
int nsamd_texture_store(const float* rgb, int64_t count, int64_t first, uint8_t* atlas_u8, nsamd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NSAMD_TEXTURE_H */
