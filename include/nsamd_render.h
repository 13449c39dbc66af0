/*
 * nsamd_render.h — the part of libnsamd.so's C ABI that serves the full-image eval render of the packed (instant-ngp) path,
 * apart from the training and rendering core of nsamd.h. Conventions as there: device pointers, fp32, dense row-major
 * tensors, packed_info [num_rays,2] int64 (start, count), a hipStream_t; 0 (NSAMD_OK) or a negative nsamd_status, nothing
 * launched on error, no allocation, no synchronisation. Paths are relative to the reference's nerfstudio/ package.
 */
#ifndef NSAMD_RENDER_H
#define NSAMD_RENDER_H

#include "nsamd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------
 * The per-ray tail of the eval render in ONE pass: nsamd_packed_weights_fwd followed by nsamd_packed_composite_fwd (rgb,
 * accumulation, expected depth; models/instant_ngp.py:191-214, renderers.py:93-119, 310-317, 365-380), BIT FOR BIT — the
 * same fp32 / double operations in the same order, one wavefront per ray over chunks of 64 samples — without the weights
 * going to memory: 24 B read per sample. sigmas [n], rgb [n,3], t_starts / t_ends [n]; background_mode 0 (none) or 1 (the
 * three host floats of background_rgb_host); eval_mode: nan_to_num on the samples' colours and a clamp of the result to
 * [0, 1]. No early exit on an underflowed transmittance (without eval_mode 0 * NaN stays NaN, as in the two launches).
 * out_rgb [num_rays,3], out_accumulation, out_depth [num_rays] are required. out_mid_lo / out_mid_hi [num_rays] (both or
 * neither): the minimum / maximum over the ray's samples of (t_start + t_end) / 2 — what the depth clip of
 * renderers.py:381-383 reduces over —, +inf / -inf for a ray without samples. num_rays == 0 is a no-op.
 * ------------------------------------------------------------------------------------------------------------ */
int nsamd_packed_render_fwd(const float* t_starts, const float* t_ends, const float* sigmas, const float* rgb,
                            const int64_t* packed_info, int64_t num_rays, int background_mode,
                            const float* background_rgb_host, int eval_mode, float* out_rgb, float* out_accumulation,
                            float* out_depth, float* out_mid_lo, float* out_mid_hi, nsamd_stream_t stream);

/* Per packed sample s of ray r = ray_indices[s]: positions [n,3] = o[r] + d[r] (t_start + t_end) / 2 — the expression and
 * the bits of nsamd_packed_positions — and sample_directions [n,3] = d[r], the row the field takes per sample (one launch
 * for nsamd_packed_positions and a gather of the directions). num_samples == 0 is a no-op. */
int nsamd_packed_ray_points(const float* origins, const float* directions, const int64_t* ray_indices,
                            const float* t_starts, const float* t_ends, int64_t num_samples, float* positions,
                            float* sample_directions, nsamd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NSAMD_RENDER_H */
