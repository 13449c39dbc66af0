/*
 * nsamd_image.h — the part of libnsamd.so's C ABI that measures and colours an evaluation frame: what a model's
 * get_image_metrics_and_images does after the render — PSNR and SSIM of the frame against its ground truth, the minimum and
 * maximum of a depth map, and the colormaps of utils/colormaps.py:46-152 — without a host round trip.
 * Conventions as in nsamd_texture.h: device pointers, dense row-major tensors, a small POD struct passed by value, a
 * nsamd_stream_t; 0 (NSAMD_OK) or a negative nsamd_status, nothing launched on error, no allocation, no synchronisation — every
 * launch can be captured in a graph; scratch is the caller's, sized by a constant or a host-only query. Images are [H, W, C]
 * fp32, channel-last, as the eval runners return them. Paths are relative to the reference's nerfstudio/ package.
 *
 * THE METRICS: the project's restatement of torchmetrics' structural_similarity_index_measure with the defaults nerfstudio
 * uses, and of its PeakSignalNoiseRatio. The definition is what is written here, not the library's code.
 *   window    Gaussian, sigma = 1.5, size 2 int(3.5 sigma + 0.5) + 1 = 11: g(d) = exp(-(d / sigma)^2 / 2), d = -5 .. 5, normalised
 *             to sum 1 (formed in fp64, rounded once to the fp32 constants the kernel uses); the 2-D window is the outer product.
 *   constants k1 = 0.01, k2 = 0.03, c1 = (k1 R)^2, c2 = (k2 R)^2; R = data_range, or, when none is given, the larger of the two
 *             images' max - min.
 *   a window  per channel, with E[.] the window-weighted mean:  mu_x = E[x], mu_y = E[y],
 *             s_xx = max(E[x^2] - mu_x^2, 0), s_yy likewise, s_xy = E[xy] - mu_x mu_y,
 *             ssim = ((2 mu_x mu_y + c1) (2 s_xy + c2)) / ((mu_x^2 + mu_y^2 + c1) (s_xx + s_yy + c2)).
 *   the value the library reflect-pads by 5 and crops 5 from every side of the map: what remains depends on unpadded pixels only,
 *             so ssim is the mean over the (H - 10) x (W - 10) x C windows that lie inside the image.
 *   psnr      10 log10(R_psnr^2 / mse), mse the mean of (x - y)^2 over all H W C values.
 * The kernel forms a window's moments ABOUT A PIVOT p that is constant over a tile of NSAMD_SSIM_TILE^2 windows (one value per
 * image and channel: the pixel at the centre of the tile's pixels, 0 where that is not finite): mu = p + E[x - p],
 * s_xx = E[(x - p)^2] - E[x - p]^2, s_xy = E[(x - p_x)(y - p_y)] - E[x - p_x] E[y - p_y] — the same quantities, without the
 * cancellation of E[x^2] - E[x]^2 against c2 on flat regions that costs the fp32 composition its fourth decimal. The sums of the
 * window values and of the squared errors are fp64 in a fixed order — per lane over a fixed stride, a fixed butterfly per
 * wavefront, the wavefronts and then the workgroups' partial sums (scratch) in index order by one finishing workgroup — and each
 * result is rounded ONCE to fp32: no atomics, the same bits run to run.
 *
 * THE COLORMAP of a one-channel value v, in fp32, separately rounded, in the order the reference writes it; the definition is
 * pinned BIT FOR BIT to a fixture written by the reference's own functions on the CPU (tests/golden/colormaps.npz): if a pixel
 * disagrees, this definition is what gets corrected.
 *   depth mode  t = (v - (float)near) / w, w = (float)((double)far - (double)near + 1e-10), t = clip(t, 0, 1); near and far are
 *               the fixed ones of the parameters or the minimum and maximum at range2_dev (nsamd_image_range of the same map).
 *   normalize   t = (t - lo) / ((hi - lo) + 1e-9f), lo and hi the minimum and maximum of the values at this point: those at
 *               range2_dev, in depth mode taken through the two lines above (they are monotone, so these ARE the extremes).
 *   then        t = t (float)(colormap_max - colormap_min) + (float)colormap_min; t = clip(t, 0, 1); invert: t = 1 - t;
 *               a NaN survives all of these (torch.clip keeps it) and becomes 0 here (torch.nan_to_num).
 *   colour      row (int)(t 255) (truncation) of the [256, 3] table; without a table ("gray") the value t three times.
 *   depth mode with an accumulation a: colour a + (1 - a), per channel.
 *   8-bit       nsamd_texture.h's rule for a colour channel, by the same code.
 */
#ifndef NSAMD_IMAGE_H
#define NSAMD_IMAGE_H

#include "nsamd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NSAMD_IMAGE_BLOCK 256        /* lanes per workgroup of every kernel here */
#define NSAMD_SSIM_WINDOW 11         /* taps of the Gaussian window per axis */
#define NSAMD_SSIM_TILE 32           /* a workgroup of nsamd_image_metrics owns a tile of 32 x 32 windows */
#define NSAMD_RANGE_MAX_BLOCKS 1024  /* workgroups of nsamd_image_range at most */
/* bytes of `scratch` of nsamd_image_range: one {min, max} fp32 pair per workgroup (8-byte aligned) */
#define NSAMD_RANGE_SCRATCH_BYTES (8 * NSAMD_RANGE_MAX_BLOCKS)

#define NSAMD_COLORMAP_PLAIN 0 /* apply_colormap of a one-channel float image */
#define NSAMD_COLORMAP_DEPTH 1 /* apply_depth_colormap */
#define NSAMD_COLORMAP_FIXED_NEAR 1 /* bits of nsamd_colormap_params.fixed */
#define NSAMD_COLORMAP_FIXED_FAR 2

typedef struct nsamd_colormap_params {
  int32_t mode;         /* NSAMD_COLORMAP_PLAIN or NSAMD_COLORMAP_DEPTH                                */
  int32_t normalize;    /* ColormapOptions.normalize                                                    */
  int32_t invert;       /* ColormapOptions.invert                                                       */
  int32_t fixed;        /* depth mode: which of near_plane / far_plane are given (bits above)           */
  double colormap_min;  /* ColormapOptions.colormap_min, colormap_max: Python floats, rounded to fp32   */
  double colormap_max;  /*   where the reference's tensor arithmetic rounds them                        */
  double near_plane;    /* used where its bit of `fixed` is set                                         */
  double far_plane;
} nsamd_colormap_params;

/* ------------------------------------------------------------------------------------------------------------
 * range2_dev[0], [1] = the minimum and the maximum of the n fp32 values at x. A NaN anywhere makes both NaN, as torch.min and
 * torch.max do. Two levels: at most NSAMD_RANGE_MAX_BLOCKS workgroups leave a pair each in scratch (NSAMD_RANGE_SCRATCH_BYTES),
 * one finishing workgroup combines them. n <= 0 is NSAMD_ERR_INVALID_ARG (the reference's minimum of nothing raises).
 * ------------------------------------------------------------------------------------------------------------ */
int nsamd_image_range(const float* x, int64_t n, void* scratch, float* range2_dev, nsamd_stream_t stream);

/* bytes of `scratch` of nsamd_image_metrics for an H x W x C image: two fp64 partial sums per tile (8-byte aligned); host only,
 * no HIP call. 0 for sizes nsamd_image_metrics refuses. */
int64_t nsamd_image_metrics_scratch_bytes(int64_t H, int64_t W, int32_t C);

/* ------------------------------------------------------------------------------------------------------------
 * out4_dev = {mse, psnr, ssim, R used} of pred against target, both [H, W, C] fp32 (THE METRICS above). With both range
 * pointers NULL R = data_range, which must be > 0; otherwise both must be given, each the {min, max} pair nsamd_image_range
 * wrote for its image, R = max(max_p - min_p, max_t - min_t) is formed on the device and data_range is ignored. psnr_range > 0
 * is R_psnr. ssim_map, when not NULL, receives the [H - 10, W - 10, C] per-window values (the library's return_full_image,
 * cropped); the four results do not depend on whether it is given. 1 <= C <= 4, H, W >= 11, H W C <= 2^31 - 1
 * (NSAMD_ERR_INVALID_ARG). R == 0 (two constant images and no data_range) yields what the formula yields, NaN in ssim; a NaN
 * pixel makes mse, psnr and ssim NaN.
 * ------------------------------------------------------------------------------------------------------------ */
int nsamd_image_metrics(const float* pred, const float* target, int64_t H, int64_t W, int32_t C, const float* range_pred2_dev,
                        const float* range_target2_dev, float data_range, float psnr_range, void* scratch, float* out4_dev,
                        float* ssim_map, nsamd_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * THE COLORMAP of the n fp32 values at `values`, one lane per pixel, into out_rgb [n, 3] fp32 and / or out_u8 [n, 3] uint8 (at
 * least one of them). lut: [256, 3] fp32, NULL = "gray". range2_dev: the {min, max} of `values` on the device; needed with
 * normalize and in depth mode unless both planes are fixed, else it may be NULL. accumulation: [n] fp32 or NULL, depth mode
 * only. 1 <= n <= 2^31 - 1; a mode other than the two above, an accumulation in plain mode, a missing range and both outputs NULL
 * are NSAMD_ERR_INVALID_ARG.
 * ------------------------------------------------------------------------------------------------------------ */
int nsamd_colormap(const float* values, int64_t n, const float* lut, const float* range2_dev, const float* accumulation,
                   nsamd_colormap_params params, float* out_rgb, uint8_t* out_u8, nsamd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NSAMD_IMAGE_H */
