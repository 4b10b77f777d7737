/*
 * gsr_eval.h -- C ABI of the evaluation metrics (PSNR, SSIM, iMAE, iRMSE), whole-image and
 * per-region, fused on the device.  Exported by libgsr_hip.so.
 *
 * Replaces the per-frame metric loop of render_hierarchy_final.py:259-390: compute_metrics (:142-157:
 * psnr / ssim for the whole image, psnr_masked / ssim_masked per depth range and per segmentation
 * category), compute_depth_metrics (:159-173) and the pixel-weighted running sums (:287-385).  LPIPS,
 * the third image metric of compute_metrics, is gsr_lpips.h.
 *
 * A region is one bit of a uint16 plane: bit r of region_bits[p] says pixel p belongs to region r.
 * Regions may overlap.  gsr_eval_depth_range_bits and gsr_eval_color_bits build the reference's two
 * kinds of region (get_depth_range_mask :121-139, the category colour match :353-358).
 *
 * With a = alpha_mask (1 when NULL), x = clamp(image, 0, 1) a, y = clamp(gt, 0, 1) a, p = invdepth,
 * g = gt_invdepth, m the region's 0/1 mask and S(.) the sum over the H W pixels:
 *
 *   row 0 (whole image)
 *     psnr   = mean_c 20 log10(1 / sqrt(S((x_c - y_c)^2) / (H W)))          utils/image_utils.py:17-19
 *     ssim   = mean over channels and pixels of the zero-padded 11x11 map    utils/loss_utils.py:43-61
 *     imae   = S(|p - g| a) / S(a),  irmse = sqrt(S((p - g)^2 a) / S(a)),    both 0 when S(a) is 0
 *     weight = H W,  evaluated = 1,  mask pixels = valid windows = H W
 *   row 1 + r (region r)
 *     evaluated = S(m) > 0; every other column is 0 when it is not
 *     psnr   = mean_c 20 log10(1 / sqrt(S((x_c - y_c)^2 m) / S(m)))          utils/image_utils.py:21-36
 *     ssim   = ssim_masked (utils/loss_utils.py:85-153): windowed moments of x m and y m divided by
 *              the windowed mask weight w; a window is valid iff w > 1e-6; a map value is kept iff
 *              its denominator is > 1e-10; the map is multiplied by m and its sum over the three
 *              channels is divided by max(3 S(m valid), 1)
 *     imae, irmse as above with a m in place of a
 *     weight = #(a m > 0)                                                    :303-305
 *     mask pixels = S(m),  valid windows = S(m valid)  (per plane)
 *
 * Map values and the per-workgroup partial sums are fp32; the partial sums are reduced in a fixed
 * order in fp64 and the log10 / sqrt are fp64.  No atomics: two calls give the same bits.  IEEE
 * results are reported as they come (an exact match has psnr = +inf).
 *
 * Conventions as in gsr.h: device pointers unless said otherwise, fp32 contiguous images, `stream` a
 * hipStream_t, return GSR_OK or a negative gsr_status (gsr_last_error).
 */
#ifndef GSR_EVAL_H
#define GSR_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_EVAL_MAX_REGIONS 16
#define GSR_EVAL_FRAME_COLS 8  /* psnr, ssim, imae, irmse, weight, evaluated, mask pixels, valid windows */
#define GSR_EVAL_TOTAL_COLS 6  /* sum w psnr, sum w ssim, sum w imae, sum w irmse, sum w, images */

/* bits[i] |= 1 << (shift + k) where d >= lo[k] && d < hi[k], d = 1.0f / (gt_invdepth[i] + 1e-6f) in
 * fp32 (IEEE division).  lo, hi: host arrays of n_ranges floats (hi may be +inf); n >= 0 pixels;
 * shift + n_ranges <= 16. */
int gsr_eval_depth_range_bits(const float *gt_invdepth, int64_t n, int n_ranges, const float *lo, const float *hi,
                              int shift, uint16_t *bits, void *stream);

/* bits[i] |= 1 << (shift + k) where the pixel's three channels equal colour k.  seg_rgb_u8: (3, n)
 * bytes, planar; colors: host array of 3 n_colors bytes (r, g, b per colour); shift + n_colors <= 16. */
int gsr_eval_color_bits(const uint8_t *seg_rgb_u8, int64_t n, int n_colors, const uint8_t *colors, int shift,
                        uint16_t *bits, void *stream);

/* Scratch of gsr_eval_frame for an H x W frame with n_regions regions (0 on invalid arguments). */
size_t gsr_eval_frame_scratch_bytes(int H, int W, int n_regions);

/* The metric pass of one frame.  image, gt: (3, H, W), unclamped.  alpha_mask: (H, W) or NULL (all
 * ones).  invdepth, gt_invdepth: (H, W), or both NULL (imae = irmse = 0).  region_bits: (H, W) uint16,
 * or NULL when n_regions is 0; 0 <= n_regions <= 16.  frame: (1 + n_regions) x 8 doubles, see above. */
int gsr_eval_frame(const float *image, const float *gt, const float *alpha_mask, const float *invdepth,
                   const float *gt_invdepth, const uint16_t *region_bits, int n_regions, int H, int W,
                   void *scratch, double *frame, void *stream);

/* totals (n_rows x 6 doubles) += the frame's rows: w psnr, w ssim, w imae, w irmse, w, 1 with
 * w = weight.  Rows with evaluated == 0 or weight == 0 are skipped (the reference would add
 * inf * 0 = NaN for a region that lies wholly where alpha is 0). */
int gsr_eval_accumulate(const double *frame, int n_rows, double *totals, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_EVAL_H */
