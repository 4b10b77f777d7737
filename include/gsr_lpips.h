/*
 * gsr_lpips.h -- C ABI of the LPIPS (VGG16, v0.1) evaluation metric around a caller-run convolution
 * trunk, whole-image and per-region.  Exported by libgsr_hip.so.
 *
 * The reference (render_hierarchy_final.py:142-157, lpipsPyTorch/modules/lpips.py:32-66) runs the
 * whole network once per row of its table and applies the region mask in the last step.  The trunk's
 * inputs do not depend on the region, so here one trunk pass over the batch (image, gt) serves every
 * row: gsr_lpips_prepare builds the batch, the caller runs the 13 convolutions, and after each of
 * the five stages gsr_lpips_tap reads that stage's pre-ReLU feature maps once and leaves the stage's
 * term of every row, and the pooled input of the next stage.  The weights are the caller's; nothing
 * here loads or fetches any.
 *
 * With X, Y the ReLU'd features of the two images at a stage ((C, h, w) each), w_c the stage's
 * linear weights and p a feature pixel:
 *
 *   nx(p) = sqrt(sum_c X_c(p)^2),  xh_c = X_c / (nx + 1e-10), likewise yh    lpipsPyTorch/modules/utils.py:6-8
 *   d(p)  = sum_c w_c (xh_c(p) - yh_c(p))^2
 *   row 0     = sum_p d(p) / (h w)                                            modules/lpips.py:39
 *   row 1 + r = sum_p d(p) m_r(p) / max(sum_p m_r(p), 1e-8)                   modules/lpips.py:51-62
 *
 * m_r(p) is bit r of region_bits at the full-resolution pixel F.interpolate(mode='nearest') reads for
 * p: row min((int)floorf(i * ((float)H / h)), H - 1) in fp32, and the same rule for the column.
 * The frame's LPIPS of a row is the sum of the five stages' terms.
 *
 * The terms of nx, ny and d are fp32 in the reference's operation order; they are added over the channels
 * and within a workgroup in fp64, each workgroup's sums are rounded to fp32, and those are reduced in a
 * fixed order in fp64.  No atomics: two calls give the same bits, and a region's row does
 * not depend on which other regions are asked for.
 *
 * Conventions as in gsr.h: device pointers unless said otherwise, fp32 contiguous tensors, `stream` a
 * hipStream_t, return GSR_OK or a negative gsr_status (gsr_last_error).
 */
#ifndef GSR_LPIPS_H
#define GSR_LPIPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_LPIPS_MAX_REGIONS 16
#define GSR_LPIPS_STAGES 5
#define GSR_LPIPS_TOTAL_COLS 2 /* sum w lpips, sum w */

/* batch (2, 3, H, W): batch[0] from image, batch[1] from gt, each value
 * (clamp(v, 0, 1) * a - mean_c) / std_c in IEEE fp32 in that order, with a = alpha_mask (1 when NULL),
 * mean = (-.030, -.088, -.188), std = (.458, .448, .450) (modules/networks.py:41-44).
 * image, gt: (3, H, W), unclamped; alpha_mask: (H, W) or NULL. */
int gsr_lpips_prepare(const float *image, const float *gt, const float *alpha_mask, int H, int W, float *batch,
                      void *stream);

/* Scratch of gsr_lpips_tap for (h, w) feature maps with n_regions regions (0 on invalid arguments). */
size_t gsr_lpips_tap_scratch_bytes(int h, int w, int n_regions);

/* One stage.  features: (2, C, h, w), the pre-ReLU output of the stage's last convolution (the ReLU
 * is applied as the values are loaded).  lin: C weights.  region_bits: (H, W) uint16, or NULL when
 * n_regions is 0; 0 <= n_regions <= 16; H >= h, W >= w.  pooled_out: NULL, or (2, C, h / 2, w / 2):
 * the 2x2 / stride-2 floor-mode max pool of the ReLU'd features.  out: (1 + n_regions) doubles, the
 * stage's term of every row. */
int gsr_lpips_tap(const float *features, const float *lin, int C, int h, int w, const uint16_t *region_bits,
                  int n_regions, int H, int W, float *pooled_out, void *scratch, double *out, void *stream);

/* totals (n_rows x 2 doubles) += (w lpips, w) with w = frame[row][4] for every row gsr_eval_accumulate
 * counts: frame[row][5] (evaluated) != 0 and w != 0.  lpips: n_rows doubles; frame: the n_rows x 8
 * table of gsr_eval_frame (include/gsr_eval.h) for the same frame. */
int gsr_lpips_accumulate(const double *lpips, const double *frame, int n_rows, double *totals, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_LPIPS_H */
