/*
 * gsr_views.h -- C ABI of the training views kept compact on the device: Pillow's 8-bit Lanczos resize,
 * and the expansion of a compact view (RGB8, mask8, source-resolution depth16) into the float32 planes
 * the train step, the coarse and post steps and the evaluator read.  Exported by libgsr_hip.so.
 *
 * Replaces, between a decoded image and the step, the reference's utils/camera_utils.py:22-92 (loadCam),
 * utils/general_utils.py:22-29 (PILtoTorch) and scene/cameras.py:47-88 (Camera.__init__), which run on
 * DataLoader workers with PIL and OpenCV.  File decoding and RGBA images stay with the caller.
 *
 * (a) Lanczos resize: Image.resize(size, Image.LANCZOS) of an 8-bit image with 1 or 3 interleaved
 * channels, bit for bit (pinned to Pillow by tests/golden/views.npz and, where Pillow is installed,
 * to Pillow itself).  Per axis, in double, with scale = in / out:
 *   fs = max(scale, 1), support = 3 fs, ksize = 2 ceil(support) + 1
 *   for output xx:  center = (xx + 0.5) scale
 *                   xmin = max((int)(center - support + 0.5), 0)        C truncation
 *                   xmax = min((int)(center + support + 0.5), in)
 *                   tap x in [0, xmax - xmin):  w_x = L((x + xmin - center + 0.5) / fs)
 *   L(t) = sinc(t) sinc(t / 3) on -3 <= t < 3 and 0 elsewhere; sinc(0) = 1, sinc(t) = sin(pi t) / (pi t)
 *   w_x /= sum of the w_x, the sum accumulated in tap order (left alone when the sum is 0)
 *   coeff_x = (int)(w_x 2^22 + 0.5) for w_x >= 0, (int)(w_x 2^22 - 0.5) for w_x < 0, truncating
 * An output sample is clip8((2^21 + sum_x coeff_x src[xmin + x]) >> 22): a signed 32-bit sum, an
 * arithmetic shift.  The horizontal pass runs first, into a uint8 image of out_w x in_h, the vertical
 * pass on that image; a pass whose axis keeps its size is skipped; the uint8 rounding between the
 * passes is part of the result.  The tables are made on the host, in double with libm's sin, as
 * Pillow makes them -- a device sin differs in the last place, and a coefficient that rounds the other
 * way moves samples by 1 -- and uploaded once per plan.
 * 4 channels are refused: Pillow premultiplies an RGBA image's colour by its alpha around the filter,
 * so filtering four plain channels is not what it computes.
 *
 * (b) View expansion, per pixel (x, y) of the W x H view, fp32, every operation rounded once, nothing
 * contracted:
 *   alpha     = (float)mask / 255.0f (an IEEE division), 1 without a mask; 0 where zero_half says so
 *               (1: x < W / 2, 2: x >= W / 2 -- scene/cameras.py:56-60, W / 2 the integer quotient)
 *   image[c]  = min(max((float)rgb[c] / 255.0f, 0), 1) * alpha; 0 without rgb (a depth-only view's
 *               black image)
 *   depth: S(i, j) = ((float)u16 / 65536.0f * scale) + offset at the source resolution (dW x dH),
 *               two rounded operations; resized to W x H by the linear rule below; negatives set to 0
 *   depth_mask = alpha; with depth_valid = 1 also 0 where the inverse depth is 0
 * The linear rule (OpenCV's float32 INTER_LINEAR as this project states it; OpenCV cannot be run beside
 * this project, so the rule is parity-unpinned), per axis with in source and out target samples:
 *   f = (float)((d + 0.5) * ((double)in / out) - 0.5), i = floor(f), f -= i
 *   i < 0: i = 0, f = 0;   i >= in - 1: i = in - 1, f = 0, the second tap replicated
 *   h(j)  = (1 - fx) S(j, ix) + fx S(j, ix + 1)            products rounded, then the sum
 *   value = (1 - fy) h(iy) + fy h(iy + 1)                  likewise; equal sizes give S itself
 *
 * Conventions as in gsr.h: device pointers unless said otherwise, `stream` a hipStream_t, GSR_OK or a
 * negative gsr_status with the message in gsr_last_error().
 */
#ifndef GSR_VIEWS_H
#define GSR_VIEWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The coefficient tables of one resize geometry (host arithmetic only: no device is touched until the
 * first gsr_resize_lanczos_u8).  1 <= every size <= 32768; NULL otherwise. */
void *gsr_resize_plan_create(int in_w, int in_h, int out_w, int out_h);
/* Frees the plan and its device tables.  NULL is a no-op. */
void gsr_resize_plan_destroy(void *plan);
/* out[0..n) (host): table uploads so far, ksize of the horizontal and of the vertical axis (0: pass
 * skipped), bytes of the device tables, bytes of scratch per channel. */
int gsr_resize_plan_info(const void *plan, int64_t *out, int n);
/* The host tables of axis 0 (horizontal) or 1 (vertical): bounds (out, 2) int32 xmin and tap count,
 * coeffs (out, ksize) int32, zero past the count.  Host pointers.  A skipped axis is an error. */
int gsr_resize_plan_tables(const void *plan, int axis, int32_t *bounds, int32_t *coeffs);
/* Bytes of scratch gsr_resize_lanczos_u8 needs (the out_w x in_h intermediate; 0 unless both passes run). */
size_t gsr_resize_scratch_bytes(const void *plan, int channels);
/* dst (out_h, out_w, C) = the resize (a) of src (in_h, in_w, C), uint8, C = channels = 1 or 3.  src, dst
 * and scratch are 4-byte aligned and do not overlap.  The first call uploads the plan's tables (and
 * synchronises the device for it); later calls on the same device upload nothing. */
int gsr_resize_lanczos_u8(void *plan, const uint8_t *src, int channels, void *scratch, uint8_t *dst, void *stream);

/* One launch of the expansion (b).  rgb (H, W, 3) uint8 or NULL; mask (H, W) uint8 or NULL; depth
 * (dH, dW) uint16 or NULL with invdepth and depth_mask NULL too.  image (3, H, W), alpha, invdepth and
 * depth_mask (H, W) float32, each 16-byte aligned; rgb and mask 4-byte aligned.  zero_half 0, 1, 2;
 * depth_valid 0, 1; scale and offset finite.  1 <= W, H, dW, dH <= 32768.  The caller decides that a view
 * has depth planes (scale > 0): with depth given they are written. */
int gsr_view_expand(int W, int H, const uint8_t *rgb, const uint8_t *mask, int zero_half, const uint16_t *depth, int dW,
                    int dH, float scale, float offset, int depth_valid, float *image, float *alpha, float *invdepth,
                    float *depth_mask, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_VIEWS_H */
