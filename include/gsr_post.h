/*
 * gsr_post.h -- C ABI of the native post-optimisation iteration (train_post.py:69-198, as
 * gs_train/post.py PostTrainStep.step drives it from Python) and of its optimizer kernel.
 * Exported by libgsr_hip.so (csrc/post_step.hip; the mark kernel beside cut_row in csrc/hier.hip).
 *
 *   gsr_post_adam_step   replaces train_post.py:167-181 (the locked rows' gradients zeroed),
 *                        :191-192 (torch.optim.Adam over every row) and the zero-fill of the five
 *                        N-row gradients, over PERSISTENT gradient buffers that are all zero bits
 *                        between iterations
 *   gsr_cut_mark_rows    names the rows one iteration's blend backward touched
 *   gsr_post_step        one whole iteration as ONE host call
 *
 * Conventions as in gsr.h: device pointers, fp32, contiguous, `stream` a hipStream_t.  New entry
 * points of ABI 7 (nothing existing changes).
 */
#ifndef GSR_POST_H
#define GSR_POST_H

#include <stddef.h>
#include <stdint.h>

#include "gsr_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* stamp[row] = value for every row gsr_interpolate_cut_backward_act writes or accumulates into for
 * this cut: the child render_indices[r] of each of the R cut rows, its parent parent_indices[r]
 * (-1, a root's, wraps to row N - 1 as in the blend) and the last S (skybox) rows.  One launch over
 * R + S rows; rows named several times get the same value from each (plain stores). */
int gsr_cut_mark_rows(int64_t N, int64_t R, int64_t S, const int *render_indices, const int *parent_indices,
                      const float *interpolation_weights, int *stamp, int value, void *stream);

/* live[row] = 1 when any element of any group's exp_avg / exp_avg_sq row has a nonzero BIT PATTERN
 * (a stored -0.0 counts: the update turns it into +0.0), else 0.  One pass over the moments: at
 * set-up and after a checkpoint restore. */
int gsr_post_live_build(int n_groups, const gsr_adam_group *groups, int64_t N, uint8_t *live, void *stream);

/* The post-optimisation's optimizer step over persistent gradients, one launch.  groups: as
 * gsr_sparse_adam_step takes them (whole-row arrays, or a column-split pair of one buffer such as
 * the DC / rest SH blocks; any other column block: GSR_ERR_UNSUPPORTED).  Per row:
 *   stamp[row] == cur, locked (row >= N - tail, or lock[row] != 0):  its gradient rows zeroed
 *   stamp[row] == cur, not locked:  the Adam update with the gradient read, the gradient rows
 *                                   zeroed, live[row] = 1
 *   stamp[row] != cur, live[row]:   the Adam update with g = 0 (the gradient neither read nor written)
 *   stamp[row] != cur, not live:    nothing
 * Provided every gradient row with stamp != cur is all zero bits and live is gsr_post_live_build's
 * (or this function's) result, parameters and moments are the bits gsr_zero_grad_rows followed by
 * gsr_sparse_adam_step(relevance = NULL) give, and every gradient is zero bits on return.
 * lock may be NULL (no locked row beside the tail). */
int gsr_post_adam_step(int n_groups, const gsr_adam_group *groups, int64_t N, const int *stamp, int cur,
                       uint8_t *live, int64_t tail, const uint8_t *lock, double beta1, double beta2, double eps,
                       void *stream);

/* ---- the iteration ------------------------------------------------------------------------
 * gsr_post_step runs, on the caller's stream and in PostTrainStep.step's order: gsr_expand_to_size
 * (the host reads the cut length), gsr_interpolation_weights, gsr_interpolate_cut_forward_act
 * (GSR_OPACITY_ABS), gsr_rasterize_forward_ex, the view's exposure + clamp (gsr_exposure_forward;
 * exposure NULL: the clamp alone), image x alpha_mask, gsr_photo_loss_forward / _backward, the
 * exposure backward, gsr_rasterize_backward (every gradient row written),
 * gsr_interpolate_cut_backward_act (GSR_CUT_UNIQUE_CHILDREN) into the caller's persistent
 * gradients, gsr_cut_mark_rows and gsr_post_adam_step.
 * The context owns the cut buffers, the blended rows, the rasterizer's buffers, the images, the row
 * stamps and `live` (grow-only, grown in stream order); the caller owns the parameters, the moments
 * (through `groups`) and the five N-row gradient buffers, which are zero on entry and zero on
 * return. */
typedef struct gsr_post_ctx gsr_post_ctx;
gsr_post_ctx *gsr_post_ctx_create(void);
/* Waits for the last step's stream, then frees the context's device buffers. */
void gsr_post_ctx_destroy(gsr_post_ctx *ctx);
/* out[0] = buffer growths since creation, out[1] = bytes held, out[2] = 1 (stream-ordered growth),
 * as gsr_train_ctx_stats.  Returns the number of values written (<= n). */
int gsr_post_ctx_stats(const gsr_post_ctx *ctx, int64_t *out, int n);
/* Copies the context's row state of the last step's N rows into a device buffer, in the order of
 * the last step's stream: what = 0: live (N bytes), 1: stamp (N int32; 0 = never stamped) and
 * *cur (optional) = the last step's stamp value. */
int gsr_post_ctx_read_rows(gsr_post_ctx *ctx, int what, void *dst, int64_t n, int *cur);

typedef struct {
    int64_t N;         /* rows (hierarchy Gaussians, the skybox's last) */
    int64_t n_nodes;   /* hierarchy nodes */
    int M, D;          /* SH coefficients per row (features is (N, M, 3)), active degree */
    int64_t skybox;    /* S: the last rows, rendered unblended and locked */
    int width, height;
    const int *nodes;    /* (n_nodes, 7) */
    const float *boxes;  /* (n_nodes, 2, 4) */
    /* raw parameters (updated in place) and their persistent gradients (zero on entry and return) */
    float *xyz, *features, *opacity, *scaling, *rotation;
    float *xyz_grad, *features_grad, *opacity_grad, *scaling_grad, *rotation_grad;
    int n_groups;
    const gsr_adam_group *groups; /* their grad pointers lie inside the gradients above */
    double beta1, beta2, eps;
    const uint8_t *lock;          /* (N) nonzero = an anchor row; NULL: none */
    int rebuild_live;             /* nonzero: live is rebuilt from the moments first (set-up, restore) */
    /* the view */
    const float *viewmatrix, *projmatrix, *campos; /* device: 16, 16, 3 */
    float campos_host[3];                           /* the same centre, for the interpolation weights */
    float tan_fovx, tan_fovy;
    const float *background;                        /* device: 3 */
    float limit;                                    /* the LOD target size of this iteration */
    const float *gt;                                /* (3, H, W) */
    const float *alpha_mask;                        /* (H, W) or NULL */
    const float *exposure;                          /* device 3 x 4 of the view, or NULL (clamp only) */
    double lambda_dssim;
    float *losses;                                  /* device, 3 floats: L1, SSIM, the loss */
    void *stream;
} gsr_post_step_args;

/* *cut_rows receives the cut length R, *num_rendered the frame's K (either may be NULL). */
int gsr_post_step(gsr_post_ctx *ctx, const gsr_post_step_args *args, int64_t *cut_rows, int64_t *num_rendered);

#ifdef __cplusplus
}
#endif
#endif /* GSR_POST_H */
