// gsr_launch.h -- host-side launchers for the gfx950 kernels (one translation unit each).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "gsr_device.h"
#include "../../include/gsr.h"
#include "../../include/gsr_train.h"

namespace gsr {

// rasterizer.hip: message returned by gsr_last_error() for the calling thread.
void set_last_error(const std::string &msg);
// The end of a function that launched kernels: GSR_OK, or hipGetLastError()'s error as
// "<who>: <its text>" in the thread's message and GSR_ERR_DEVICE (the message is built on failure only).
int launched(const char *who);
// gsr_set_true_scale_gradient: dL/dscales including the scale_modifier factor (default off: upstream)
bool true_scale_gradient();

struct Camera {
    const float *view;  // device, 16
    const float *proj;  // device, 16
    const float *campos;  // device, 3
    float tanx, tany, fx, fy;
    int W, H, gx, gy;
};

// raw (the native train step, FrameOpts / BackwardOpts): scales / rotations / opacities are the
// pre-activation parameters (log-scales, unnormalised quaternions, logits), activated in the
// kernels that read them (gsr_device.h act_*), so no activated copy is written and re-read.
struct GaussianInputs {
    int P, D, M;
    const float *means3D, *shs, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp;
    float scale_modifier;
    int raw;
    // cut.ri != nullptr (render_post's blend fused, forwards without a backward): the P rows are
    // blended on the fly from the cut.N rows the pointers above address (gsr_device.h CutRef)
    CutRef cut{};
};
// the fused cut is supported for SH frames the colour pass takes (M = 16), scales + rotations
bool cut_fusable(const GaussianInputs &in);

// preprocess.hip
void launch_preprocess(const GaussianInputs &in, const Camera &cam, const GeomState &gs, int *radii,
                       hipStream_t s, bool split_color);
// SH colour of the visible Gaussians (rec.col, clamped) after a split_color preprocess
bool color_split_supported(const GaussianInputs &in);
// blocks > 0: a persistent grid of that many blocks (the pass held to part of the chip)
void launch_preprocess_color(const GaussianInputs &in, const Camera &cam, const GeomState &gs, const int *radii,
                             hipStream_t s, int blocks = 0);
// render.hip: the forward's launch order, tiles by descending list length; zero_classes != NULL: the
// backward class counters render_fwd fills are zeroed.
// fctl != NULL and fseg_len != 0: also the forward segments' item queue (FwdSegLayout in the
// binning buffer at bin_base; fctl = bwd_cnt + kFwdItemsWord).
void launch_tile_order(const uint2 *ranges, int T, int shift, uint32_t *order, hipStream_t s, const uint32_t *kdev,
                       uint32_t cap, uint32_t *zero_classes, uint32_t *fctl, void *bin_base, uint32_t seg_len,
                       uint32_t fseg_len, uint32_t *host_tilelist, uint32_t *fwd_ready, uint32_t fseg_min);
void launch_mark_visible(int P, const float *means3D, const float *view, uint8_t *present, hipStream_t s);

// sort.hip (rocPRIM)
// Stable LSD sort of n (key, value) pairs over key bits [0, end_bit) (kNN Morton order).
size_t sort_pairs_temp_bytes(size_t n, int end_bit);
hipError_t sort_pairs(void *tmp, size_t tmp_bytes, const uint32_t *kin, uint32_t *kout, const uint32_t *vin,
                      uint32_t *vout, size_t n, int end_bit, hipStream_t s);
// Stable sort of n (64-bit key, value) pairs over key bits [0, end_bit) (grid_cell.h's cell keys).
size_t sort_pairs64_temp_bytes(size_t n, int end_bit);
hipError_t sort_pairs64(void *tmp, size_t tmp_bytes, const uint64_t *kin, uint64_t *kout, const uint32_t *vin,
                        uint32_t *vout, size_t n, int end_bit, hipStream_t s);
// Runs of equal keys in a sorted array: each run's key and first position, and the number of runs.
size_t key_runs_temp_bytes(size_t n);
hipError_t key_runs(void *tmp, size_t tmp_bytes, const uint64_t *keys, size_t n, uint64_t *run_key,
                    uint32_t *run_start, uint32_t *n_runs, hipStream_t s);
// Exclusive prefix sum of n 32-bit counts (lidar.hip: the caller keeps the total below 2^32).
size_t scan_u32_temp_bytes(size_t n);
hipError_t scan_u32(void *tmp, size_t tmp_bytes, const uint32_t *in, uint32_t *out, size_t n, hipStream_t s);

// cell_grid.hip: the fp32 bounding box of the N rows of xyz with keep[i] != 0 (keep may be NULL: all),
// by ordered-integer atomics into eight words (grid_cell.h: kBBoxWords, bbox_words_init, ord2f) that
// the caller's own init kernel has set; whether a counted coordinate is NaN or Inf, and the rows counted.
void launch_bbox(int64_t N, const float *xyz, const uint8_t *keep, uint32_t *words, hipStream_t s,
                 int max_blocks = 1024);

// gtcloud.hip: what a query kernel needs of a gsr_gt_index (grid_cell.h)
struct GtGrid;
bool gt_grid_of(const void *index, GtGrid *out);  // false: NULL or not a live index
// T: the largest fp32 <= thr^2 (thr a double); reach: an fp32 upper bound of the per-axis distance
// of any point with d2 <= T.  false: thr not finite, <= 0 or thr^2 below the fp32 normal range
bool gt_thresholds(double thr, float *T, float *reach);
// out[i] = D_i (gsr_gtcloud.h) for rows with skip[i] == 0 (skip may be NULL), else 0
void launch_gt_far_mask(int64_t P, const float *xyz, const GtGrid &g, float T, float reach, const uint8_t *skip,
                        uint8_t *out, hipStream_t s);

// dsort.hip: the stable (depth bits, id) order of the P Gaussians (gs.order), depth-ordered tile
// rects (gs.drect, from gs.rect8), the Gaussian-major record offsets (rec.off) and
// K = sum of tiles_touched, stored to *dsort_K_word and, when host_K != NULL, to that pinned
// host word; k_ready (optional) is recorded once K is final, before the sort passes run.
int dsort_blocks(int P);
size_t dsort_ctrl_words(int P);
size_t dsort_ctrl_zero_words(int P);
// host_wide (optional, pinned; with host_K, stored before it): 1 when a visible key lies outside the
// three-pass window, so the frame's order came from the fourth pass.
// host_err (optional, pinned): set with a system-scope store when a lookback spin gives up.
void launch_depth_sort(int P, const GeomState &gs, uint32_t *host_K, uint32_t *host_wide, uint32_t *host_err,
                       hipStream_t s, hipEvent_t k_ready);
uint32_t *dsort_K_word(const GeomState &gs);
uint32_t *dsort_err_word(const GeomState &gs);
// a zeroed-per-frame control word the binning uses as a completion counter
uint32_t *dsort_aux_word(const GeomState &gs);
// local-sort frames: the longest SB list (sb_colscan); the head words (tickets, counters, K, ...)
// a frame re-run through the global sort must zero again
uint32_t *dsort_maxsb_word(const GeomState &gs);
// the forward split's queue-ready word (zeroed with the control words by every frame's preprocess)
uint32_t *dsort_fwdready_word(const GeomState &gs);
int device_cus();  // compute units of the current device (rasterizer.hip, cached per device)
uint32_t *dsort_live_words(const GeomState &gs);
uint32_t *dsort_culled_word(const GeomState &gs);  // culled Gaussians of the frame (the upsweep's sum)
int dsort_head_words();
// binning.hip: per-tile lists (two stable counting levels).  index_order: level 1 over the
// Gaussians in index order (local sort: sb_sort_bin orders each SB list by depth in LDS); else over
// dsort's depth order (gs.order / gs.drect; tile_bin).
SBGrid sb_grid(int gx, int gy, int P);
bool sb_grid_supported(const SBGrid &g);
int sort_cap();  // the longest SB list the local sort holds
int sort_blocks_per_cu();  // sb_sort_bin workgroups resident per CU (its launch bounds and LDS)
int debug_trace(int64_t *out, int n, int reset);  // GSR_SB_TRACE builds: sb_sort_bin phase stamps
// level-1 counts and SB bases; with fw.dev_K set (local sort) the column scan also stores K, the
// longest SB list and the level-1 total (FrameWords)
void launch_binning_count(int P, const Camera &cam, const GeomState &gs, bool index_order, const FrameWords &fw,
                          hipStream_t s, uint32_t tb_split = 0, uint32_t *host_sblist = nullptr);
void launch_binning_scatter(int P, const Camera &cam, const GeomState &gs, const BinningState &bs, bool index_order,
                            hipStream_t s);
// local_sort: sb_sort_bin (exits when *maxsb > sort_cap()); else tile_bin over depth-ordered lists
void launch_binning_tiles(int P, const Camera &cam, const GeomState &gs, const BinningState &bs, const ImageState &is,
                          bool local_sort, const uint32_t *maxsb, hipStream_t s, bool tb_split = false,
                          hipStream_t split_stream = nullptr);

// The gradient arrays render_bwd zeroes beside its replay (ZeroRows): up to six arrays (float
// counts n[k], 16-B aligned; unused entries n = 0) as one concatenated float4 range split evenly
// over the backward's workgroups (per4 float4 each; c4 the cumulative float4 counts).  render_bwd
// also stamps the Gaussians it stages (GeomState.live_stamp = this backward's stamp), and
// preprocess_bwd then runs the chain rule over the stamped rows only and writes nothing else.
constexpr int kZeroArrays = 6;
struct ZeroRows {
    float *p[kZeroArrays];
    uint64_t n[kZeroArrays];
    uint64_t c4[kZeroArrays + 1];
    uint64_t per4;
    uint32_t *stamps;  // != NULL: render_bwd stamps every staged Gaussian (live_stamp) with `stamp`
    uint32_t stamp;
};

// render.hip
void launch_render_fwd(const Camera &cam, const GeomState &gs, const BinningState &bs, const ImageState &is,
                       const float *bg, float *out_color, float *out_invdepth, hipStream_t s, bool need_bwd,
                       uint32_t seg_len, uint32_t fseg_len, hipStream_t worker_stream, bool workers_launched,
                       uint32_t fseg_min, FwdSpin spin);
// Forward segments' worker pool launched ahead of tile_order (on a side stream that has waited for
// the binning and the colour pass): its workgroups are resident before render_fwd's grid fills the
// CUs and start on the queue as soon as tile_order (given the same word) releases `ready`
// (dsort_fwdready_word: zero since the frame's preprocess).
void launch_render_fwd_workers(const Camera &cam, const GeomState &gs, const BinningState &bs, const ImageState &is,
                               const float *bg, float *out_color, float *out_invdepth, bool need_bwd, uint32_t seg_len,
                               uint32_t fseg_len, hipStream_t ws, const uint32_t *ready, FwdSpin spin);
// The pool's second launch, on the main stream after render_fwd when the pool was launched ahead:
// a small grid that takes whatever the early workers left in the queue (nothing, unless some gave up
// waiting for tile_order's ready word because the two streams did not run concurrently).
void launch_render_fwd_cleanup(const Camera &cam, const GeomState &gs, const BinningState &bs, const ImageState &is,
                               const float *bg, float *out_color, float *out_invdepth, bool need_bwd, uint32_t seg_len,
                               uint32_t fseg_len, hipStream_t s, FwdSpin spin);
// the workers' spin limits (gsr_set_fwd_spin_limits) with the pinned host words
FwdSpin fwd_spin(uint32_t *host_words);
void set_fwd_spin_limits(uint32_t ready, uint32_t flag);
// seg_len != 0: the backward's heavy tiles are cut into segments of seg_len list positions
// (gsr_set_bwd_segment; the backward must get the value its forward was made with)
void launch_render_bwd(const Camera &cam, const GeomState &gs, const BinningState &bs, const ImageState &is,
                       const int *radii, const float *bg, const float *dL_dpix, const float *dL_dinvdepth,
                       const BwdScratch &sc, hipStream_t s, const ZeroRows *zr = nullptr, uint32_t seg_len = 0);
bool bwd_segments_supported();
bool fwd_segments_supported();
uint32_t fseg_min_len(uint32_t Lf);  // the shortest list the forward split takes
uint32_t set_fwd_split_min(uint32_t len);  // gsr_set_fwd_split_min

// backward.hip
// sparse_rows (the native train step only, BackwardOpts): the rows of Gaussians with ten
// zero accumulated sums (every gradient zero) are not written in dmeans3D / dsh / dscales / drots,
// and dmeans2D's third column carries the row's liveness (1 written, 0 not) instead of its zero.
// Only rows whose opacity gradient is nonzero are read by the sparse Adam (OurAdam's `relevant`,
// train_single.py:226), and its dense fallback reads the liveness column.
struct GaussianGrads {
    float *dmeans2D, *dcolors, *dopacity, *dmeans3D, *dcov3D, *dsh, *dscales, *drots;
    int sparse_rows;
};

// The native step's activation backward fused into the live-row pass of preprocess_bwd
// (BackwardOpts.act): the gradient outputs are then the raw parameters'
// gradients (dscales / drots / dopacity: of the log-scales, the unnormalised quaternions and the
// logits, skybox rows' opacity gradient locked at zero, train_single.py:217-223), the
// densification statistics of every visible row are updated (train_single.py:193-194) and *flag
// is set when a row's opacity gradient is nonzero (OurAdam's `relevant`).  launch_preprocess_bwd
// returns whether it did it (else the caller runs the activation backward): only with raw inputs
// and sparse rows, and only on the split path.
struct StepAct {
    const float *s_raw, *o_raw;
    const float4 *q_raw;
    int64_t skybox;
    const int *radii;
    float *maxr, *accum, *denom;
    int *flag;
    int on;
};
bool live_list();  // gsr_set_live_list
bool launch_preprocess_bwd(const GaussianInputs &in, const Camera &cam, const GeomState &gs, const ImageState &is,
                           const int *radii, const BwdScratch &sc, const GaussianGrads &out, hipStream_t s,
                           const ZeroRows *zr = nullptr, const StepAct *step_act = nullptr);
// the frame's gradient arrays for render_bwd to zero and its live stamps (false: preprocess_bwd
// writes the zeros itself -- record mode, the single-kernel path or unaligned arrays)
bool bwd_zero_rows(const GaussianInputs &in, const GaussianGrads &out, const BwdScratch &sc, uint32_t *gs_stamps,
                   int nblocks, ZeroRows *z);

// rasterizer.hip: the bodies of gsr_rasterize_forward_ex / gsr_rasterize_backward: run() takes the
// C entry point's arguments (include/gsr.h; same checks and errors), the members are the options
// only the native train step sets -- the C entry points run them with the defaults.
// raw_params: plain frames only (no precomputed covariance, no hierarchy cut).
struct ForwardCall {
    bool raw_params = false;  // GaussianInputs.raw
    decltype(gsr_rasterize_forward_ex) run;
};
struct BackwardCall {
    bool raw_params = false, sparse_rows = false;  // GaussianInputs.raw, GaussianGrads.sparse_rows
    const StepAct *act = nullptr;                  // NULL: none
    bool act_done = false;                         // out: run() did the fused activation backward
    decltype(gsr_rasterize_backward) run;
};

// loss.hip (the image side) and optim.hip (the Gaussian side): the native train step's fused
// launches (train_step.hip).  What a launch works on is passed as one struct per term of the step,
// filled by member name in gsr_train_step.

// torch applies these python floats as fp32 scalars: b and (1 - b) are rounded from the double
struct AdamHyper {
    double beta1, beta2, eps;
};

// The photometric term (train_single.py:121-123) of one view, shared by step_loss_forward and
// step_loss_backward.
struct PhotoTerms {
    const float *img;  // (3, H, W): the exposed image (x the alpha mask)
    const float *gt;   // (3, H, W): the target
    int H, W;
    double lambda_dssim;
    const float *one;    // device: dL/dloss (1)
    const float *alpha;  // (H, W) or NULL
    // (3, H, W), written by the forward: the SSIM gradient field G (the tile kernel), or the
    // photometric gradient itself (dL/dloss = *one, times alpha when given; the streaming kernel).
    // gmap_is_photo says which: the forward sets it, the backward reads it.
    float *gmap;
    bool gmap_is_photo = false;
};

// The masked inverse-depth L1 (train_single.py:135-141), or the depth-only view's loss
// (gsr_depth_only_loss), with its gradient for an upstream of 1 in d_invd.
struct DepthTerms {
    const float *invd;  // rendered
    const float *mono;  // target; NULL: no depth term
    const float *mask;  // or NULL
    float weight;
    void *scratch;  // gsr_depth_l1_scratch_bytes / gsr_depth_only_scratch_bytes
    float *d_invd;
};

// The view's exposure: colour -> exposed image (launch_exposure_forward: color, E, npix), and in
// step_loss_backward the colour gradient, the exposure gradient and the exposure optimizer's step.
struct ExposureTerms {
    const float *color;  // rendered (3, H, W)
    const float *E;      // the view's 3 x 4 (row `view` of the group's n_images x 12 parameter)
    int64_t npix;
    float *d_color;
    void *scratch;  // gsr_exposure_scratch_bytes
    int n_images, view;
    gsr_adam_group group;
    float *grad;  // n_images x 12
    AdamHyper adam;
};

// What the native step adds to gsr_sparse_adam_step (the defaults: that entry point as it is).
struct SparseAdamOpts {
    bool flag_ready = false;  // the relevance flag is already computed: no any-nonzero pass
    // train_single.py:235-241's scale shrink of rows >= shrink_first in the same launch (NULL: none)
    float *shrink_raw = nullptr;
    int64_t shrink_first = 0;
    float shrink_limit = 0.f;
    // live3 != NULL (sparse gradient rows): when no row is relevant, the dense fallback takes a zero
    // gradient for rows whose live3[3 row + 2] is 0 (never written) and for the locked skybox rows
    // below `skybox` (train_single.py:217-223 zeroes all six of their gradients).
    const float *live3 = nullptr;
    int64_t skybox = 0;
    // scratch of >= P + 64 ints for the compacted row list (the train context's grow-only slot);
    // NULL: allocated per call in stream order, and the row-block kernel (no scratch) runs when
    // that allocation fails.
    int *row_list = nullptr;
};
int sparse_adam(int n_groups, const gsr_adam_group *groups, int64_t P, const float *relevance, int *flag_scratch,
                const AdamHyper &hyper, const SparseAdamOpts &opts, hipStream_t s);

// SSIM map forward (+ the depth term's forward with its gradient when depth.mono != NULL) and the
// loss epilogue: losses[0..2] photometric, [3..4] depth, [5] total; *flag = 0.
int step_loss_forward(PhotoTerms &photo, const DepthTerms &depth, void *loss_scratch, float *losses, int *flag,
                      hipStream_t s);
// the depth-only view's loss over n pixels (dens_weight: additional_depth_maps_weight);
// losses = (dens, 0, 0, pure, loss, loss); *flag = 0
int step_depth_only_forward(const DepthTerms &depth, int64_t n, double dens_weight, float *losses, int *flag,
                            hipStream_t s);
int launch_exposure_forward(const ExposureTerms &exposure, float *out, const float *alpha, hipStream_t s);
// photometric gradient (x alpha) through the exposure into d_color, the exposure gradient and the
// exposure optimizer's dense Adam step
int step_loss_backward(const PhotoTerms &photo, const ExposureTerms &exposure, hipStream_t s);

// What step_activate_backward takes beside the StepAct the fused form takes: the rasterizer
// backward's gradients of the activated parameters, the raw parameters' gradients it writes, and
// the screen-space gradient.  sparse_rows: the rasterizer backward wrote sparse rows
// (GaussianGrads): the scale / rotation gradients of rows it did not write are neither read nor
// written.
struct ActGrads {
    const float *d_scales, *d_rots, *d_opac;
    float *scaling_grad, *rotation_grad, *opacity_grad;
    const float *d_means2D;
    bool sparse_rows;
};
// activation backward + skybox lock + relevance flag + densification statistics, the activations
// recomputed from the raw parameters (act.s_raw, q_raw, o_raw)
int step_activate_backward(int64_t P, const StepAct &act, const ActGrads &grads, hipStream_t s);

// kernel stamps of each translation unit (GSR_KSTAMP builds; gsr_kstamp_read)
int kstamp_read_preprocess(unsigned long long *out);
int kstamp_read_dsort(unsigned long long *out);
int kstamp_read_binning(unsigned long long *out);
int kstamp_read_render(unsigned long long *out);
int kstamp_read_backward(unsigned long long *out);

}  // namespace gsr
