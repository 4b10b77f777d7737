// post_step.hip -- the native post-optimisation iteration (include/gsr_post.h): gsr_post_step runs one
// train_post.py iteration (:69-198) as one host call, through the entry points gs_train/post.py
// PostTrainStep.step reaches from Python and in its order, and ends in gsr_post_adam_step, the
// optimizer step over persistent gradient buffers.
//
// What the Python step pays around the blend and the rasterizer: _CutAct.backward zero-fills five
// N-row gradient tensors (59 floats per row) every iteration, gsr_zero_grad_rows clears the locked
// rows, and the dense Adam then reads those gradients and reads and writes parameters and moments
// of EVERY row (28 B per float), although a cut reaches only part of the hierarchy and a row no cut
// has reached yet has zero gradient and zero moments: its update is the identity, bit for bit
// (m b1 + (1 - b1) 0 = +0, v likewise, p + (-ss) (0 / eps) = p + (-0) = p for every p, +-0 included).
// Here the gradients live in buffers that are all zero bits between iterations; the blend backward
// writes the rows of this cut, gsr_cut_mark_rows stamps them, and post_adam_kernel looks the state of
// every row up once per 64-row tile: stamped rows are updated with their gradient, which is cleared
// behind the read; rows with nonzero moments (`live`) decay with g = 0 without touching a gradient;
// the rest costs 6 bytes per row and array.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>

#include "../../include/gsr.h"
#include "../../include/gsr_hier.h"
#include "../../include/gsr_post.h"
#include "../../include/gsr_train.h"
#include "gsr_adam.h"
#include "gsr_launch.h"

namespace gsr {
namespace {

// ---------------------------------------------------------------------------------------------
// The optimizer kernel.  One wave per (64 consecutive rows, array): lane l looks up the state of row
// r0 + l (4 B of stamp, 1 B of live, 1 B of lock), a ballot ends the wave when no row of the tile has
// anything to do.  The tile's rows are one contiguous span of each array, so a wide array (the
// 48-float SH rows) is walked as float4, row / 4 per row, each float4 taking its row's action from
// the owner lane by shuffle; a narrow array (1, 3, 4 floats) is updated lane = row.  The row is the
// granularity of the look-up because the flat kernel's 2048-float blocks end inside rows (48- and
// 3-float rows), and a tile of whole rows keeps every access of an idle row's gradient out.
// What a row needs, as flags: kClear its gradient rows zeroed, kUpdate the Adam update, kRead the
// update reads the gradient (otherwise g = 0 and the gradient is not touched).
//   stamped, locked    kClear (and kUpdate when live: with moments from elsewhere the dense step would
//                      decay them; a locked row trained here never has any)
//   stamped, unlocked  kClear | kUpdate | kRead
//   idle, live         kUpdate
enum RowAction { kRowNone = 0, kClear = 1, kUpdate = 2, kRead = 4 };

struct PostAdamArgs {
    FlatAdamRun r[kMaxGroups];
    int n;
};

constexpr int kPostThreads = 256;
constexpr int kPostBatch = 3;  // float4 per lane and trip, loads first (12 float4 per SH row: 4 trips per tile)

__device__ __forceinline__ float col_step(const FlatAdamRun &R, int col) { return col < R.split_col ? R.step0 : R.step1; }

template <int kW>
__device__ __forceinline__ void post_adam_narrow(const FlatAdamRun &R, int64_t base, int act, float b1, float b2,
                                                 float omb1, float omb2, float eps) {
    float *grad = const_cast<float *>(R.grad);
    if (act & kUpdate) {
        float g[kW], m[kW], v[kW], p[kW];
#pragma unroll
        for (int c = 0; c < kW; c++) {
            g[c] = (act & kRead) ? R.grad[base + c] : 0.f;
            m[c] = R.exp_avg[base + c];
            v[c] = R.exp_avg_sq[base + c];
            p[c] = R.param[base + c];
        }
#pragma unroll
        for (int c = 0; c < kW; c++) {
            flat_adam_one(R, p[c], m[c], v[c], g[c], col_step(R, c), b1, b2, omb1, omb2, eps);
            R.exp_avg[base + c] = m[c];
            R.exp_avg_sq[base + c] = v[c];
            R.param[base + c] = p[c];
        }
    }
    if (act & kClear) {
#pragma unroll
        for (int c = 0; c < kW; c++) grad[base + c] = 0.f;
    }
}

__global__ __launch_bounds__(kPostThreads) void post_adam_kernel(PostAdamArgs a, int64_t N,
                                                                 const int *__restrict__ stamp, int cur,
                                                                 uint8_t *live, int64_t tail,
                                                                 const uint8_t *__restrict__ lock, float b1, float b2,
                                                                 float omb1, float omb2, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t r0 = (((int64_t)blockIdx.x * kPostThreads + threadIdx.x) >> 6) * 64;
    if (r0 >= N) return;  // wave-uniform
    const int64_t row = r0 + lane;
    int act = kRowNone;
    bool step = false;
    if (row < N) {
        const bool is_live = live[row] != 0;
        if (stamp[row] == cur) {
            const bool locked = row >= N - tail || (lock != nullptr && lock[row] != 0);
            step = !locked;
            act = locked ? (kClear | (is_live ? kUpdate : 0)) : (kClear | kUpdate | kRead);
        } else if (is_live) {
            act = kUpdate;
        }
    }
    if (__ballot(act != kRowNone) == 0) return;  // wave-uniform: nothing to do in this tile
    const FlatAdamRun &R = a.r[blockIdx.y];
    // only rows whose action no longer depends on live are set, so the other arrays' waves of the
    // tile may read it meanwhile
    if (blockIdx.y == 0 && step) live[row] = 1;
    const int w = R.row;
    if (R.vec && w > 4) {
        const int q = w >> 2;      // float4 per row
        const int tot = 64 * q;    // of the tile (rows past N: no action)
        float *grad = const_cast<float *>(R.grad);
        for (int f0 = 0; f0 < tot; f0 += 64 * kPostBatch) {
            float4 g[kPostBatch], m[kPostBatch], v[kPostBatch], p[kPostBatch];
            int ac[kPostBatch], col[kPostBatch];
            int64_t off[kPostBatch];
#pragma unroll
            for (int h = 0; h < kPostBatch; h++) {
                const int f = f0 + 64 * h + lane;
                const int rl = min(f / q, 63);
                const int ra = __shfl(act, rl, 64);
                ac[h] = f < tot ? ra : kRowNone;
                col[h] = 4 * (f - rl * q);
                off[h] = (r0 + rl) * (int64_t)w + col[h];
                g[h] = m[h] = v[h] = p[h] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ac[h] & kRead) g[h] = *reinterpret_cast<const float4 *>(R.grad + off[h]);
                if (ac[h] & kUpdate) {
                    m[h] = *reinterpret_cast<const float4 *>(R.exp_avg + off[h]);
                    v[h] = *reinterpret_cast<const float4 *>(R.exp_avg_sq + off[h]);
                    p[h] = *reinterpret_cast<const float4 *>(R.param + off[h]);
                }
            }
#pragma unroll
            for (int h = 0; h < kPostBatch; h++) {
                if (ac[h] & kUpdate) {
                    flat_adam_one(R, p[h].x, m[h].x, v[h].x, g[h].x, col_step(R, col[h] + 0), b1, b2, omb1, omb2, eps);
                    flat_adam_one(R, p[h].y, m[h].y, v[h].y, g[h].y, col_step(R, col[h] + 1), b1, b2, omb1, omb2, eps);
                    flat_adam_one(R, p[h].z, m[h].z, v[h].z, g[h].z, col_step(R, col[h] + 2), b1, b2, omb1, omb2, eps);
                    flat_adam_one(R, p[h].w, m[h].w, v[h].w, g[h].w, col_step(R, col[h] + 3), b1, b2, omb1, omb2, eps);
                    *reinterpret_cast<float4 *>(R.exp_avg + off[h]) = m[h];
                    *reinterpret_cast<float4 *>(R.exp_avg_sq + off[h]) = v[h];
                    *reinterpret_cast<float4 *>(R.param + off[h]) = p[h];
                }
                if (ac[h] & kClear) *reinterpret_cast<float4 *>(grad + off[h]) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        return;
    }
    if (act == kRowNone) return;
    const int64_t base = row * (int64_t)w;
    switch (w) {
        case 1: post_adam_narrow<1>(R, base, act, b1, b2, omb1, omb2, eps); break;
        case 3: post_adam_narrow<3>(R, base, act, b1, b2, omb1, omb2, eps); break;
        case 4: post_adam_narrow<4>(R, base, act, b1, b2, omb1, omb2, eps); break;
        default: {
            // any other width (or an unaligned wide array): one element at a time, its own column's step
            float *grad = const_cast<float *>(R.grad);
            for (int c = 0; c < w; c++) {
                if (act & kUpdate) {
                    float p = R.param[base + c], m = R.exp_avg[base + c], v = R.exp_avg_sq[base + c];
                    const float g = (act & kRead) ? R.grad[base + c] : 0.f;
                    flat_adam_one(R, p, m, v, g, col_step(R, c), b1, b2, omb1, omb2, eps);
                    R.exp_avg[base + c] = m;
                    R.exp_avg_sq[base + c] = v;
                    R.param[base + c] = p;
                }
                if (act & kClear) grad[base + c] = 0.f;
            }
        }
    }
}

// live[row] = some moment element of the row has a nonzero bit pattern (set-up and restore only)
__global__ __launch_bounds__(256) void post_live_kernel(PostAdamArgs a, int64_t N, uint8_t *__restrict__ live) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= N) return;
    uint32_t bits = 0;
    for (int k = 0; k < a.n; k++) {
        const FlatAdamRun &R = a.r[k];
        const int64_t base = row * (int64_t)R.row;
        for (int c = 0; c < R.row; c++)
            bits |= __float_as_uint(R.exp_avg[base + c]) | __float_as_uint(R.exp_avg_sq[base + c]);
    }
    live[row] = bits != 0 ? 1 : 0;
}

int post_runs(int n_groups, const gsr_adam_group *groups, int64_t N, PostAdamArgs &pa, const char *who) {
    if (n_groups < 0 || n_groups > kMaxGroups || N < 0 || N > 0x7fffffff || (n_groups > 0 && !groups)) {
        set_last_error(std::string(who) + ": bad group count, row count or NULL groups");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    for (int i = 0; i < n_groups; i++) {
        const gsr_adam_group &g = groups[i];
        if (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq || g.width <= 0 ||
            (g.row_stride != 0 && g.row_stride < g.width)) {
            set_last_error(std::string(who) + ": group has a NULL array, non-positive width or row_stride < width");
            return GSR_ERR_INVALID_ARGUMENT;
        }
    }
    FlatAdamArgs fa;
    int rest[kMaxGroups], n_rest = 0;
    flat_adam_runs(n_groups, groups, N, fa, rest, n_rest);
    if (n_rest > 0) {
        set_last_error(std::string(who) + ": every group must be whole rows or one half of a column-split pair");
        return GSR_ERR_UNSUPPORTED;
    }
    std::memset(&pa, 0, sizeof(pa));
    pa.n = fa.n;
    for (int k = 0; k < fa.n; k++) pa.r[k] = fa.r[k];
    return GSR_OK;
}

// ---------------------------------------------------------------------------------------------
// The image-side steps the Python iteration runs as torch ops.

// torch.clamp(x, 0, 1) (NaN propagates) and its backward (the gradient passes where 0 <= x <= 1)
__global__ __launch_bounds__(256) void clamp01_kernel(const float *__restrict__ x, int64_t n, float *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    y[i] = v != v ? v : fminf(fmaxf(v, 0.f), 1.f);
}
__global__ __launch_bounds__(256) void clamp01_bwd_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                          int64_t n, float *__restrict__ d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    d[i] = (v >= 0.f && v <= 1.f) ? g[i] : 0.f;
}
// out (3, npix) = a (3, npix) * mask (npix): image * alpha_mask, and its backward on the gradient
__global__ __launch_bounds__(256) void mul_mask_kernel(const float *__restrict__ a, const float *__restrict__ mask,
                                                       int64_t npix, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * npix) return;
    out[i] = a[i] * mask[i % npix];
}

enum Slot {
    kGeom, kBinning, kImage, kBwdScratch,                           // rasterizer buffers
    kRi, kPi, kNi, kWeights, kKids, kCutScratch,                    // the cut
    kMeans, kScales, kRots, kOpac, kShs, kRadii,                    // the blended rows
    kDMeans2D, kDMeans3D, kDScales, kDRots, kDOpac, kDShs,          // their gradients
    kColor, kExposed, kMasked, kGradMap, kDImg, kDExposed, kDColor, // image-sized
    kLossScratch, kExpScratch, kWords,                              // small
    kStamp, kLive,                                                  // the row state
    kSlots
};

}  // namespace
}  // namespace gsr

using namespace gsr;

struct gsr_post_ctx {
    struct Buf {
        void *p = nullptr;
        size_t cap = 0;
    } buf[kSlots];
    hipStream_t stream = nullptr;
    bool failed_alloc = false;
    bool one_written = false;
    int64_t growths = 0;
    // stream-ordered growth from the context's own pool, as gsr_train_ctx
    bool pool_ready = false;
    hipMemPool_t pool = nullptr;
    int64_t rows = -1;  // the N stamp / live were made for
    int cur = 0;        // the last stamp value

    void pool_setup() {
        if (pool_ready) return;
        pool_ready = true;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return;
        hipMemPoolProps props;
        std::memset(&props, 0, sizeof(props));
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        if (hipMemPoolCreate(&pool, &props) != hipSuccess) {
            pool = nullptr;
            (void)hipGetLastError();
            return;
        }
        uint64_t keep = UINT64_MAX;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
    // grow-only; slack: 1/4 more than asked (the buffers that follow the cut and K), or exact
    void *get(int slot, size_t bytes, bool slack = true) {
        Buf &b = buf[slot];
        if (bytes <= b.cap && b.p) return b.p;
        growths++;
        const size_t want = std::max<size_t>(256, slack ? bytes + bytes / 4 : bytes);
        pool_setup();
        if (b.p) (void)hipFreeAsync(b.p, stream);
        b.p = nullptr;
        b.cap = 0;
        const hipError_t e = pool ? hipMallocFromPoolAsync(&b.p, want, pool, stream) : hipMallocAsync(&b.p, want, stream);
        if (e != hipSuccess) {
            b.p = nullptr;
            failed_alloc = true;
            return nullptr;
        }
        b.cap = want;
        return b.p;
    }
    int64_t held() const {
        int64_t n = 0;
        for (const auto &b : buf) n += (int64_t)b.cap;
        return n;
    }
    float *f32(int slot, size_t n) { return static_cast<float *>(get(slot, n * sizeof(float))); }
    int *i32(int slot, size_t n) { return static_cast<int *>(get(slot, n * sizeof(int))); }

    ~gsr_post_ctx() {
        for (auto &b : buf)
            if (b.p) (void)hipFreeAsync(b.p, stream);
        (void)hipStreamSynchronize(stream);
        if (pool) (void)hipMemPoolDestroy(pool);
    }
};

namespace {

void *post_resize_geom(void *c, size_t n) { return static_cast<gsr_post_ctx *>(c)->get(kGeom, n); }
void *post_resize_binning(void *c, size_t n) { return static_cast<gsr_post_ctx *>(c)->get(kBinning, n); }
void *post_resize_image(void *c, size_t n) { return static_cast<gsr_post_ctx *>(c)->get(kImage, n); }
void *post_resize_scratch(void *c, size_t n) { return static_cast<gsr_post_ctx *>(c)->get(kBwdScratch, n); }

int post_fail(int rc, const char *what) {
    if (rc == GSR_OK) return rc;
    set_last_error(std::string("gsr_post_step: ") + what + ": " + gsr_last_error());
    return rc;
}

int post_invalid(const char *msg) {
    set_last_error(std::string("gsr_post_step: ") + msg);
    return GSR_ERR_INVALID_ARGUMENT;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

int gsr_post_live_build(int n_groups, const gsr_adam_group *groups, int64_t N, uint8_t *live, void *stream) {
    PostAdamArgs pa;
    const int rc = post_runs(n_groups, groups, N, pa, "gsr_post_live_build");
    if (rc) return rc;
    if (N == 0) return GSR_OK;
    if (!live) {
        set_last_error("gsr_post_live_build: NULL live");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(post_live_kernel, dim3(blocks_of(N)), dim3(256), 0, static_cast<hipStream_t>(stream), pa, N,
                       live);
    return launched("gsr_post_live_build");
}

int gsr_post_adam_step(int n_groups, const gsr_adam_group *groups, int64_t N, const int *stamp, int cur,
                       uint8_t *live, int64_t tail, const uint8_t *lock, double beta1, double beta2, double eps,
                       void *stream) {
    PostAdamArgs pa;
    const int rc = post_runs(n_groups, groups, N, pa, "gsr_post_adam_step");
    if (rc) return rc;
    if (tail < 0 || tail > N) {
        set_last_error("gsr_post_adam_step: tail outside [0, N]");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (N == 0 || pa.n == 0) return GSR_OK;
    if (!stamp || !live) {
        set_last_error("gsr_post_adam_step: NULL stamp or live");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    // torch applies python-float hyper-parameters as fp32 scalars (optim.hip sparse_adam)
    const float b1 = (float)beta1, b2 = (float)beta2, e = (float)eps;
    const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
    hipLaunchKernelGGL(post_adam_kernel, dim3((unsigned)((N + kPostThreads - 1) / kPostThreads), (unsigned)pa.n),
                       dim3(kPostThreads), 0, static_cast<hipStream_t>(stream), pa, N, stamp, cur, live, tail, lock, b1,
                       b2, omb1, omb2, e);
    return launched("gsr_post_adam_step");
}

gsr_post_ctx *gsr_post_ctx_create(void) { return new (std::nothrow) gsr_post_ctx(); }

void gsr_post_ctx_destroy(gsr_post_ctx *ctx) {
    if (!ctx) return;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
}

int gsr_post_ctx_stats(const gsr_post_ctx *ctx, int64_t *out, int n) {
    if (!ctx || !out || n < 0) return post_invalid("NULL context or stats buffer");
    const int64_t v[3] = {ctx->growths, ctx->held(), 1};
    int k = 0;
    for (; k < n && k < 3; k++) out[k] = v[k];
    return k;
}

int gsr_post_ctx_read_rows(gsr_post_ctx *ctx, int what, void *dst, int64_t n, int *cur) {
    if (!ctx || (what != 0 && what != 1) || n < 0 || (n > 0 && !dst)) return post_invalid("read_rows: bad arguments");
    if (cur) *cur = ctx->cur;
    if (n == 0) return GSR_OK;
    if (ctx->rows < n || !ctx->buf[kStamp].p || !ctx->buf[kLive].p)
        return post_invalid("read_rows: the context has not stepped over that many rows");
    const void *src = what == 0 ? ctx->buf[kLive].p : ctx->buf[kStamp].p;
    const size_t bytes = (size_t)n * (what == 0 ? 1 : sizeof(int));
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
        set_last_error("gsr_post_ctx_read_rows: copy failed");
        return GSR_ERR_DEVICE;
    }
    return GSR_OK;
}

int gsr_post_step(gsr_post_ctx *ctx, const gsr_post_step_args *a, int64_t *cut_rows, int64_t *num_rendered) {
    if (cut_rows) *cut_rows = 0;
    if (num_rendered) *num_rendered = 0;
    if (!ctx || !a) return post_invalid("NULL context or arguments");
    const int64_t N = a->N, S = a->skybox;
    const int W = a->width, H = a->height, M = a->M;
    if (N <= 0 || N > 0x7fffffff || a->n_nodes <= 0 || S < 0 || S > N || W <= 0 || H <= 0 || M <= 0 || M > 16 ||
        a->D < 0 || (a->D + 1) * (a->D + 1) > M)
        return post_invalid("bad sizes");
    if (!a->nodes || !a->boxes) return post_invalid("NULL hierarchy");
    if (!a->xyz || !a->features || !a->opacity || !a->scaling || !a->rotation || !a->xyz_grad || !a->features_grad ||
        !a->opacity_grad || !a->scaling_grad || !a->rotation_grad)
        return post_invalid("NULL parameter or gradient");
    if (a->n_groups <= 0 || !a->groups) return post_invalid("no optimizer groups");
    if (!a->viewmatrix || !a->projmatrix || !a->campos || !a->background || !a->gt || !a->losses)
        return post_invalid("NULL camera, background, target or loss output");
    if (!(a->lambda_dssim >= 0.0 && a->lambda_dssim <= 1.0)) return post_invalid("lambda_dssim outside [0, 1]");
    PostAdamArgs pa;  // the groups checked before anything is launched
    int rc = post_runs(a->n_groups, a->groups, N, pa, "gsr_post_step");
    if (rc) return rc;

    hipStream_t s = static_cast<hipStream_t>(a->stream);
    if (ctx->stream != s) {  // the buffers are freed in the order of ctx->stream only (gsr_train_step)
        if (ctx->stream && hipStreamSynchronize(ctx->stream) != hipSuccess)
            return post_fail(GSR_ERR_DEVICE, "previous stream");
        ctx->stream = s;
    }
    void *sv = a->stream;
    const int64_t npix = (int64_t)W * H;

    // the row state: made for N rows, zero stamps (0 = never stamped; the values start at 1)
    bool rebuild = a->rebuild_live != 0;
    if (ctx->rows != N || ctx->cur == 0x7fffffff) {
        int *st = static_cast<int *>(ctx->get(kStamp, sizeof(int) * (size_t)N, false));
        if (!st || !ctx->get(kLive, (size_t)N, false) || hipMemsetAsync(st, 0, sizeof(int) * (size_t)N, s) != hipSuccess) {
            ctx->failed_alloc = false;
            ctx->rows = -1;
            set_last_error("gsr_post_step: device allocation failed");
            return GSR_ERR_ALLOCATION;
        }
        rebuild = rebuild || ctx->rows != N;
        ctx->rows = N;
        ctx->cur = 0;
    }
    int *stamp = static_cast<int *>(ctx->buf[kStamp].p);
    uint8_t *live = static_cast<uint8_t *>(ctx->buf[kLive].p);
    if (rebuild && (rc = gsr_post_live_build(a->n_groups, a->groups, N, live, sv))) return post_fail(rc, "live rows");

    // 1-2: the cut (train_post.py:91-113); one entry per Gaussian, as the Python step's buffers
    int *ri = ctx->i32(kRi, N), *pi = ctx->i32(kPi, N), *ni = ctx->i32(kNi, N), *kids = ctx->i32(kKids, N);
    float *wts = ctx->f32(kWeights, N);
    const size_t cut_bytes = gsr_expand_to_size_scratch_bytes(a->n_nodes);
    void *cut_scratch = ctx->get(kCutScratch, cut_bytes);
    void *words = ctx->get(kWords, 64);
    if (ctx->failed_alloc || !ri || !pi || !ni || !kids || !wts || !cut_scratch || !words) {
        ctx->failed_alloc = false;
        set_last_error("gsr_post_step: device allocation failed");
        return GSR_ERR_ALLOCATION;
    }
    if (!ctx->one_written) {  // dL/dloss = 1, once per context (the slot is never re-allocated)
        const uint32_t w1[4] = {0x3f800000u, 0u, 0u, 0u};
        if (hipMemcpyAsync(words, w1, sizeof(w1), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return post_fail(GSR_ERR_DEVICE, "step words");
        ctx->one_written = true;
    }
    const float *one = static_cast<const float *>(words);
    int64_t R = 0;
    rc = gsr_expand_to_size(a->n_nodes, a->nodes, a->boxes, a->limit, a->campos, ri, pi, ni, N, cut_scratch, cut_bytes,
                            &R, sv);
    if (rc) return post_fail(rc, "expand_to_size");
    if (cut_rows) *cut_rows = R;
    const int64_t rows = R + S;
    if (rows <= 0 || rows > 0x7fffffff) return post_invalid("empty cut");
    rc = gsr_interpolation_weights(R, ni, a->limit, a->nodes, a->boxes, a->campos_host[0], a->campos_host[1],
                                   a->campos_host[2], wts, kids, sv);
    if (rc) return post_fail(rc, "interpolation weights");

    float *means = ctx->f32(kMeans, 3 * rows), *scales = ctx->f32(kScales, 3 * rows), *rots = ctx->f32(kRots, 4 * rows);
    float *opac = ctx->f32(kOpac, rows), *shs = ctx->f32(kShs, (size_t)3 * M * rows);
    int *radii = ctx->i32(kRadii, rows);
    float *d_means2D = ctx->f32(kDMeans2D, 3 * rows), *d_means3D = ctx->f32(kDMeans3D, 3 * rows);
    float *d_scales = ctx->f32(kDScales, 3 * rows), *d_rots = ctx->f32(kDRots, 4 * rows);
    float *d_opac = ctx->f32(kDOpac, rows), *d_shs = ctx->f32(kDShs, (size_t)3 * M * rows);
    float *color = ctx->f32(kColor, 3 * npix), *exposed = ctx->f32(kExposed, 3 * npix);
    float *masked = a->alpha_mask ? ctx->f32(kMasked, 3 * npix) : exposed;
    float *gmap = ctx->f32(kGradMap, 3 * npix), *d_img = ctx->f32(kDImg, 3 * npix);
    float *d_exposed = a->alpha_mask ? ctx->f32(kDExposed, 3 * npix) : d_img;
    float *d_color = ctx->f32(kDColor, 3 * npix);
    void *loss_scratch = ctx->get(kLossScratch, std::max<size_t>(1, gsr_l1_ssim_scratch_bytes(3, H, W)));
    // the exposure backward's scratch, then the 12 floats of the exposure gradient nobody reads
    const size_t exp_bytes = (gsr_exposure_scratch_bytes(npix) + 15) / 16 * 16;
    void *exp_scratch = ctx->get(kExpScratch, exp_bytes + 64);
    if (ctx->failed_alloc || !means || !scales || !rots || !opac || !shs || !radii || !d_means2D || !d_means3D ||
        !d_scales || !d_rots || !d_opac || !d_shs || !color || !exposed || !masked || !gmap || !d_img || !d_exposed ||
        !d_color || !loss_scratch || !exp_scratch) {
        ctx->failed_alloc = false;
        set_last_error("gsr_post_step: device allocation failed");
        return GSR_ERR_ALLOCATION;
    }
    float *d_E = reinterpret_cast<float *>(static_cast<char *>(exp_scratch) + exp_bytes);

    // 3: render_post's blend over the raw parameters
    rc = gsr_interpolate_cut_forward_act(N, M, R, S, ri, pi, wts, a->xyz, a->scaling, a->rotation, a->opacity,
                                         a->features, GSR_OPACITY_ABS, means, scales, rots, opac, shs, sv);
    if (rc) return post_fail(rc, "cut forward");
    // 4: the rasterizer (no depth, no hierarchy fields: the rows are blended already)
    int64_t K = 0;
    rc = gsr_rasterize_forward_ex(post_resize_geom, post_resize_binning, post_resize_image, ctx, (int)rows, a->D, M,
                                  a->background, W, H, means, shs, nullptr, opac, scales, 1.0f, rots, nullptr,
                                  a->viewmatrix, a->projmatrix, a->campos, a->tan_fovx, a->tan_fovy, 0, color, nullptr,
                                  radii, nullptr, nullptr, nullptr, nullptr, 0, 0, sv, &K, 0u);
    if (rc) return post_fail(rc, "rasterizer forward");
    // 5-6: exposure + clamp (or the clamp alone), x alpha mask
    if (a->exposure) {
        if ((rc = gsr_exposure_forward(color, a->exposure, npix, exposed, sv))) return post_fail(rc, "exposure");
    } else {
        hipLaunchKernelGGL(clamp01_kernel, dim3(blocks_of(3 * npix)), dim3(256), 0, s, color, 3 * npix, exposed);
    }
    if (a->alpha_mask)
        hipLaunchKernelGGL(mul_mask_kernel, dim3(blocks_of(3 * npix)), dim3(256), 0, s, exposed, a->alpha_mask, npix,
                           masked);
    // 7: the photometric loss and its gradient for dL/dloss = 1
    rc = gsr_photo_loss_forward(masked, a->gt, 3, H, W, a->lambda_dssim, loss_scratch, a->losses, gmap, sv);
    if (rc) return post_fail(rc, "photo loss");
    rc = gsr_photo_loss_backward(masked, a->gt, gmap, 3, H, W, a->lambda_dssim, one, d_img, sv);
    if (rc) return post_fail(rc, "photo loss backward");
    // 8: back through the mask and the exposure (or the clamp)
    if (a->alpha_mask)
        hipLaunchKernelGGL(mul_mask_kernel, dim3(blocks_of(3 * npix)), dim3(256), 0, s, d_img, a->alpha_mask, npix,
                           d_exposed);
    if (a->exposure) {
        rc = gsr_exposure_backward(color, a->exposure, npix, d_exposed, d_color, d_E, exp_scratch, sv);
        if (rc) return post_fail(rc, "exposure backward");
    } else {
        hipLaunchKernelGGL(clamp01_bwd_kernel, dim3(blocks_of(3 * npix)), dim3(256), 0, s, color, d_exposed, 3 * npix,
                           d_color);
    }
    // 9: the rasterizer backward; every row of the R + S gradients is written (the blend reads them all)
    rc = gsr_rasterize_backward(post_resize_scratch, ctx, (int)rows, a->D, M, K, a->background, W, H, means, shs,
                                nullptr, scales, 1.0f, rots, nullptr, a->viewmatrix, a->projmatrix, a->campos,
                                a->tan_fovx, a->tan_fovy, radii, ctx->buf[kGeom].p, ctx->buf[kBinning].p,
                                ctx->buf[kImage].p, d_color, nullptr, d_means2D, nullptr, d_opac, d_means3D, nullptr,
                                d_shs, d_scales, d_rots, nullptr, nullptr, nullptr, nullptr, 0, 0, sv);
    if (rc) return post_fail(rc, "rasterizer backward");
    // 10: the blend's backward into the persistent (zero) N-row gradients
    rc = gsr_interpolate_cut_backward_act(N, M, R, S, ri, pi, wts, a->scaling, a->rotation, a->opacity,
                                          GSR_OPACITY_ABS | GSR_CUT_UNIQUE_CHILDREN, d_means3D, d_scales, d_rots,
                                          d_opac, d_shs, a->xyz_grad, a->scaling_grad, a->rotation_grad,
                                          a->opacity_grad, a->features_grad, sv);
    if (rc) return post_fail(rc, "cut backward");
    // 11-12: the rows it touched, then locks + Adam + the gradients' clear in one launch
    const int cur = ++ctx->cur;
    if ((rc = gsr_cut_mark_rows(N, R, S, ri, pi, wts, stamp, cur, sv))) return post_fail(rc, "mark");
    rc = gsr_post_adam_step(a->n_groups, a->groups, N, stamp, cur, live, S, a->lock, a->beta1, a->beta2, a->eps, sv);
    if (rc) return post_fail(rc, "Adam");
    if ((rc = launched("gsr_post_step"))) return rc;
    if (num_rendered) *num_rendered = K;
    return GSR_OK;
}

}  // extern "C"
