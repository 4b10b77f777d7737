// eval.hip -- the evaluation metrics of one rendered frame (include/gsr_eval.h): PSNR, SSIM, iMAE and
// iRMSE for the whole image and for up to 16 regions (depth ranges, segmentation categories) in one
// pass over the frame.
//
// The reference (render_hierarchy_final.py:259-390) runs one five-convolution ssim for the whole
// image and one seven-convolution ssim_masked per region, each with full-size temporaries, boolean
// indexed assignments and `.sum() > 0` host syncs.  Here a workgroup owns a 64x16 output tile and
// stages the 74x26 halo of x = clamp(image) alpha and y = clamp(gt) alpha (three channels each) and
// of the region bits once in LDS.  The whole-image pass and then one pass per region run the
// separable window (gsr_ssim.h) over the staged halo; per region the mask weight is windowed once,
// with the first channel.  A region with no pixel in the tile contributes zeros and costs nothing.
// Every workgroup writes ten partial sums per row with plain stores; a second launch reduces them
// in a fixed order in fp64 and forms the metrics.  The frame is read from HBM once however many
// regions there are, and nothing is written per pixel.
#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/gsr.h"
#include "../../include/gsr_eval.h"
#include "gsr_launch.h"
#include "gsr_ssim.h"

namespace gsr {
namespace {

constexpr int kEvRH = kTH + 2 * kR, kEvRW = kTW + 2 * kR;  // 26 x 74 staged halo
constexpr int kEvIP = odd_pitch(kEvRW), kEvHP = odd_pitch(kTW);
constexpr int kEvIn = kEvRH * kEvIP, kEvHs = kEvRH * kEvHP;
constexpr int kEvBitsWords = (kEvIn + 1) / 2;  // the uint16 bits halo, in floats
constexpr int kEvQ = 10;  // partial sums per row, see Part
constexpr int kEvWaves = kLossThreads / 64;
// 6 image maps + bits + 6 horizontal maps (five moments and the mask weight) + reduction words: 89.3 KiB
constexpr size_t kEvLds = sizeof(float) * (6 * kEvIn + kEvBitsWords + 6 * kEvHs + kEvWaves * kEvQ + kEvWaves);

// Partial sums of one row of one tile (the same ten for the whole image, with m = 1).
enum Part { kSsim, kValid, kMask, kSe0, kSe1, kSe2, kDabs, kDsq, kAsum, kApos };

struct EvalArgs {
    const float *image, *gt, *alpha, *invd, *gt_invd;
    const uint16_t *bits;
    int n_regions, H, W;
};

// Horizontal pass of the five moments of x m and y m, and (kWeight) of m itself, over the staged
// halo: hpass5's tasks and order with the region's bit applied as the values are loaded.
template <int kS, bool kWeight>
__device__ __forceinline__ void hpass_masked(const float *sx, const float *sy, const uint16_t *sb, unsigned bit,
                                             const Window &win, float *hs) {
    constexpr int segs = (kTW + kS - 1) / kS;
    for (int task = threadIdx.x; task < kEvRH * segs; task += kLossThreads) {
        const int s = task / kEvRH, r = task - s * kEvRH, c0 = s * kS;
        const float *px = sx + r * kEvIP + c0, *py = sy + r * kEvIP + c0;
        const uint16_t *pb = sb + r * kEvIP + c0;
        float u[kS + 2 * kR], v[kS + 2 * kR];
        bool m[kS + 2 * kR];
#pragma unroll
        for (int k = 0; k < kS + 2 * kR; k++) {
            m[k] = c0 + k < kEvRW && (pb[k] & bit) != 0;
            u[k] = m[k] ? px[k] : 0.f;
            v[k] = m[k] ? py[k] : 0.f;
        }
#pragma unroll
        for (int o = 0; o < kS; o++) {
            float m1 = 0.f, m2 = 0.f, a11 = 0.f, a22 = 0.f, a12 = 0.f, mw = 0.f;
#pragma unroll
            for (int j = 0; j < 2 * kR + 1; j++) {
                const float w = win.w[j];
                m1 = fmaf(w, u[o + j], m1);
                m2 = fmaf(w, v[o + j], m2);
                a11 = fmaf(w, u[o + j] * u[o + j], a11);
                a22 = fmaf(w, v[o + j] * v[o + j], a22);
                a12 = fmaf(w, u[o + j] * v[o + j], a12);
                if (kWeight) mw = fmaf(w, m[o + j] ? 1.f : 0.f, mw);
            }
            if (c0 + o < kTW) {
                const int i = r * kEvHP + c0 + o;
                hs[i] = m1;
                hs[kEvHs + i] = m2;
                hs[2 * kEvHs + i] = a11;
                hs[3 * kEvHs + i] = a22;
                hs[4 * kEvHs + i] = a12;
                if (kWeight) hs[5 * kEvHs + i] = mw;
            }
        }
    }
}

// The tile's ten sums to partials[(row * kEvQ + q) * nb + b]: the waves' sums through LDS, added in
// wave order by one thread per quantity.
__device__ __forceinline__ void write_partials(float (&v)[kEvQ], float *red, float *__restrict__ partials, int row,
                                               int nb, int b) {
    wave_allreduce<kEvQ>(v);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < kEvQ; q++) red[wv * kEvQ + q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < kEvQ) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kEvWaves; k++) s += red[k * kEvQ + threadIdx.x];
        partials[((size_t)row * kEvQ + threadIdx.x) * nb + b] = s;
    }
}

// One channel of one region: the masked moments of the staged halo, then this thread's four pixels.
template <bool kFirst>
__device__ __forceinline__ void region_channel(const float *sx, const float *sy, const uint16_t *sb, unsigned bit,
                                               const Window &win, float *hs, const unsigned (&pbits)[4],
                                               float (&wacc)[4], float &ss, float &se, float &valid) {
    hpass_masked<8, kFirst>(sx, sy, sb, bit, win, hs);
    __syncthreads();
    float acc[kFirst ? 6 : 5][4];
    vpass_tile<kFirst ? 6 : 5>(hs, kEvHP, kEvHs, win, acc);
    const int c = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 4;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (kFirst) wacc[k] = acc[kFirst ? 5 : 0][k];
        if (!(pbits[k] & bit)) continue;  // the map is multiplied by m
        const int li = (r0 + k + kR) * kEvIP + c + kR;
        const float d = sx[li] - sy[li];
        se += d * d;
        const float w = wacc[k];
        if (!(w > 1e-6f)) continue;  // valid_windows (utils/loss_utils.py:110)
        if (kFirst) valid += 1.f;
        const Moments mo{acc[0][k] / w, acc[1][k] / w, acc[2][k] / w, acc[3][k] / w, acc[4][k] / w};
        float num, den;
        ssim_terms(mo, num, den);
        if (den > 1e-10f) ss += num / den;  // valid_ssim (:144)
    }
    __syncthreads();  // hs is rewritten by the next pass
}

__global__ __launch_bounds__(kLossThreads) void eval_frame_kernel(EvalArgs a, Window win,
                                                                  float *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sxy = reinterpret_cast<float *>(smem);  // x0 x1 x2 y0 y1 y2
    uint16_t *sb = reinterpret_cast<uint16_t *>(sxy + 6 * kEvIn);
    float *hs = sxy + 6 * kEvIn + kEvBitsWords;
    float *red = hs + 6 * kEvHs;
    unsigned *s_or = reinterpret_cast<unsigned *>(red + kEvWaves * kEvQ);
    const int H = a.H, W = a.W;
    const size_t HW = (size_t)H * W;
    const int ox = blockIdx.x * kTW, oy = blockIdx.y * kTH;
    const int nb = gridDim.x * gridDim.y, b = blockIdx.y * gridDim.x + blockIdx.x;

    // stage the halo: x = clamp(image) alpha, y = clamp(gt) alpha, zero outside the image
    for (int i = threadIdx.x; i < kEvRH * kEvRW; i += kLossThreads) {
        const int r = i / kEvRW, c = i - r * kEvRW;
        const int gy = oy - kR + r, gx = ox - kR + c;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t o = in ? (size_t)gy * W + gx : 0;
        const float al = a.alpha ? a.alpha[o] : 1.f;
        const int li = r * kEvIP + c;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float xv = fminf(fmaxf(a.image[ch * HW + o], 0.f), 1.f) * al;
            const float yv = fminf(fmaxf(a.gt[ch * HW + o], 0.f), 1.f) * al;
            sxy[ch * kEvIn + li] = in ? xv : 0.f;
            sxy[(3 + ch) * kEvIn + li] = in ? yv : 0.f;
        }
        sb[li] = in && a.bits ? a.bits[o] : (uint16_t)0;
    }

    // this thread's four pixels: column c, rows r0 .. r0 + 3 of the tile
    const int c = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 4;
    bool inb[4];
    float al[4], dd[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int gy = oy + r0 + k, gx = ox + c;
        inb[k] = gy < H && gx < W;
        const size_t o = inb[k] ? (size_t)gy * W + gx : 0;
        al[k] = a.alpha ? a.alpha[o] : 1.f;
        dd[k] = a.invd ? a.invd[o] - a.gt_invd[o] : 0.f;
    }
    __syncthreads();
    unsigned pbits[4], ob = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        pbits[k] = sb[(r0 + k + kR) * kEvIP + c + kR];  // zero outside the image
        ob |= pbits[k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ob |= __shfl_xor(ob, off);
    if ((threadIdx.x & 63) == 0) s_or[threadIdx.x >> 6] = ob;

    // row 0: the whole image
    {
        float v[kEvQ] = {};
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float *sx = sxy + ch * kEvIn, *sy = sxy + (3 + ch) * kEvIn;
            hpass5<8>(sx, sy, kEvRH, kEvRW, kEvIP, kTW, kEvHP, kEvHs, win, hs);
            __syncthreads();
            float acc[5][4];
            vpass_tile<5>(hs, kEvHP, kEvHs, win, acc);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!inb[k]) continue;
                v[kSsim] += ssim_value(Moments{acc[0][k], acc[1][k], acc[2][k], acc[3][k], acc[4][k]});
                const int li = (r0 + k + kR) * kEvIP + c + kR;
                const float d = sx[li] - sy[li];
                v[kSe0 + ch] += d * d;
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!inb[k]) continue;
            v[kValid] += 1.f;
            v[kMask] += 1.f;
            v[kDabs] += fabsf(dd[k]) * al[k];
            v[kDsq] += dd[k] * dd[k] * al[k];
            v[kAsum] += al[k];
            v[kApos] += al[k] > 0.f ? 1.f : 0.f;
        }
        write_partials(v, red, partials, 0, nb, b);
    }
    unsigned tile_bits = 0;  // s_or was written before the passes' barriers
#pragma unroll
    for (int k = 0; k < kEvWaves; k++) tile_bits |= s_or[k];

    for (int rg = 0; rg < a.n_regions; rg++) {
        const unsigned bit = 1u << rg;
        if (!(tile_bits & bit)) {  // uniform: no pixel of the region in this tile
            if (threadIdx.x < kEvQ) partials[((size_t)(1 + rg) * kEvQ + threadIdx.x) * nb + b] = 0.f;
            continue;
        }
        float v[kEvQ] = {};
        float wacc[4];
        region_channel<true>(sxy, sxy + 3 * kEvIn, sb, bit, win, hs, pbits, wacc, v[kSsim], v[kSe0], v[kValid]);
        region_channel<false>(sxy + kEvIn, sxy + 4 * kEvIn, sb, bit, win, hs, pbits, wacc, v[kSsim], v[kSe1],
                              v[kValid]);
        region_channel<false>(sxy + 2 * kEvIn, sxy + 5 * kEvIn, sb, bit, win, hs, pbits, wacc, v[kSsim], v[kSe2],
                              v[kValid]);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!(pbits[k] & bit)) continue;
            v[kMask] += 1.f;
            v[kDabs] += fabsf(dd[k]) * al[k];
            v[kDsq] += dd[k] * dd[k] * al[k];
            v[kAsum] += al[k];
            v[kApos] += al[k] > 0.f ? 1.f : 0.f;
        }
        write_partials(v, red, partials, 1 + rg, nb, b);
    }
}

// One workgroup per row: the tiles' partial sums in a fixed order in fp64, then the metrics.
__global__ __launch_bounds__(256) void eval_finalize_kernel(const float *__restrict__ partials, int nb, int H, int W,
                                                            int has_depth, double *__restrict__ frame) {
    __shared__ double sh[256];
    const int row = blockIdx.x;
    double t[kEvQ];
    for (int q = 0; q < kEvQ; q++) {
        const float *p = partials + ((size_t)row * kEvQ + q) * nb;
        double s = 0.0;
        for (int i = threadIdx.x; i < nb; i += 256) s += (double)p[i];
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
            __syncthreads();
        }
        t[q] = sh[0];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double *out = frame + (size_t)row * GSR_EVAL_FRAME_COLS;
    const double n = row == 0 ? (double)H * W : t[kMask];
    if (!(n > 0.0)) {  // an empty region: not evaluated
        for (int k = 0; k < GSR_EVAL_FRAME_COLS; k++) out[k] = 0.0;
        return;
    }
    double psnr = 0.0;
    for (int ch = 0; ch < 3; ch++) psnr += 20.0 * log10(1.0 / sqrt(t[kSe0 + ch] / n));
    out[0] = psnr / 3.0;
    out[1] = row == 0 ? t[kSsim] / (3.0 * n) : t[kSsim] / fmax(3.0 * t[kValid], 1.0);
    const bool depth = has_depth && t[kAsum] > 0.0;
    out[2] = depth ? t[kDabs] / t[kAsum] : 0.0;
    out[3] = depth ? sqrt(t[kDsq] / t[kAsum]) : 0.0;
    out[4] = row == 0 ? n : t[kApos];
    out[5] = 1.0;
    out[6] = n;
    out[7] = t[kValid];
}

__global__ __launch_bounds__(64) void eval_accumulate_kernel(const double *__restrict__ frame, int n_rows,
                                                             double *__restrict__ totals) {
    const int row = threadIdx.x;
    if (row >= n_rows) return;
    const double *f = frame + (size_t)row * GSR_EVAL_FRAME_COLS;
    const double w = f[4];
    if (f[5] == 0.0 || w == 0.0) return;
    double *t = totals + (size_t)row * GSR_EVAL_TOTAL_COLS;
    for (int k = 0; k < 4; k++) t[k] += w * f[k];
    t[4] += w;
    t[5] += 1.0;
}

struct Ranges {
    float lo[GSR_EVAL_MAX_REGIONS], hi[GSR_EVAL_MAX_REGIONS];
};

__global__ __launch_bounds__(256) void depth_range_bits_kernel(const float *__restrict__ gt_invd, int64_t n,
                                                               int n_ranges, Ranges rg, int shift,
                                                               uint16_t *__restrict__ bits) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = 1.0f / (gt_invd[i] + 1e-6f);  // render_hierarchy_final.py:132-136
        unsigned m = 0;
        for (int k = 0; k < n_ranges; k++)
            if (d >= rg.lo[k] && d < rg.hi[k]) m |= 1u << (shift + k);
        bits[i] = (uint16_t)(bits[i] | m);
    }
}

struct Colors {
    uint8_t c[3 * GSR_EVAL_MAX_REGIONS];
};

__global__ __launch_bounds__(256) void color_bits_kernel(const uint8_t *__restrict__ seg, int64_t n, int n_colors,
                                                         Colors col, int shift, uint16_t *__restrict__ bits) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t r = seg[i], g = seg[n + i], b = seg[2 * n + i];
        unsigned m = 0;
        for (int k = 0; k < n_colors; k++)
            if (r == col.c[3 * k] && g == col.c[3 * k + 1] && b == col.c[3 * k + 2]) m |= 1u << (shift + k);
        bits[i] = (uint16_t)(bits[i] | m);
    }
}

dim3 eval_grid(int H, int W) { return dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH); }

unsigned stride_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 4096); }

bool bad_bits(int n, int shift) { return n < 0 || shift < 0 || shift + n > GSR_EVAL_MAX_REGIONS; }

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_eval_depth_range_bits(const float *gt_invdepth, int64_t n, int n_ranges, const float *lo, const float *hi,
                              int shift, uint16_t *bits, void *stream) {
    if (n < 0 || bad_bits(n_ranges, shift) || (n > 0 && (!gt_invdepth || !bits)) || (n_ranges > 0 && (!lo || !hi))) {
        set_last_error("gsr_eval_depth_range_bits: NULL pointer, n < 0 or shift + n_ranges outside 0..16");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (n == 0 || n_ranges == 0) return GSR_OK;
    Ranges rg{};
    for (int k = 0; k < n_ranges; k++) {
        rg.lo[k] = lo[k];
        rg.hi[k] = hi[k];
    }
    hipLaunchKernelGGL(depth_range_bits_kernel, dim3(stride_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       gt_invdepth, n, n_ranges, rg, shift, bits);
    return launched("gsr_eval_depth_range_bits");
}

int gsr_eval_color_bits(const uint8_t *seg_rgb_u8, int64_t n, int n_colors, const uint8_t *colors, int shift,
                        uint16_t *bits, void *stream) {
    if (n < 0 || bad_bits(n_colors, shift) || (n > 0 && (!seg_rgb_u8 || !bits)) || (n_colors > 0 && !colors)) {
        set_last_error("gsr_eval_color_bits: NULL pointer, n < 0 or shift + n_colors outside 0..16");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (n == 0 || n_colors == 0) return GSR_OK;
    Colors col{};
    for (int k = 0; k < 3 * n_colors; k++) col.c[k] = colors[k];
    hipLaunchKernelGGL(color_bits_kernel, dim3(stride_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       seg_rgb_u8, n, n_colors, col, shift, bits);
    return launched("gsr_eval_color_bits");
}

size_t gsr_eval_frame_scratch_bytes(int H, int W, int n_regions) {
    if (H <= 0 || W <= 0 || n_regions < 0 || n_regions > GSR_EVAL_MAX_REGIONS) return 0;
    const dim3 g = eval_grid(H, W);
    return sizeof(float) * kEvQ * (size_t)(1 + n_regions) * g.x * g.y;
}

int gsr_eval_frame(const float *image, const float *gt, const float *alpha_mask, const float *invdepth,
                   const float *gt_invdepth, const uint16_t *region_bits, int n_regions, int H, int W,
                   void *scratch, double *frame, void *stream) {
    if (H <= 0 || W <= 0 || !image || !gt || !scratch || !frame) {
        set_last_error("gsr_eval_frame: empty image or NULL pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (n_regions < 0 || n_regions > GSR_EVAL_MAX_REGIONS || (n_regions > 0 && !region_bits)) {
        set_last_error("gsr_eval_frame: n_regions outside 0..16, or regions without region_bits");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if ((invdepth == nullptr) != (gt_invdepth == nullptr)) {
        set_last_error("gsr_eval_frame: invdepth and gt_invdepth go together (both or neither)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    static const hipError_t attr = hipFuncSetAttribute((const void *)eval_frame_kernel,
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEvLds);
    if (attr != hipSuccess) {
        set_last_error(std::string("gsr_eval_frame: ") + hipGetErrorString(attr));
        return GSR_ERR_DEVICE;
    }
    const dim3 g = eval_grid(H, W);
    const EvalArgs a{image, gt, alpha_mask, invdepth, gt_invdepth, n_regions > 0 ? region_bits : nullptr,
                     n_regions, H, W};
    float *part = static_cast<float *>(scratch);
    hipLaunchKernelGGL(eval_frame_kernel, g, dim3(kLossThreads), kEvLds, s, a, ssim_window(), part);
    hipLaunchKernelGGL(eval_finalize_kernel, dim3(1 + n_regions), dim3(256), 0, s, part, (int)(g.x * g.y), H, W,
                       invdepth ? 1 : 0, frame);
    return launched("gsr_eval_frame");
}

int gsr_eval_accumulate(const double *frame, int n_rows, double *totals, void *stream) {
    if (!frame || !totals || n_rows < 1 || n_rows > 1 + GSR_EVAL_MAX_REGIONS) {
        set_last_error("gsr_eval_accumulate: NULL pointer or n_rows outside 1..17");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), frame, n_rows,
                       totals);
    return launched("gsr_eval_accumulate");
}

}  // extern "C"
