// lpips.hip -- the LPIPS metric around a caller-run VGG16 trunk (include/gsr_lpips.h): the batch the
// trunk reads, the per-stage tap for the whole image and up to 16 regions, and the running sums.
//
// The reference (lpipsPyTorch/modules/lpips.py:32-66) runs the trunk on both images once per row of
// the results table, writes five pairs of channel-normalised feature maps and their squared
// difference at full size, and only then applies the region's mask.  Here the trunk runs once per
// frame on a batch of two, and lpips_tap_kernel reads each stage's pre-ReLU output once from HBM.
//
// A workgroup owns 64 quads of 2x2 feature pixels, one per lane, and its 4, 8 or 16 waves share the
// channels: deep stages have few pixels and many channels, and pixels alone would leave most of the
// chip idle there.  Each wave applies the ReLU as it loads, sums the squares of its channels and
// writes the quads' maxima (the next stage's input); the waves' sums meet in LDS and give the two
// norms; a second pass over the same channels forms the wave's share of
// d = sum_c w_c (x_c / (|x| + eps) - y_c / (|y| + eps))^2 -- from registers when a wave's channels
// fit there (eight per wave: the 64- and 128-channel stages, 79% of the bytes), else from a re-read
// of addresses the workgroup has just read.  This two-pass form is the accurate one: the one-pass
// expansion into five sums cancels when the two images agree.  The terms are fp32 (the reference's
// operations in its order); they are added over the channels and within the workgroup in fp64, so
// the error does not grow with the channel count.  Waves 0..3 then hold one pixel of every quad each
// and reduce d's sum and each region's masked sum and pixel count; every workgroup leaves them as
// plain fp32 stores and lpips_finalize_kernel adds them in a fixed order in fp64.  Nothing is
// written per pixel except the pooled features.
#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/gsr.h"
#include "../../include/gsr_lpips.h"
#include "gsr_launch.h"

namespace gsr {
namespace {

constexpr int kTapQuads = 64;      // quads per workgroup: one per lane
constexpr int kTapMaxWaves = 16;   // waves that share a workgroup's channels
constexpr int kTapHold = 8;        // channels a wave keeps in registers between the two passes
constexpr int kTapRows = 1 + GSR_LPIPS_MAX_REGIONS;

// dynamic LDS: the waves' partial sums [nw][8][64] fp64, the norms [8][64] fp32, the row sums
// [4][kTapRows][2] fp64
constexpr size_t tap_lds(int nw) {
    return sizeof(double) * nw * 8 * 64 + sizeof(float) * 8 * 64 + sizeof(double) * 4 * kTapRows * 2;
}

struct TapArgs {
    const float *feat, *lin;
    const uint16_t *bits;
    float *pooled;
    int C, h, w, n_regions, H, W;
};

// The two values at p[0], p[1] after the ReLU; kVec: one 8-byte load (w even, so both are in the row
// and the address is 8-byte aligned), else two guarded loads.
template <bool kVec>
__device__ __forceinline__ void load_pair(const float *p, bool v0, bool v1, float &a, float &b) {
    if (kVec) {
        const float2 t = v0 ? *reinterpret_cast<const float2 *>(p) : make_float2(0.f, 0.f);
        a = fmaxf(t.x, 0.f);
        b = fmaxf(t.y, 0.f);
    } else {
        a = v0 ? fmaxf(p[0], 0.f) : 0.f;
        b = v1 ? fmaxf(p[1], 0.f) : 0.f;
    }
}

// One channel of a quad in both images (zero outside the map): pixels (r0, c0), (r0, c0 + 1),
// (r0 + 1, c0), (r0 + 1, c0 + 1) at offsets o0, o0 + 1, o2, o2 + 1.
template <bool kVec>
__device__ __forceinline__ void load_quad(const float *fx, const float *fy, size_t o0, size_t o2, const bool (&v)[4],
                                          float (&x)[4], float (&y)[4]) {
    load_pair<kVec>(fx + o0, v[0], v[1], x[0], x[1]);
    load_pair<kVec>(fx + o2, v[2], v[3], x[2], x[3]);
    load_pair<kVec>(fy + o0, v[0], v[1], y[0], y[1]);
    load_pair<kVec>(fy + o2, v[2], v[3], y[2], y[3]);
}

// F.interpolate(mode='nearest'): the source index of output index i, in fp32
__device__ __forceinline__ int nearest_src(int i, float scale, int n) {
    return min((int)floorf((float)i * scale), n - 1);
}

// The wave's sum in every lane, in a fixed order.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// blockDim.x = 64 nw, nw in {4, 8, 16}.  kHold: C == nw * kTapHold, a wave keeps its channels.
template <bool kVec, bool kHold>
__global__ __launch_bounds__(64 * kTapMaxWaves) void lpips_tap_kernel(TapArgs a, float *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double *part = reinterpret_cast<double *>(smem);
    float *den = reinterpret_cast<float *>(part + nw * 8 * 64);
    double *red = reinterpret_cast<double *>(den + 8 * 64);

    const int h = a.h, w = a.w, C = a.C;
    const int qw = (w + 1) / 2, qh = (h + 1) / 2, ph = h / 2, pw = w / 2;
    const int64_t Q = (int64_t)qh * qw, q = (int64_t)blockIdx.x * kTapQuads + lane;
    const bool live = q < Q;
    const int i = live ? (int)(q / qw) : 0, j = live ? (int)(q - (int64_t)i * qw) : 0;
    const int r0 = 2 * i, c0 = 2 * j;
    const bool v[4] = {live, live && c0 + 1 < w, live && r0 + 1 < h, live && c0 + 1 < w && r0 + 1 < h};
    const size_t hw = (size_t)h * w, o0 = (size_t)r0 * w + c0, o2 = o0 + w;
    const float *fx = a.feat, *fy = a.feat + (size_t)C * hw;
    // this wave's channels
    const int cpw = kHold ? kTapHold : (C + nw - 1) / nw;
    const int cb = min(C, wv * cpw), ce = min(C, cb + cpw);

    const bool pool = a.pooled != nullptr && v[3];
    const size_t phw = (size_t)ph * pw, po = (size_t)i * pw + j;
    float *px = a.pooled, *py = a.pooled + (size_t)C * phw;
    float hx[kHold ? kTapHold : 1][4], hy[kHold ? kTapHold : 1][4];
    double sx[4] = {}, sy[4] = {};  // fp32 terms, added in fp64: no growth with the channel count
    if (kHold) {
#pragma unroll
        for (int u = 0; u < kTapHold; u++) load_quad<kVec>(fx + (cb + u) * hw, fy + (cb + u) * hw, o0, o2, v, hx[u], hy[u]);
#pragma unroll
        for (int u = 0; u < kTapHold; u++) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                sx[k] += (double)(hx[u][k] * hx[u][k]);
                sy[k] += (double)(hy[u][k] * hy[u][k]);
            }
            if (pool) {
                px[(cb + u) * phw + po] = fmaxf(fmaxf(hx[u][0], hx[u][1]), fmaxf(hx[u][2], hx[u][3]));
                py[(cb + u) * phw + po] = fmaxf(fmaxf(hy[u][0], hy[u][1]), fmaxf(hy[u][2], hy[u][3]));
            }
        }
    } else {
#pragma unroll 4
        for (int c = cb; c < ce; c++) {
            float x[4], y[4];
            load_quad<kVec>(fx + c * hw, fy + c * hw, o0, o2, v, x, y);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                sx[k] += (double)(x[k] * x[k]);
                sy[k] += (double)(y[k] * y[k]);
            }
            if (pool) {
                px[c * phw + po] = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
                py[c * phw + po] = fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3]));
            }
        }
    }

    // the norms: the waves' sums added in wave order
#pragma unroll
    for (int k = 0; k < 4; k++) {
        part[(wv * 8 + k) * 64 + lane] = sx[k];
        part[(wv * 8 + 4 + k) * 64 + lane] = sy[k];
    }
    __syncthreads();
    for (int k = wv; k < 8; k += nw) {
        double s = 0.0;
        for (int u = 0; u < nw; u++) s += part[(u * 8 + k) * 64 + lane];
        den[k * 64 + lane] = sqrtf((float)s) + 1e-10f;
    }
    __syncthreads();
    float dx[4], dy[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        dx[k] = den[k * 64 + lane];
        dy[k] = den[(4 + k) * 64 + lane];
    }

    double d[4] = {};
    if (kHold) {
#pragma unroll
        for (int u = 0; u < kTapHold; u++) {
            const float wc = a.lin[cb + u];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float t = hx[u][k] / dx[k] - hy[u][k] / dy[k];
                d[k] += (double)(wc * (t * t));
            }
        }
    } else {
#pragma unroll 4
        for (int c = cb; c < ce; c++) {
            float x[4], y[4];
            load_quad<kVec>(fx + c * hw, fy + c * hw, o0, o2, v, x, y);
            const float wc = a.lin[c];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float t = x[k] / dx[k] - y[k] / dy[k];
                d[k] += (double)(wc * (t * t));
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) part[(wv * 4 + k) * 64 + lane] = d[k];  // the norms' reads are behind a barrier
    __syncthreads();

    // wave k < 4 takes pixel k of every quad: d in wave order, the pixel's region bits, the row sums
    if (wv < 4) {
        double dt = 0.0;
        for (int u = 0; u < nw; u++) dt += part[(u * 4 + wv) * 64 + lane];
        const int rr = r0 + (wv >> 1), cc = c0 + (wv & 1);
        const bool valid = live && rr < h && cc < w;  // d is zero where it is not
        unsigned pb = 0, ob = 0;
        if (a.n_regions > 0) {
            const float sh = (float)a.H / (float)h, sw = (float)a.W / (float)w;
            if (valid) pb = a.bits[(size_t)nearest_src(rr, sh, a.H) * a.W + nearest_src(cc, sw, a.W)];
            ob = pb;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) ob |= __shfl_xor(ob, off);
            ob = __builtin_amdgcn_readfirstlane(ob);
        }
        double *rw = red + (size_t)wv * kTapRows * 2;
        const double t0 = wave_sum(dt);
        if (lane == 0) {
            rw[0] = t0;
            rw[1] = 0.0;  // row 0 divides by h w
        }
        for (int rg = 0; rg < a.n_regions; rg++) {
            const unsigned bit = 1u << rg;
            double t = 0.0, n = 0.0;
            if (ob & bit) {  // wave-uniform: a wave without a pixel of the region adds zeros
                const bool m = (pb & bit) != 0;
                t = wave_sum(m ? dt : 0.0);
                n = wave_sum(m ? 1.0 : 0.0);
            }
            if (lane == 0) {
                rw[2 * (1 + rg)] = t;
                rw[2 * (1 + rg) + 1] = n;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * (1 + a.n_regions)) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) s += red[(size_t)k * kTapRows * 2 + threadIdx.x];
        const int row = threadIdx.x >> 1, col = threadIdx.x & 1;
        partials[((size_t)row * 2 + col) * gridDim.x + blockIdx.x] = (float)s;
    }
}

// One workgroup per row: the workgroups' sums in a fixed order in fp64, then the row's mean.
__global__ __launch_bounds__(256) void lpips_finalize_kernel(const float *__restrict__ partials, int nb, int h, int w,
                                                             double *__restrict__ out) {
    __shared__ double sh[256];
    const int row = blockIdx.x;
    double t[2];
    for (int col = 0; col < 2; col++) {
        const float *p = partials + ((size_t)row * 2 + col) * nb;
        double s = 0.0;
        for (int k = threadIdx.x; k < nb; k += 256) s += (double)p[k];
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int n = 128; n > 0; n >>= 1) {
            if ((int)threadIdx.x < n) sh[threadIdx.x] += sh[threadIdx.x + n];
            __syncthreads();
        }
        t[col] = sh[0];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    out[row] = row == 0 ? t[0] / ((double)h * w) : t[0] / fmax(t[1], 1e-8);
}

__global__ __launch_bounds__(256) void lpips_prepare_kernel(const float *__restrict__ image,
                                                            const float *__restrict__ gt,
                                                            const float *__restrict__ alpha, int64_t n,
                                                            float *__restrict__ batch) {
    const float mean[3] = {-.030f, -.088f, -.188f}, sd[3] = {.458f, .448f, .450f};  // modules/networks.py:41-44
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const float al = alpha ? alpha[p] : 1.f;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float x = fminf(fmaxf(image[ch * n + p], 0.f), 1.f) * al;
            const float y = fminf(fmaxf(gt[ch * n + p], 0.f), 1.f) * al;
            batch[ch * n + p] = (x - mean[ch]) / sd[ch];
            batch[(3 + ch) * n + p] = (y - mean[ch]) / sd[ch];
        }
    }
}

__global__ __launch_bounds__(64) void lpips_accumulate_kernel(const double *__restrict__ lpips,
                                                              const double *__restrict__ frame, int n_rows,
                                                              double *__restrict__ totals) {
    const int row = threadIdx.x;
    if (row >= n_rows) return;
    const double *f = frame + (size_t)row * 8;  // GSR_EVAL_FRAME_COLS: [4] weight, [5] evaluated
    const double wt = f[4];
    if (f[5] == 0.0 || wt == 0.0) return;
    totals[(size_t)row * GSR_LPIPS_TOTAL_COLS] += wt * lpips[row];
    totals[(size_t)row * GSR_LPIPS_TOTAL_COLS + 1] += wt;
}

int64_t tap_blocks(int h, int w) {
    const int64_t Q = (int64_t)((h + 1) / 2) * ((w + 1) / 2);
    return (Q + kTapQuads - 1) / kTapQuads;
}

bool bad_regions(int n) { return n < 0 || n > GSR_LPIPS_MAX_REGIONS; }

// The largest workgroup asks for more than the 64 KiB a kernel gets without saying so.
template <bool kVec, bool kHold>
hipError_t tap_launch(const TapArgs &a, int nw, int64_t nb, float *part, hipStream_t s) {
    static const hipError_t attr =
        hipFuncSetAttribute((const void *)lpips_tap_kernel<kVec, kHold>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)tap_lds(kTapMaxWaves));
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL((lpips_tap_kernel<kVec, kHold>), dim3((unsigned)nb), dim3(64 * nw), tap_lds(nw), s, a, part);
    return hipSuccess;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_lpips_prepare(const float *image, const float *gt, const float *alpha_mask, int H, int W, float *batch,
                      void *stream) {
    if (H <= 0 || W <= 0 || !image || !gt || !batch) {
        set_last_error("gsr_lpips_prepare: empty image or NULL pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const int64_t n = (int64_t)H * W;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(lpips_prepare_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), image, gt,
                       alpha_mask, n, batch);
    return launched("gsr_lpips_prepare");
}

size_t gsr_lpips_tap_scratch_bytes(int h, int w, int n_regions) {
    if (h <= 0 || w <= 0 || bad_regions(n_regions)) return 0;
    return sizeof(float) * 2 * (size_t)(1 + n_regions) * (size_t)tap_blocks(h, w);
}

int gsr_lpips_tap(const float *features, const float *lin, int C, int h, int w, const uint16_t *region_bits,
                  int n_regions, int H, int W, float *pooled_out, void *scratch, double *out, void *stream) {
    if (C <= 0 || h <= 0 || w <= 0 || !features || !lin || !scratch || !out) {
        set_last_error("gsr_lpips_tap: empty feature map or NULL pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (bad_regions(n_regions) || (n_regions > 0 && !region_bits)) {
        set_last_error("gsr_lpips_tap: n_regions outside 0..16, or regions without region_bits");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (n_regions > 0 && (H < h || W < w)) {
        set_last_error("gsr_lpips_tap: the bits plane is smaller than the feature map");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const int64_t nb = tap_blocks(h, w);
    if (nb > 0x7fffffff) {
        set_last_error("gsr_lpips_tap: feature map too large");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const TapArgs a{features, lin, n_regions > 0 ? region_bits : nullptr, pooled_out, C, h, w, n_regions, H, W};
    float *part = static_cast<float *>(scratch);
    // waves per workgroup: eight channels each where that gives 4, 8 or 16 waves (kept in registers),
    // else 16 channels or more each
    const bool hold = C % kTapHold == 0 && (C / kTapHold == 4 || C / kTapHold == 8 || C / kTapHold == 16);
    const int nw = hold ? C / kTapHold : C < 128 ? 4 : C < 256 ? 8 : kTapMaxWaves;
    const bool vec = w % 2 == 0 && reinterpret_cast<uintptr_t>(features) % 8 == 0;
    const hipError_t e = vec ? (hold ? tap_launch<true, true>(a, nw, nb, part, s) : tap_launch<true, false>(a, nw, nb, part, s))
                             : (hold ? tap_launch<false, true>(a, nw, nb, part, s) : tap_launch<false, false>(a, nw, nb, part, s));
    if (e != hipSuccess) {
        set_last_error(std::string("gsr_lpips_tap: ") + hipGetErrorString(e));
        return GSR_ERR_DEVICE;
    }
    hipLaunchKernelGGL(lpips_finalize_kernel, dim3(1 + n_regions), dim3(256), 0, s, part, (int)nb, h, w, out);
    return launched("gsr_lpips_tap");
}

int gsr_lpips_accumulate(const double *lpips, const double *frame, int n_rows, double *totals, void *stream) {
    if (!lpips || !frame || !totals || n_rows < 1 || n_rows > 1 + GSR_LPIPS_MAX_REGIONS) {
        set_last_error("gsr_lpips_accumulate: NULL pointer or n_rows outside 1..17");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(lpips_accumulate_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), lpips, frame,
                       n_rows, totals);
    return launched("gsr_lpips_accumulate");
}

}  // extern "C"
