// views.hip -- training views kept compact on the device (include/gsr_views.h): Pillow's 8-bit Lanczos
// resize with host-made coefficient tables, and the one-launch expansion of a compact view (RGB8, mask8,
// source-resolution depth16) into the float32 planes the steps and the evaluator read.
//
//   resize_h: one 256-thread workgroup per 256 output pixels of one source row, a lane per output pixel
//          of all channels.  The taps of neighbouring outputs overlap (6 scale + 1 each, 13 at 2x), so
//          the workgroup stages the source segment its outputs cover into LDS once, with dword loads
//          from the 4-byte boundary below the segment (rows start off such a boundary when W C is not a
//          multiple of 4; the last dword of the image is read bytewise), and every lane reads its
//          taps' bytes from LDS.  A segment longer than kStagePx pixels is staged in pieces and each
//          lane adds the taps that fall into the piece.  The coefficient table is stored tap-major
//          (ksize, out) so that the lanes of a wave read consecutive words.
//   resize_v: a lane per 4 consecutive bytes of an output row (rows whose byte count is a multiple of 4),
//          or per byte: it walks its taps down the rows of the intermediate image, every load and the
//          store coalesced; the tap's coefficient is the same for the whole workgroup (scalar loads).
//   expand:  a lane per 4 consecutive pixels of the flat image: three dwords of RGB, one of mask, four
//          bilinear depth samples, six float4 stores.  The last lane takes the ragged tail bytewise.
//
// The arithmetic is integer in the resize and single IEEE operations in the expansion (the file is
// compiled with fp contraction off; the depth affine map uses the explicitly rounded intrinsics), so
// the numpy restatements in tests/views_ref.py are matched bit for bit.
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/gsr.h"
#include "../../include/gsr_views.h"
#include "gsr_launch.h"

namespace gsr {
namespace {

constexpr uint64_t kPlanMagic = 0x6773725f72737a70ull;  // "gsr_rszp"
constexpr int kPrecisionBits = 22;
constexpr int kMaxSide = 32768;
constexpr int kBlock = 256;
constexpr int kStagePx = 4096;  // source pixels staged per piece: 12 KiB of LDS at 3 channels

struct Axis {
    int in = 0, out = 0, ksize = 0;   // ksize 0: the pass is skipped
    std::vector<int32_t> bounds;      // (out, 2): xmin, count
    std::vector<int32_t> coeffs;      // (out, ksize), zero past the count
};

struct Plan {
    uint64_t magic = 0;
    int in_w = 0, in_h = 0, out_w = 0, out_h = 0;
    Axis x, y;
    int device = -1;            // where the tables live (-1: not uploaded)
    int32_t *d_tables = nullptr;
    size_t off_xb = 0, off_xc = 0, off_yb = 0, off_yc = 0, table_words = 0;
    int64_t uploads = 0;
};

double sinc_pi(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

double lanczos3(double t) {
    return (-3.0 <= t && t < 3.0) ? sinc_pi(t) * sinc_pi(t / 3.0) : 0.0;
}

void make_axis(int in, int out, Axis *a) {
    a->in = in;
    a->out = out;
    if (in == out) return;
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * fs;
    a->ksize = (int)ceil(support) * 2 + 1;
    a->bounds.assign((size_t)out * 2, 0);
    a->coeffs.assign((size_t)out * a->ksize, 0);
    std::vector<double> w((size_t)a->ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = lanczos3((x + xmin - center + 0.5) / fs);
            ww += w[x];
        }
        int32_t *k = &a->coeffs[(size_t)xx * a->ksize];
        for (int x = 0; x < n; ++x) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int32_t)(v * (double)(1 << kPrecisionBits) - 0.5)
                         : (int32_t)(v * (double)(1 << kPrecisionBits) + 0.5);
        }
        a->bounds[2 * (size_t)xx] = xmin;
        a->bounds[2 * (size_t)xx + 1] = n;
    }
}

Plan *plan_of(const void *p) {
    Plan *pl = (Plan *)p;
    return pl && pl->magic == kPlanMagic ? pl : nullptr;
}

__device__ __forceinline__ uint8_t clip8(int v) {
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---- the horizontal pass ----------------------------------------------------------------------------

template <int C>
__global__ __launch_bounds__(kBlock) void resize_h_kernel(const uint8_t *__restrict__ src, int in_w, int out_w, int ksize,
                                                          const int32_t *__restrict__ bounds,
                                                          const int32_t *__restrict__ coeff_t, int64_t total_bytes,
                                                          uint8_t *__restrict__ dst) {
    // a piece is at most kStagePx * C bytes plus the 3 in front of it down to the dword boundary
    __shared__ uint32_t stage[(kStagePx * C + 6) / 4 + 1];
    const int y = blockIdx.y;
    const int x0 = blockIdx.x * kBlock;
    const int xx = x0 + (int)threadIdx.x;
    const bool live = xx < out_w;
    const int xl = min(x0 + kBlock - 1, out_w - 1);
    // xmin and xmin + count do not decrease with xx: the workgroup's outputs read [seg0, seg1)
    const int seg0 = bounds[2 * x0];
    const int seg1 = bounds[2 * xl] + bounds[2 * xl + 1];
    const int xmin = live ? bounds[2 * xx] : 0;
    const int cnt = live ? bounds[2 * xx + 1] : 0;
    const int64_t row = (int64_t)y * in_w * C;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (kPrecisionBits - 1);

    for (int q0 = seg0; q0 < seg1; q0 += kStagePx) {
        const int q1 = min(q0 + kStagePx, seg1);
        const int64_t first = row + (int64_t)q0 * C;
        const int64_t p0 = first & ~(int64_t)3;
        const int64_t pend = row + (int64_t)q1 * C;  // <= total_bytes
        const int nd = (int)((pend - p0 + 3) >> 2);
        for (int i = threadIdx.x; i < nd; i += kBlock) {
            const int64_t a = p0 + 4 * (int64_t)i;
            uint32_t v = 0;
            if (a + 4 <= total_bytes) {
                v = *(const uint32_t *)(src + a);
            } else {
                for (int j = 0; j < 4; ++j)
                    if (a + j < total_bytes) v |= (uint32_t)src[a + j] << (8 * j);
            }
            stage[i] = v;
        }
        __syncthreads();
        if (live) {
            const int ka = max(0, q0 - xmin), kb = min(cnt, q1 - xmin);
            // byte of tap k, channel c: (first - p0) + (xmin + k - q0) * C + c, >= 0 for k >= ka
            const uint8_t *sb = (const uint8_t *)stage + (int)(first - p0);
            for (int k = ka; k < kb; ++k) {
                const int w = coeff_t[(int64_t)k * out_w + xx];
                const int o = (xmin + k - q0) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += w * (int)sb[o + c];
            }
        }
        __syncthreads();
    }
    if (live) {
        uint8_t *d = dst + ((int64_t)y * out_w + xx) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = clip8(acc[c] >> kPrecisionBits);
    }
}

// ---- the vertical pass --------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kBlock) void resize_v_kernel(const uint8_t *__restrict__ src, int64_t row_bytes, int ksize,
                                                          const int32_t *__restrict__ bounds,
                                                          const int32_t *__restrict__ coeffs, uint8_t *__restrict__ dst) {
    const int yy = blockIdx.y;
    const int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
    const int32_t *k = coeffs + (int64_t)yy * ksize;
    const int64_t j = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * (VEC ? 4 : 1);
    if (j >= row_bytes) return;
    const uint8_t *s = src + (int64_t)ymin * row_bytes + j;
    if (VEC) {
        int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0, a3 = a0;
        for (int t = 0; t < cnt; ++t) {
            const int w = k[t];
            const uint32_t v = *(const uint32_t *)(s + (int64_t)t * row_bytes);
            a0 += w * (int)(v & 255u);
            a1 += w * (int)((v >> 8) & 255u);
            a2 += w * (int)((v >> 16) & 255u);
            a3 += w * (int)(v >> 24);
        }
        // Each byte is clipped on its own and hidden from the optimiser before the four are packed: for a
        // shift-clip-pack of two sums hipcc selects v_ashr_pk_u8_i32 and then takes the upper half of
        // its result for zero, which on the MI355X it was not -- bytes 2 and 3 of the dword came out
        // ORed with stray bits.
        uint32_t b0 = clip8(a0 >> kPrecisionBits), b1 = clip8(a1 >> kPrecisionBits);
        uint32_t b2 = clip8(a2 >> kPrecisionBits), b3 = clip8(a3 >> kPrecisionBits);
        asm volatile("" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3));
        const uint32_t o = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        *(uint32_t *)(dst + (int64_t)yy * row_bytes + j) = o;
    } else {
        int a0 = 1 << (kPrecisionBits - 1);
        for (int t = 0; t < cnt; ++t) a0 += k[t] * (int)s[(int64_t)t * row_bytes];
        dst[(int64_t)yy * row_bytes + j] = clip8(a0 >> kPrecisionBits);
    }
}

// ---- the expansion ------------------------------------------------------------------------------------

struct ExpandArgs {
    int W, H, dW, dH;
    const uint8_t *rgb, *mask;
    const uint16_t *depth;
    int zero_half, depth_valid;
    float scale, offset;
    double sx, sy;  // (double)dW / W, (double)dH / H
    float *image, *alpha, *invdepth, *depth_mask;
};

// the linear rule's tap of output sample d on an axis of `in` source samples
__device__ __forceinline__ void linear_tap(int d, double scale, int in, int *i0, int *i1, float *f) {
    float v = (float)((d + 0.5) * scale - 0.5);
    int i = (int)floorf(v);
    v -= (float)i;
    if (i < 0) {
        i = 0;
        v = 0.f;
    }
    if (i >= in - 1) {
        i = in - 1;
        v = 0.f;
    }
    *i0 = i;
    *i1 = min(i + 1, in - 1);
    *f = v;
}

__device__ __forceinline__ float depth_affine(const ExpandArgs &a, int y, int x) {
    const float m = (float)a.depth[(int64_t)y * a.dW + x] / 65536.0f;
    return __fadd_rn(__fmul_rn(m, a.scale), a.offset);
}

__global__ __launch_bounds__(kBlock) void view_expand_kernel(ExpandArgs a) {
    const int64_t n = (int64_t)a.W * a.H;
    const int64_t p0 = 4 * ((int64_t)blockIdx.x * kBlock + threadIdx.x);
    if (p0 >= n) return;
    const int m = (int)min((int64_t)4, n - p0);
    uint32_t rgb[3] = {0, 0, 0}, mk = 0xffffffffu;
    if (m == 4) {
        if (a.rgb) {
            const uint32_t *r = (const uint32_t *)(a.rgb + 3 * p0);
            rgb[0] = r[0];
            rgb[1] = r[1];
            rgb[2] = r[2];
        }
        if (a.mask) mk = *(const uint32_t *)(a.mask + p0);
    } else {
        if (a.rgb)
            for (int b = 0; b < 3 * m; ++b) rgb[b >> 2] |= (uint32_t)a.rgb[3 * p0 + b] << (8 * (b & 3));
        if (a.mask) {
            mk = 0;
            for (int b = 0; b < m; ++b) mk |= (uint32_t)a.mask[p0 + b] << (8 * b);
        }
    }
    int y = (int)(p0 / a.W), x = (int)(p0 - (int64_t)y * a.W);
    const int half = a.W / 2;
    float img[3][4], al[4], dv[4], dm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float alpha = a.mask ? (float)((mk >> (8 * i)) & 255u) / 255.0f : 1.0f;
        if ((a.zero_half == 1 && x < half) || (a.zero_half == 2 && x >= half)) alpha = 0.f;
        al[i] = alpha;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int b = 3 * i + c;
            const float v = (float)((rgb[b >> 2] >> (8 * (b & 3))) & 255u) / 255.0f;
            img[c][i] = a.rgb ? fminf(fmaxf(v, 0.f), 1.f) * alpha : 0.f;
        }
        dv[i] = 0.f;
        dm[i] = alpha;
        if (a.depth && i < m) {
            int x0, x1, y0, y1;
            float fx, fy;
            linear_tap(x, a.sx, a.dW, &x0, &x1, &fx);
            linear_tap(y, a.sy, a.dH, &y0, &y1, &fy);
            const float a0 = 1.f - fx, b0 = 1.f - fy;
            const float h0 = __fadd_rn(__fmul_rn(a0, depth_affine(a, y0, x0)), __fmul_rn(fx, depth_affine(a, y0, x1)));
            const float h1 = __fadd_rn(__fmul_rn(a0, depth_affine(a, y1, x0)), __fmul_rn(fx, depth_affine(a, y1, x1)));
            float d = __fadd_rn(__fmul_rn(b0, h0), __fmul_rn(fy, h1));
            if (d < 0.f) d = 0.f;
            dv[i] = d;
            if (a.depth_valid == 1 && d == 0.f) dm[i] = 0.f;
        }
        if (++x == a.W) {
            x = 0;
            ++y;
        }
    }
    if (m == 4) {
        if ((n & 3) == 0) {  // else the second and third colour planes start off a 16-byte boundary
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *(float4 *)(a.image + (int64_t)c * n + p0) = make_float4(img[c][0], img[c][1], img[c][2], img[c][3]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) a.image[(int64_t)c * n + p0 + i] = img[c][i];
        }
        *(float4 *)(a.alpha + p0) = make_float4(al[0], al[1], al[2], al[3]);
        if (a.depth) {
            *(float4 *)(a.invdepth + p0) = make_float4(dv[0], dv[1], dv[2], dv[3]);
            *(float4 *)(a.depth_mask + p0) = make_float4(dm[0], dm[1], dm[2], dm[3]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= m) continue;
            for (int c = 0; c < 3; ++c) a.image[(int64_t)c * n + p0 + i] = img[c][i];
            a.alpha[p0 + i] = al[i];
            if (a.depth) {
                a.invdepth[p0 + i] = dv[i];
                a.depth_mask[p0 + i] = dm[i];
            }
        }
    }
}

int invalid(const std::string &msg) {
    set_last_error(msg);
    return GSR_ERR_INVALID_ARGUMENT;
}

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

void *gsr_resize_plan_create(int in_w, int in_h, int out_w, int out_h) {
    for (int v : {in_w, in_h, out_w, out_h})
        if (v < 1 || v > kMaxSide) {
            set_last_error("gsr_resize_plan_create: every size must be in 1 .. 32768");
            return nullptr;
        }
    Plan *p = new (std::nothrow) Plan();
    if (!p) {
        set_last_error("gsr_resize_plan_create: out of host memory");
        return nullptr;
    }
    p->in_w = in_w;
    p->in_h = in_h;
    p->out_w = out_w;
    p->out_h = out_h;
    make_axis(in_w, out_w, &p->x);
    make_axis(in_h, out_h, &p->y);
    p->off_xb = 0;
    p->off_xc = p->off_xb + p->x.bounds.size();
    p->off_yb = p->off_xc + p->x.coeffs.size();
    p->off_yc = p->off_yb + p->y.bounds.size();
    p->table_words = p->off_yc + p->y.coeffs.size();
    p->magic = kPlanMagic;
    return p;
}

void gsr_resize_plan_destroy(void *plan) {
    Plan *p = plan_of(plan);
    if (!p) return;
    p->magic = 0;
    if (p->d_tables) {
        int cur = -1;
        const bool there = hipGetDevice(&cur) == hipSuccess;
        if (there && cur != p->device) (void)hipSetDevice(p->device);
        (void)hipFree(p->d_tables);
        if (there && cur != p->device) (void)hipSetDevice(cur);
    }
    delete p;
}

int gsr_resize_plan_info(const void *plan, int64_t *out, int n) {
    const Plan *p = plan_of(plan);
    if (!p || !out || n < 0) return invalid("gsr_resize_plan_info: not a live plan, or no output");
    const int64_t v[5] = {p->uploads, p->x.ksize, p->y.ksize, (int64_t)(p->table_words * sizeof(int32_t)),
                          (int64_t)gsr_resize_scratch_bytes(plan, 1)};
    for (int i = 0; i < n && i < 5; ++i) out[i] = v[i];
    return GSR_OK;
}

int gsr_resize_plan_tables(const void *plan, int axis, int32_t *bounds, int32_t *coeffs) {
    const Plan *p = plan_of(plan);
    if (!p || (axis != 0 && axis != 1) || !bounds || !coeffs)
        return invalid("gsr_resize_plan_tables: not a live plan, axis not 0 or 1, or no output");
    const Axis &a = axis == 0 ? p->x : p->y;
    if (a.ksize == 0) return invalid("gsr_resize_plan_tables: this axis keeps its size: the pass is skipped");
    memcpy(bounds, a.bounds.data(), a.bounds.size() * sizeof(int32_t));
    memcpy(coeffs, a.coeffs.data(), a.coeffs.size() * sizeof(int32_t));
    return GSR_OK;
}

size_t gsr_resize_scratch_bytes(const void *plan, int channels) {
    const Plan *p = plan_of(plan);
    if (!p || (channels != 1 && channels != 3)) return 0;
    return p->x.ksize && p->y.ksize ? (size_t)p->out_w * p->in_h * channels : 0;
}

int gsr_resize_lanczos_u8(void *plan, const uint8_t *src, int channels, void *scratch, uint8_t *dst, void *stream) {
    Plan *p = plan_of(plan);
    if (!p) return invalid("gsr_resize_lanczos_u8: not a live plan");
    if (channels == 4)
        return invalid("gsr_resize_lanczos_u8: 4 channels are refused: Pillow premultiplies an RGBA image's colour by "
                       "its alpha around the filter, which a plain 4-channel pass does not; resize RGB and the "
                       "alpha plane as Pillow would, or drop the alpha");
    if (channels != 1 && channels != 3) return invalid("gsr_resize_lanczos_u8: channels must be 1 or 3");
    const bool two = p->x.ksize && p->y.ksize;
    if (!src || !dst || (two && !scratch)) return invalid("gsr_resize_lanczos_u8: NULL src, dst or scratch");
    if (!aligned(src, 4) || !aligned(dst, 4) || !aligned(scratch, 4))
        return invalid("gsr_resize_lanczos_u8: src, dst and scratch must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int C = channels;
    if (!p->x.ksize && !p->y.ksize) {
        const hipError_t e = hipMemcpyAsync(dst, src, (size_t)p->in_w * p->in_h * C, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) {
            set_last_error(std::string("gsr_resize_lanczos_u8: copy: ") + hipGetErrorString(e));
            return GSR_ERR_DEVICE;
        }
        return GSR_OK;
    }
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) {
        set_last_error("gsr_resize_lanczos_u8: no device");
        return GSR_ERR_DEVICE;
    }
    if (p->d_tables && p->device != dev)
        return invalid("gsr_resize_lanczos_u8: the plan's tables live on another device: one plan per device");
    if (!p->d_tables) {
        std::vector<int32_t> host(p->table_words);
        memcpy(&host[p->off_xb], p->x.bounds.data(), p->x.bounds.size() * sizeof(int32_t));
        // the horizontal table tap-major: the lanes of a wave (consecutive outputs) read consecutive words
        for (int xx = 0; xx < (p->x.ksize ? p->x.out : 0); ++xx)
            for (int k = 0; k < p->x.ksize; ++k)
                host[p->off_xc + (size_t)k * p->x.out + xx] = p->x.coeffs[(size_t)xx * p->x.ksize + k];
        memcpy(&host[p->off_yb], p->y.bounds.data(), p->y.bounds.size() * sizeof(int32_t));
        memcpy(&host[p->off_yc], p->y.coeffs.data(), p->y.coeffs.size() * sizeof(int32_t));
        void *d = nullptr;
        hipError_t e = hipMalloc(&d, p->table_words * sizeof(int32_t));
        if (e != hipSuccess) {
            set_last_error(std::string("gsr_resize_lanczos_u8: table allocation: ") + hipGetErrorString(e));
            return GSR_ERR_ALLOCATION;
        }
        e = hipMemcpy(d, host.data(), p->table_words * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            set_last_error(std::string("gsr_resize_lanczos_u8: table upload: ") + hipGetErrorString(e));
            return GSR_ERR_DEVICE;
        }
        p->d_tables = (int32_t *)d;
        p->device = dev;
        p->uploads += 1;
    }
    const int32_t *T = p->d_tables;
    const uint8_t *vsrc = src;
    if (p->x.ksize) {
        uint8_t *hdst = two ? (uint8_t *)scratch : dst;
        const dim3 grid((unsigned)((p->out_w + kBlock - 1) / kBlock), (unsigned)p->in_h);
        const int64_t total = (int64_t)p->in_w * p->in_h * C;
        if (C == 1)
            resize_h_kernel<1><<<grid, kBlock, 0, s>>>(src, p->in_w, p->out_w, p->x.ksize, T + p->off_xb, T + p->off_xc,
                                                       total, hdst);
        else
            resize_h_kernel<3><<<grid, kBlock, 0, s>>>(src, p->in_w, p->out_w, p->x.ksize, T + p->off_xb, T + p->off_xc,
                                                       total, hdst);
        vsrc = hdst;
    }
    if (p->y.ksize) {
        const int64_t row_bytes = (int64_t)p->out_w * C;
        const bool vec = row_bytes % 4 == 0;
        const int64_t lanes = vec ? row_bytes / 4 : row_bytes;
        const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock), (unsigned)p->out_h);
        if (vec)
            resize_v_kernel<true><<<grid, kBlock, 0, s>>>(vsrc, row_bytes, p->y.ksize, T + p->off_yb, T + p->off_yc, dst);
        else
            resize_v_kernel<false><<<grid, kBlock, 0, s>>>(vsrc, row_bytes, p->y.ksize, T + p->off_yb, T + p->off_yc, dst);
    }
    return launched("gsr_resize_lanczos_u8");
}

int gsr_view_expand(int W, int H, const uint8_t *rgb, const uint8_t *mask, int zero_half, const uint16_t *depth, int dW,
                    int dH, float scale, float offset, int depth_valid, float *image, float *alpha, float *invdepth,
                    float *depth_mask, void *stream) {
    if (W < 1 || H < 1 || W > kMaxSide || H > kMaxSide) return invalid("gsr_view_expand: W, H must be in 1 .. 32768");
    if (zero_half < 0 || zero_half > 2 || depth_valid < 0 || depth_valid > 1)
        return invalid("gsr_view_expand: zero_half must be 0, 1 or 2 and depth_valid 0 or 1");
    if (!image || !alpha) return invalid("gsr_view_expand: NULL image or alpha plane");
    if (depth) {
        if (dW < 1 || dH < 1 || dW > kMaxSide || dH > kMaxSide)
            return invalid("gsr_view_expand: the depth map's dW, dH must be in 1 .. 32768");
        if (!invdepth || !depth_mask) return invalid("gsr_view_expand: depth given without its two planes");
        if (!std::isfinite(scale) || !std::isfinite(offset)) return invalid("gsr_view_expand: scale, offset must be finite");
        if (!aligned(depth, 2)) return invalid("gsr_view_expand: depth must be 2-byte aligned");
    } else if (invdepth || depth_mask) {
        return invalid("gsr_view_expand: depth planes given without a depth map");
    }
    if (!aligned(rgb, 4) || !aligned(mask, 4)) return invalid("gsr_view_expand: rgb and mask must be 4-byte aligned");
    if (!aligned(image, 16) || !aligned(alpha, 16) || !aligned(invdepth, 16) || !aligned(depth_mask, 16))
        return invalid("gsr_view_expand: the planes must be 16-byte aligned");
    ExpandArgs a;
    a.W = W;
    a.H = H;
    a.dW = depth ? dW : 1;
    a.dH = depth ? dH : 1;
    a.rgb = rgb;
    a.mask = mask;
    a.depth = depth;
    a.zero_half = zero_half;
    a.depth_valid = depth_valid;
    a.scale = scale;
    a.offset = offset;
    a.sx = (double)a.dW / (double)W;
    a.sy = (double)a.dH / (double)H;
    a.image = image;
    a.alpha = alpha;
    a.invdepth = invdepth;
    a.depth_mask = depth_mask;
    const int64_t lanes = ((int64_t)W * H + 3) / 4;
    view_expand_kernel<<<(unsigned)((lanes + kBlock - 1) / kBlock), kBlock, 0, (hipStream_t)stream>>>(a);
    return launched("gsr_view_expand");
}

}  // extern "C"
