// model_init.hip -- the model from a point cloud, and the scaffold rows in front of a chunk
// (include/gsr_model_init.h).  Streaming kernels, bound by memory.
//
//   gsr_model_init_cloud (scene/gaussian_model.py:163-222)
//     bbox:     per-thread min / max over a grid-stride range, wave reduction by __shfl_xor, one
//               value per block, one combining block; the same pass finds the first non-finite point
//               (atomicMin on its index).  The host reads the box and that index once.
//     skybox:   the S skybox positions (direction in fp64, rounded once; then two fp32 operations)
//     kNN:      gsr_knn_mean_dist2 over the S + N output positions
//     rows:     one launch over every SH float; the first `rows` threads also write their row's
//               opacity, scaling and rotation
//
//   gsr_scaffold_merge_count / _write (:224-264)
//     flags:    the ring predicate, one ballot per wave: the wave's 64-bit mask and its popcount
//     scan:     rocPRIM exclusive scan of the wave counts
//     list:     selected row -> its output position (wave base + popcount of the lower lanes); K
//     write:    one launch over every output SH float of [K selected rows | chunk rows]; the first
//               K + Pc threads also copy their row's other four arrays
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>  // memset, for rocprim.hpp
#include <string>

#include <rocprim/rocprim.hpp>

#include "../../include/gsr.h"
#include "../../include/gsr_knn.h"
#include "../../include/gsr_model_init.h"
#include "grid_cell.h"  // wave_minf / wave_maxf
#include "gsr_launch.h"

namespace gsr {
namespace {

constexpr int kBBoxBlocks = 1024;
constexpr float kSHC0 = 0.28209479177387814f;  // utils/sh_utils.py C0, as torch rounds the scalar

struct BBoxPart {
    float lo[3], hi[3];
};
struct BBoxOut {
    float lo[3], hi[3];
    unsigned long long bad;  // index of the first point with a NaN or Inf coordinate; ~0: none
};

struct InitLayout {
    BBoxOut *box;
    BBoxPart *part;
    float *dist2;
    void *knn;
    size_t total;
};

InitLayout init_layout(char *base, int64_t N, int64_t S) {
    InitLayout L{};
    Carve c(base);
    L.box = c.take<BBoxOut>(sizeof(BBoxOut));
    L.part = c.take<BBoxPart>(sizeof(BBoxPart) * kBBoxBlocks);
    L.dist2 = c.take<float>(sizeof(float) * (size_t)(S + N));
    L.knn = c.take(gsr_knn_scratch_bytes(S + N));
    L.total = c.off;
    return L;
}

// Block reduction of six values (three minima, three maxima): waves, then wave 0 over the waves' values.
__device__ inline void block_minmax(float lo[3], float hi[3], float (*sh)[6]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = wave_minf(lo[c]);
        hi[c] = wave_maxf(hi[c]);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sh[w][c] = lo[c];
            sh[w][3 + c] = hi[c];
        }
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = wave_minf(lane < nw ? sh[lane][c] : FLT_MAX);
            hi[c] = wave_maxf(lane < nw ? sh[lane][3 + c] : -FLT_MAX);
        }
    }
}

// fminf / fmaxf drop a NaN, so the box is that of the finite coordinates; `bad` carries the rest
__global__ __launch_bounds__(256) void bbox_kernel(int64_t N, const float *__restrict__ pts,
                                                   BBoxPart *__restrict__ part, BBoxOut *__restrict__ box) {
    __shared__ float sh[4][6];
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    unsigned long long bad = ~0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = pts[3 * i + c];
            lo[c] = fminf(lo[c], v);
            hi[c] = fmaxf(hi[c], v);
            if (!isfinite(v) && (unsigned long long)i < bad) bad = (unsigned long long)i;
        }
    }
    if (bad != ~0ull) atomicMin(&box->bad, bad);
    block_minmax(lo, hi, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            part[blockIdx.x].lo[c] = lo[c];
            part[blockIdx.x].hi[c] = hi[c];
        }
    }
}

__global__ __launch_bounds__(256) void bbox_combine_kernel(int n, const BBoxPart *__restrict__ part,
                                                           BBoxOut *__restrict__ box) {
    __shared__ float sh[4][6];
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(lo[c], part[i].lo[c]);
            hi[c] = fmaxf(hi[c], part[i].hi[c]);
        }
    }
    block_minmax(lo, hi, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            box->lo[c] = lo[c];
            box->hi[c] = hi[c];
        }
    }
}

struct Float3 {
    float v[3];
};

// scene/gaussian_model.py:190-196; r10 = 10 * radius
__global__ __launch_bounds__(256) void skybox_kernel(int64_t S, const float *__restrict__ u_theta,
                                                     const float *__restrict__ u_phi, Float3 mean, float r10,
                                                     float *__restrict__ xyz) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S) return;
    double st, ct;
    sincospi(2.0 * (double)u_theta[r], &st, &ct);
    const double cp = 1.0 - 1.4 * (double)u_phi[r];
    const double sp = sqrt(fmax(1.0 - cp * cp, 0.0));
    const float dir[3] = {(float)(ct * sp), (float)(st * sp), (float)cp};
#pragma unroll
    for (int c = 0; c < 3; ++c) xyz[3 * r + c] = mean.v[c] + r10 * dir[c];
}

__global__ __launch_bounds__(256) void init_rows_kernel(int64_t rows, int64_t S, int W, int sky_mode,
                                                        const float *__restrict__ colors,
                                                        const float *__restrict__ dist2, float op_cloud, float op_sky,
                                                        float *__restrict__ features, float *__restrict__ opacity,
                                                        float *__restrict__ scaling, float *__restrict__ rotation) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * W) return;
    const int64_t row = e / W;
    const int k = (int)(e - row * W);
    float v = 0.f;
    if (k < 3) {
        const float rgb = row < S ? (k == 0 ? 0.7f : k == 1 ? 0.8f : 0.95f) : colors[3 * (row - S) + k];
        v = (rgb - 0.5f) / kSHC0;  // RGB2SH: a division
    }
    features[e] = v;
    if (e < rows) {
        float d = fmaxf(dist2[e], 0.0000001f);
        if (sky_mode) d = e < S ? d * 10.f : fminf(d, 10.f);
        const float s = logf(sqrtf(d));
        scaling[3 * e] = s;
        scaling[3 * e + 1] = s;
        scaling[3 * e + 2] = s;
        rotation[4 * e] = 1.f;
        rotation[4 * e + 1] = 0.f;
        rotation[4 * e + 2] = 0.f;
        rotation[4 * e + 3] = 0.f;
        opacity[e] = e < S ? op_sky : op_cloud;
    }
}

// ---- scaffold selection ----

struct MergeLayout {
    unsigned long long *mask;  // per wave of 64 rows
    uint32_t *cnt, *pre;       // per wave: selected rows, and those of the waves before it
    uint32_t *list;            // the selected rows in order (at most Ps)
    void *tmp;
    size_t tmp_bytes, total;
};

MergeLayout merge_layout(char *base, int64_t Ps) {
    MergeLayout L{};
    Carve c(base);
    const size_t n = (size_t)(Ps > 0 ? Ps : 1), nw = (n + 63) / 64;
    L.mask = c.take<unsigned long long>(sizeof(unsigned long long) * nw);
    L.cnt = c.take<uint32_t>(sizeof(uint32_t) * nw);
    L.pre = c.take<uint32_t>(sizeof(uint32_t) * nw);
    L.list = c.take<uint32_t>(sizeof(uint32_t) * n);
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, nw,
                            rocprim::plus<uint32_t>());
    L.tmp_bytes = bytes;
    L.tmp = c.take(bytes);
    L.total = c.off;
    return L;
}

// blocks of 256 threads over rows in order: a wave holds rows 64 w .. 64 w + 63
__global__ __launch_bounds__(256) void merge_flags_kernel(int64_t Ps, int64_t S, const float *__restrict__ xyz,
                                                          float cx, float cy, float lo, float hi,
                                                          unsigned long long *__restrict__ mask,
                                                          uint32_t *__restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool sel = false;
    if (r < Ps) {
        const float ax = fabsf(xyz[3 * r] - cx), ay = fabsf(xyz[3 * r + 1] - cy);
        // torch.max carries a NaN of either side; fmaxf would drop it
        const float m = (isnan(ax) || isnan(ay)) ? NAN : fmaxf(ax, ay);
        sel = r < S || (m > lo && m < hi);
    }
    const unsigned long long b = __ballot(sel);
    if ((threadIdx.x & 63) == 0 && r < Ps) {
        mask[r >> 6] = b;
        cnt[r >> 6] = (uint32_t)__popcll(b);
    }
}

__global__ __launch_bounds__(256) void merge_list_kernel(int64_t Ps, const unsigned long long *__restrict__ mask,
                                                         const uint32_t *__restrict__ cnt,
                                                         const uint32_t *__restrict__ pre,
                                                         uint32_t *__restrict__ list, int64_t *__restrict__ count) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= Ps) return;
    const int64_t w = r >> 6;
    const int lane = (int)(r & 63);
    const unsigned long long b = mask[w];
    if ((b >> lane) & 1ull) list[pre[w] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)r;
    if (r == Ps - 1) *count = (int64_t)pre[w] + cnt[w];
}

struct MergeRows {
    const float *xyz, *shs, *opacity, *scaling, *rotation;
};
struct MergeOut {
    float *xyz, *shs, *opacity, *scaling, *rotation;
};

__global__ __launch_bounds__(256) void merge_write_kernel(int64_t Ps, int64_t K, int64_t Pc, int W, MergeRows sc,
                                                          MergeRows ch, const uint32_t *__restrict__ list,
                                                          MergeOut out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t rows = K + Pc;
    if (e >= rows * W) return;
    const int64_t row = e / W;
    const int k = (int)(e - row * W);
    float v = 0.f;
    if (row < K) {
        const int64_t src = list[row];
        if (k < 12 && src < Ps) v = sc.shs[12 * src + k];
    } else {
        v = ch.shs[(row - K) * W + k];
    }
    out.shs[e] = v;
    if (e < rows) {
        const bool scaffold = e < K;
        const int64_t src = scaffold ? (int64_t)list[e] : e - K;
        if (scaffold && src >= Ps) return;  // a K that is not the counted one: nothing to copy
        const MergeRows &in = scaffold ? sc : ch;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            out.xyz[3 * e + c] = in.xyz[3 * src + c];
            out.scaling[3 * e + c] = in.scaling[3 * src + c];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) out.rotation[4 * e + c] = in.rotation[4 * src + c];
        out.opacity[e] = in.opacity[src];
    }
}

int fail(int rc, const std::string &msg) {
    set_last_error(msg);
    return rc;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_model_init_scratch_bytes(int64_t N, int64_t S) {
    if (N < 1 || S < 0 || N + S >= (1LL << 31)) return 0;
    return init_layout(nullptr, N, S).total;
}

int gsr_model_init_cloud(int64_t N, const float *points, const float *colors, int64_t S, const float *u_theta,
                         const float *u_phi, int M, int mode, float *xyz, float *features, float *opacity_raw,
                         float *scaling_raw, float *rotation, float *bounds, void *scratch, void *stream) {
    const char *who = "gsr_model_init_cloud";
    if (N < 1 || S < 0 || N + S >= (1LL << 31) || M < 1 || M > 16)
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": bad sizes (N >= 1, S >= 0, N + S < 2^31, 1 <= M <= 16)");
    if (!(mode == GSR_MODEL_INIT_SKYBOX && S >= 1) && !(mode == GSR_MODEL_INIT_PLAIN && S == 0))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": skybox mode needs S >= 1, plain mode S == 0");
    if (!points || !colors || (S > 0 && (!u_theta || !u_phi)) || !xyz || !features || !opacity_raw || !scaling_raw ||
        !rotation || !scratch)
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const InitLayout L = init_layout(static_cast<char *>(scratch), N, S);
    const int64_t rows = S + N;

    // the bounding box and the first non-finite point: the one host read
    hipError_t e = hipMemsetAsync(L.box, 0xFF, sizeof(BBoxOut), s);
    if (e != hipSuccess) return fail(GSR_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    const int blocks = (int)std::min<int64_t>((N + 255) / 256, kBBoxBlocks);
    hipLaunchKernelGGL(bbox_kernel, dim3(blocks), dim3(256), 0, s, N, points, L.part, L.box);
    hipLaunchKernelGGL(bbox_combine_kernel, dim3(1), dim3(256), 0, s, blocks, L.part, L.box);
    BBoxOut box;
    e = hipMemcpyAsync(&box, L.box, sizeof(BBoxOut), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(GSR_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    if (box.bad != ~0ull)
        return fail(GSR_ERR_INVALID_ARGUMENT,
                    std::string(who) + ": cloud point " + std::to_string(box.bad) + " has a NaN or Inf coordinate");
    Float3 mean;
    float d[3];
    for (int c = 0; c < 3; ++c) {
        mean.v[c] = 0.5f * (box.lo[c] + box.hi[c]);
        d[c] = box.hi[c] - mean.v[c];
    }
    // torch.linalg.norm; the products and sums rounded to fp32 one by one
    const float radius = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (bounds) {
        for (int c = 0; c < 3; ++c) bounds[c] = mean.v[c];
        bounds[3] = radius;
    }

    if (S > 0)
        hipLaunchKernelGGL(skybox_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, S, u_theta, u_phi, mean,
                           10.f * radius, xyz);
    e = hipMemcpyAsync(xyz + 3 * S, points, sizeof(float) * 3 * (size_t)N, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return fail(GSR_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    const int rc = gsr_knn_mean_dist2(rows, xyz, L.dist2, L.knn, stream);
    if (rc != GSR_OK) return rc;
    const bool sky = mode == GSR_MODEL_INIT_SKYBOX;
    const float op_cloud = (float)std::log((sky ? 0.02 : 0.01) / (1.0 - (sky ? 0.02 : 0.01)));
    const int W = 3 * M;
    hipLaunchKernelGGL(init_rows_kernel, dim3((unsigned)((rows * W + 255) / 256)), dim3(256), 0, s, rows, S, W,
                       sky ? 1 : 0, colors, L.dist2, op_cloud, 0.7f, features, opacity_raw, scaling_raw, rotation);
    return launched(who);
}

size_t gsr_scaffold_merge_scratch_bytes(int64_t Ps) {
    if (Ps < 0 || Ps >= (1LL << 31)) return 0;
    return merge_layout(nullptr, Ps).total;
}

int gsr_scaffold_merge_count(int64_t Ps, int64_t S, const float *xyz, const float *center, const float *extent,
                             void *scratch, int64_t *count, void *stream) {
    const char *who = "gsr_scaffold_merge_count";
    if (Ps < 0 || Ps >= (1LL << 31) || S < 0 || !center || !extent || !scratch || !count || (Ps > 0 && !xyz))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": bad sizes (0 <= Ps < 2^31, S >= 0) or NULL pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MergeLayout L = merge_layout(static_cast<char *>(scratch), Ps);
    if (Ps == 0) {
        const hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), s);
        if (e != hipSuccess) return fail(GSR_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
        return GSR_OK;
    }
    const unsigned blocks = (unsigned)((Ps + 255) / 256);
    const size_t nw = (size_t)((Ps + 63) / 64);
    const float hi = 1.5f * extent[0];  // rounded once
    hipLaunchKernelGGL(merge_flags_kernel, dim3(blocks), dim3(256), 0, s, Ps, S, xyz, center[0], center[1],
                       0.5f * extent[0], hi, L.mask, L.cnt);
    size_t tb = L.tmp_bytes;
    const hipError_t e = rocprim::exclusive_scan(L.tmp, tb, L.cnt, L.pre, 0u, nw, rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return fail(GSR_ERR_DEVICE, std::string(who) + ": scan: " + hipGetErrorString(e));
    hipLaunchKernelGGL(merge_list_kernel, dim3(blocks), dim3(256), 0, s, Ps, L.mask, L.cnt, L.pre, L.list, count);
    return launched(who);
}

int gsr_scaffold_merge_write(int64_t Ps, int64_t K, const float *s_xyz, const float *s_shs, const float *s_opacity,
                             const float *s_scaling, const float *s_rotation, int64_t Pc, int M, const float *c_xyz,
                             const float *c_features, const float *c_opacity, const float *c_scaling,
                             const float *c_rotation, float *xyz, float *features, float *opacity_raw,
                             float *scaling_raw, float *rotation, const void *scratch, void *stream) {
    const char *who = "gsr_scaffold_merge_write";
    if (Ps < 0 || Ps >= (1LL << 31) || K < 0 || K > Ps || Pc < 0 || K + Pc >= (1LL << 31) || M < 4 || M > 16)
        return fail(GSR_ERR_INVALID_ARGUMENT,
                    std::string(who) + ": bad sizes (0 <= K <= Ps < 2^31, Pc >= 0, K + Pc < 2^31, 4 <= M <= 16)");
    if (!scratch || (K > 0 && (!s_xyz || !s_shs || !s_opacity || !s_scaling || !s_rotation)) ||
        (Pc > 0 && (!c_xyz || !c_features || !c_opacity || !c_scaling || !c_rotation)) ||
        (K + Pc > 0 && (!xyz || !features || !opacity_raw || !scaling_raw || !rotation)))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL pointer");
    if (K + Pc == 0) return GSR_OK;
    const MergeLayout L = merge_layout(const_cast<char *>(static_cast<const char *>(scratch)), Ps);
    const int W = 3 * M;
    const MergeRows sc{s_xyz, s_shs, s_opacity, s_scaling, s_rotation};
    const MergeRows ch{c_xyz, c_features, c_opacity, c_scaling, c_rotation};
    const MergeOut out{xyz, features, opacity_raw, scaling_raw, rotation};
    hipLaunchKernelGGL(merge_write_kernel, dim3((unsigned)(((K + Pc) * W + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), Ps, K, Pc, W, sc, ch, L.list, out);
    return launched(who);
}

}  // extern "C"
