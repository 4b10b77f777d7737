// optim.hip -- the Gaussian side of one train_single.py iteration (8(f)
// row 2): the work over rows around the rasterizer -- the parameter activations and their
// backward, the densification statistics, the scale shrink and the fused sparse Adam step over all
// six Gaussian parameter groups.  The image side (pixels) is loss.hip.
//
// Adam.  OurAdam (scene/OurAdam.py:249-337) gathers the `relevant` rows of every group,
// updates them and scatters them back, one torch op at a time, after a host-synchronising
// nonzero().  Here one launch walks all six groups' (param, grad, m, v) arrays once, testing
// relevance (opacity grad != 0) per row on the device.
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>

#include "../../include/gsr.h"
#include "../../include/gsr_train.h"
#include "gsr_adam.h"
#include "gsr_launch.h"

namespace gsr {
namespace {

// ---------------------------------------------------------------------------------------------
// Sparse Adam.


struct AdamArgs {
    gsr_adam_group g[kMaxGroups];
    int64_t block_start[kMaxGroups + 1];
    int n;
};

__global__ __launch_bounds__(256) void any_nonzero_kernel(const float *__restrict__ v, int64_t n,
                                                          int *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool nz = i < n && v[i] != 0.f;
    if (__ballot(nz) != 0 && (threadIdx.x & 63) == 0) *flag = 1;
}

template <int Wd>
__device__ __forceinline__ int64_t row_of(int64_t e, int64_t w) {
    return Wd > 0 ? e / Wd : e / w;
}

template <int Wd>
__device__ __forceinline__ void adam_element(const gsr_adam_group &G, int64_t e, const float *rel, bool dense,
                                             float b1, float b2, float omb1, float omb2, float eps) {
    const int64_t row = row_of<Wd>(e, G.width);
    if (!dense && rel[row] == 0.f) return;
    // element e of the group's (P, width) block sits at row * row_stride + col of its arrays
    const int64_t width = Wd > 0 ? Wd : G.width;
    e += row * (G.row_stride - width);
    const float g = G.grad[e];
    // scene/OurAdam.py:297-324: exp_avg.mul_(b1).add_(g, alpha=1-b1);
    // exp_avg_sq.mul_(b2).addcmul_(g, g, value=1-b2); denom = sqrt(v)/bc2_sqrt + eps;
    // param.addcdiv_(exp_avg, denom, value=-step_size)
    const float m = G.exp_avg[e] * b1 + omb1 * g;
    const float v = G.exp_avg_sq[e] * b2 + omb2 * (g * g);
    const float denom = sqrtf(v) / G.bias_correction2_sqrt + eps;
    G.exp_avg[e] = m;
    G.exp_avg_sq[e] = v;
    G.param[e] = G.param[e] + (-G.step_size) * (m / denom);
}

__global__ __launch_bounds__(kAdamThreads) void sparse_adam_kernel(AdamArgs a, const float *__restrict__ rel,
                                                                   int64_t P, float b1, float b2, float omb1,
                                                                   float omb2, float eps,
                                                                   const int *__restrict__ flag) {
    int gi = 0;
    while (gi + 1 < a.n && (int64_t)blockIdx.x >= a.block_start[gi + 1]) gi++;
    const gsr_adam_group &G = a.g[gi];
    const int64_t e = ((int64_t)blockIdx.x - a.block_start[gi]) * kAdamThreads + threadIdx.x;
    if (e >= P * G.width) return;
    const bool dense = flag == nullptr || *flag == 0;  // no relevance given, or no relevant row
    switch (G.width) {
        case 1: adam_element<1>(G, e, rel, dense, b1, b2, omb1, omb2, eps); break;
        case 3: adam_element<3>(G, e, rel, dense, b1, b2, omb1, omb2, eps); break;
        case 4: adam_element<4>(G, e, rel, dense, b1, b2, omb1, omb2, eps); break;
        case 45: adam_element<45>(G, e, rel, dense, b1, b2, omb1, omb2, eps); break;
        default: adam_element<0>(G, e, rel, dense, b1, b2, omb1, omb2, eps); break;
    }
}

// Row-block form: one wave per 64 consecutive rows.  The relevance of the 64 rows is one
// coalesced load and a ballot; a block of irrelevant rows costs nothing more.  Narrow groups
// (xyz, opacity, scaling, rotation, f_dc) are updated lane = row; a wide group (f_rest) row by
// relevant row, lanes across its columns (one contiguous 180-B segment per row).  The per-element
// arithmetic is adam_element's, so the result is bit-identical to sparse_adam_kernel's; the
// element-per-thread form launched P x 59 threads that mostly only read rel[row].
constexpr int kAdamNarrow = 8;
// The native step's scale shrink (shrink_scales_kernel's arithmetic), applied by the lane that
// owns the row after its Adam update: s_raw NULL = none.
struct ShrinkArgs {
    float *s_raw;
    int64_t first;
    float limit;
};
// Sparse gradient rows (the native step): in the dense fallback (no relevant row) a row takes a
// zero gradient when the rasterizer backward did not write it (live3[3 row + 2] == 0) or when it is
// a locked skybox row (train_single.py:217-223 zeroes its six gradients).  live3 NULL: every row
// is read.
struct DenseRows {
    const float *live3;
    int64_t skybox;
};

// One wave per (64 consecutive rows, group): blockIdx.y is the group, so the groups' updates run
// in parallel waves instead of one after the other in one wave (each group's loads were a
// dependent round trip behind the previous group's stores).  Every element's loads are issued
// before its stores in program order (the arrays may alias as far as the compiler knows), so a
// lane's loads are in flight together.  The scale shrink runs in the wave that updates the
// scaling group (sh_group; -1: group 0's wave, no group writes the scales).
template <int kW>
__device__ __forceinline__ void adam_narrow(const gsr_adam_group &G, int64_t base, bool z, float b1, float b2,
                                            float omb1, float omb2, float eps) {
    float g[kW], m[kW], v[kW], p[kW];
#pragma unroll
    for (int c = 0; c < kW; c++) {
        g[c] = z ? 0.f : G.grad[base + c];
        m[c] = G.exp_avg[base + c];
        v[c] = G.exp_avg_sq[base + c];
        p[c] = G.param[base + c];
    }
#pragma unroll
    for (int c = 0; c < kW; c++) {
        const float mm = m[c] * b1 + omb1 * g[c];
        const float vv = v[c] * b2 + omb2 * (g[c] * g[c]);
        const float denom = sqrtf(vv) / G.bias_correction2_sqrt + eps;
        G.exp_avg[base + c] = mm;
        G.exp_avg_sq[base + c] = vv;
        G.param[base + c] = p[c] + (-G.step_size) * (mm / denom);
    }
}

__global__ __launch_bounds__(kAdamThreads) void sparse_adam_rows_kernel(AdamArgs a, const float *__restrict__ rel,
                                                                        int64_t P, float b1, float b2, float omb1,
                                                                        float omb2, float eps,
                                                                        const int *__restrict__ flag, ShrinkArgs sh,
                                                                        DenseRows dr, int sh_group) {
    __shared__ uint8_t s_idx[kAdamThreads / 64][64];  // the wave's relevant rows, compacted
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r0 = (((int64_t)blockIdx.x * kAdamThreads + threadIdx.x) >> 6) * 64;
    if (r0 >= P) return;  // wave-uniform
    const int gi = (int)blockIdx.y;
    const gsr_adam_group &G = a.g[gi];
    const int64_t row = r0 + lane;
    const bool dense = flag == nullptr || *flag == 0;  // no relevance given, or no relevant row
    const bool relv = row < P && (dense || rel[row] != 0.f);
    const uint64_t mask = __ballot(relv);
    // dense fallback over sparse rows: rows whose gradient reads as zero
    const bool zrow = dense && row < P && (row < dr.skybox || (dr.live3 && dr.live3[3 * row + 2] == 0.f));
    const uint64_t zmask = __ballot(zrow);
    const int w = G.width;
    const int64_t rs = G.row_stride;
    if (mask != 0) {
        if (w <= kAdamNarrow) {
            if (relv) {
                const int64_t base = row * rs;
                switch (w) {
                    case 1: adam_narrow<1>(G, base, zrow, b1, b2, omb1, omb2, eps); break;
                    case 3: adam_narrow<3>(G, base, zrow, b1, b2, omb1, omb2, eps); break;
                    case 4: adam_narrow<4>(G, base, zrow, b1, b2, omb1, omb2, eps); break;
                    default:
                        for (int c = 0; c < w; c++) adam_narrow<1>(G, base + c, zrow, b1, b2, omb1, omb2, eps);
                        break;
                }
            }
        } else {
            // wide group: the relevant rows' elements flattened over the lanes (element e of the
            // wave's n rows: row slot e / w, column e % w), two per lane per trip with both loads
            // issued first
            if (relv) s_idx[wv][__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u))] = (uint8_t)lane;
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            const int tot = __popcll(mask) * w;
            for (int e0 = 0; e0 < tot; e0 += 128) {
                int64_t off[2];
                bool ok[2];
                float g[2], m[2], v[2], p[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int e = e0 + 64 * h + lane;
                    ok[h] = e < tot;
                    const int slot = ok[h] ? e / w : 0;
                    const int rl = s_idx[wv][slot];
                    off[h] = (r0 + rl) * rs + (e - slot * w);
                    const bool z = (zmask >> rl) & 1ull;
                    if (ok[h]) {
                        g[h] = z ? 0.f : G.grad[off[h]];
                        m[h] = G.exp_avg[off[h]];
                        v[h] = G.exp_avg_sq[off[h]];
                        p[h] = G.param[off[h]];
                    }
                }
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    if (!ok[h]) continue;
                    const float mm = m[h] * b1 + omb1 * g[h];
                    const float vv = v[h] * b2 + omb2 * (g[h] * g[h]);
                    const float denom = sqrtf(vv) / G.bias_correction2_sqrt + eps;
                    G.exp_avg[off[h]] = mm;
                    G.exp_avg_sq[off[h]] = vv;
                    G.param[off[h]] = p[h] + (-G.step_size) * (mm / denom);
                }
            }
        }
    }
    if (gi == (sh_group < 0 ? 0 : sh_group) && sh.s_raw && row >= sh.first && row < P) {
        float *sr = sh.s_raw + 3 * row;
        const float x = expf(sr[0]), y = expf(sr[1]), z = expf(sr[2]);
        if (fmaxf(fmaxf(x, y), z) > sh.limit) {
            sr[0] = logf(x * 0.8f);
            sr[1] = logf(y * 0.8f);
            sr[2] = logf(z * 0.8f);
        }
    }
}

// The dense step over whole rows (no relevance, no zero rows, no fused shrink: torch.optim.Adam's
// update of every element, train_post's optimizer): each group is one flat run of P * row_stride
// floats, streamed as float4.  A column-split pair (the DC and rest SH blocks of one buffer, each
// with its own learning rate) is merged on the host into one run whose step size switches at
// split_col, so the buffer is read once in full rows instead of twice in strided blocks.  Same
// arithmetic as adam_narrow, element for element.
// FlatAdamRun, FlatAdamArgs and flat_adam_one (the per-element arithmetic): gsr_adam.h, shared with
// post_step.hip's row-state kernel.
__global__ __launch_bounds__(kAdamThreads) void dense_adam_flat_kernel(FlatAdamArgs a, float b1, float b2, float omb1,
                                                                       float omb2, float eps) {
    int k = 0;
    while (k + 1 < a.n && (int64_t)blockIdx.x >= a.block_start[k + 1]) k++;
    const FlatAdamRun &R = a.r[k];
    const int64_t b0 = ((int64_t)blockIdx.x - a.block_start[k]) * kFlatPerBlock;
    if (R.vec) {
        float4 g[2], m[2], v[2], p[2];
        bool ok[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int64_t e = b0 + (int64_t)h * (kAdamThreads * 4) + 4 * threadIdx.x;
            ok[h] = e < R.n;  // n is a multiple of 4 (row % 4 == 0)
            if (ok[h]) {
                g[h] = *reinterpret_cast<const float4 *>(R.grad + e);
                m[h] = *reinterpret_cast<const float4 *>(R.exp_avg + e);
                v[h] = *reinterpret_cast<const float4 *>(R.exp_avg_sq + e);
                p[h] = *reinterpret_cast<const float4 *>(R.param + e);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (!ok[h]) continue;
            const int64_t e = b0 + (int64_t)h * (kAdamThreads * 4) + 4 * threadIdx.x;
            // the four share a row (row % 4 == 0); one step size: no column needed
            const int c = R.split_col < R.row ? (int)(e % R.row) : 0;
            float ss[4];
#pragma unroll
            for (int j = 0; j < 4; j++) ss[j] = c + j < R.split_col ? R.step0 : R.step1;
            flat_adam_one(R, p[h].x, m[h].x, v[h].x, g[h].x, ss[0], b1, b2, omb1, omb2, eps);
            flat_adam_one(R, p[h].y, m[h].y, v[h].y, g[h].y, ss[1], b1, b2, omb1, omb2, eps);
            flat_adam_one(R, p[h].z, m[h].z, v[h].z, g[h].z, ss[2], b1, b2, omb1, omb2, eps);
            flat_adam_one(R, p[h].w, m[h].w, v[h].w, g[h].w, ss[3], b1, b2, omb1, omb2, eps);
            *reinterpret_cast<float4 *>(R.exp_avg + e) = m[h];
            *reinterpret_cast<float4 *>(R.exp_avg_sq + e) = v[h];
            *reinterpret_cast<float4 *>(R.param + e) = p[h];
        }
    } else {
#pragma unroll
        for (int j = 0; j < kFlatPerThread; j++) {
            const int64_t e = b0 + (int64_t)j * kAdamThreads + threadIdx.x;
            if (e >= R.n) break;
            float p = R.param[e], m = R.exp_avg[e], v = R.exp_avg_sq[e];
            const float ss = (int)(e % R.row) < R.split_col ? R.step0 : R.step1;
            flat_adam_one(R, p, m, v, R.grad[e], ss, b1, b2, omb1, omb2, eps);
            R.exp_avg[e] = m;
            R.exp_avg_sq[e] = v;
            R.param[e] = p;
        }
    }
}

// Builds the flat runs of a dense step.  A group that is a column block not pairing with its
// neighbour into whole rows is left for the row-block kernel: its index goes to rest[].  Returns
// the number of flat runs.
}  // namespace
int flat_adam_runs(int n_groups, const gsr_adam_group *groups, int64_t P, FlatAdamArgs &fa, int *rest,
                   int &n_rest) {
    std::memset(&fa, 0, sizeof(fa));
    n_rest = 0;
    int64_t blocks = 0;
    for (int i = 0; i < n_groups; i++) {
        const gsr_adam_group &g = groups[i];
        const int64_t rs = g.row_stride == 0 ? g.width : g.row_stride;
        FlatAdamRun r;
        std::memset(&r, 0, sizeof(r));
        r.param = g.param;
        r.grad = g.grad;
        r.exp_avg = g.exp_avg;
        r.exp_avg_sq = g.exp_avg_sq;
        r.step0 = r.step1 = g.step_size;
        r.bc2s = g.bias_correction2_sqrt;
        r.split_col = (int)rs;
        if (rs > 0x7fffffff) {
            rest[n_rest++] = i;
            continue;
        }
        if (rs != g.width) {
            const gsr_adam_group *h = i + 1 < n_groups ? &groups[i + 1] : nullptr;
            const int64_t hs = h ? (h->row_stride == 0 ? h->width : h->row_stride) : 0;
            if (!h || hs != rs || g.width + h->width != rs || h->param != g.param + g.width ||
                h->grad != g.grad + g.width || h->exp_avg != g.exp_avg + g.width ||
                h->exp_avg_sq != g.exp_avg_sq + g.width || h->bias_correction2_sqrt != g.bias_correction2_sqrt) {
                rest[n_rest++] = i;
                continue;
            }
            r.split_col = (int)g.width;
            r.step1 = h->step_size;
            i++;
        }
        r.row = (int)rs;
        r.n = P * rs;
        const uintptr_t al = reinterpret_cast<uintptr_t>(r.param) | reinterpret_cast<uintptr_t>(r.grad) |
                             reinterpret_cast<uintptr_t>(r.exp_avg) | reinterpret_cast<uintptr_t>(r.exp_avg_sq);
        r.vec = (al & 15) == 0 && rs % 4 == 0;
        fa.r[fa.n] = r;
        fa.block_start[fa.n] = blocks;
        blocks += (r.n + kFlatPerBlock - 1) / kFlatPerBlock;
        fa.n++;
    }
    fa.block_start[fa.n] = blocks;
    return fa.n;
}
namespace {

// The relevant rows compacted first (sparse steps: OurAdam's `relevant` rows, train_single.py:226).
// The row-block kernel above launches a wave per (64 rows, group) -- P / 64 x groups waves, most of
// which (88% of the rows are irrelevant late in a street chunk) only read 64 flags and leave -- and
// updates a relevant row's narrow groups lane = row, one 64-B line per few useful bytes.  Here:
//   adam_compact_kernel  a grid-stride pass over the flags: each wave's relevant rows appended to a
//                        list (one atomic per wave; Adam's rows are independent, so the order is
//                        free), and the scale shrink of the rows no update touches;
//   adam_rowlist_kernel  one wave per listed row (grid-stride): lane l updates element l of the
//                        row's groups concatenated (59 at SH degree 3: xyz 3, f_dc 3, f_rest 45,
//                        opacity 1, scaling 3, rotation 4), so the SH pair's 48 floats are ONE
//                        192-B contiguous access per array, then the shrink of the row's scales.
// With no relevant row (the dense fallback, OurAdam.py:214) the list pass is skipped and the row
// kernel walks every row (the sparse-rows zero gradients of DenseRows applied).  Same per-element
// arithmetic as adam_narrow (bits unchanged).  gsr_set_adam_kernel(1): the row-block kernel instead.
constexpr int kAdamListMaxLanes = 64;
__device__ __forceinline__ uint32_t lane_prefix_u64(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
struct AdamLaneMap {
    uint8_t group[kAdamListMaxLanes], col[kAdamListMaxLanes];
    int lanes;      // elements per row (sum of the group widths)
    int sh_lane0;   // the first of the three scaling lanes (the shrink), -1: none
};

// Workgroup b owns the contiguous rows [b * per, (b + 1) * per): a first walk counts its relevant
// rows (ballots) and shrinks the rows no update touches, ONE atomic reserves the workgroup's run
// of the list, a second walk (the flags again, now cache-hot) writes the rows.  One atomic per
// wave instead (the first version) put ~16K returning atomics on one word per call, which
// saturates at ~88 per us (MI355X_MICROARCH.md, dequeue): 164 us per call at 1M rows.
constexpr int kCompactThreads = 1024;
constexpr int kCompactWaves = kCompactThreads / 64;
constexpr int kCompactMaxBlocks = 256;
__global__ __launch_bounds__(kCompactThreads) void adam_compact_kernel(const float *__restrict__ rel, int64_t P,
                                                                       const int *__restrict__ flag, int *__restrict__ list,
                                                                       int *__restrict__ count, ShrinkArgs sh) {
    if (*flag == 0) return;  // the dense fallback: the row kernel takes every row (and shrinks them)
    __shared__ uint32_t s_wc[kCompactWaves];
    __shared__ int s_base;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t per = ((P + gridDim.x - 1) / gridDim.x + kCompactThreads - 1) / kCompactThreads * kCompactThreads;
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(P, r0 + per);
    uint32_t cnt = 0;
    for (int64_t b = r0 + (int64_t)w * 64; b < r1; b += kCompactThreads) {
        const int64_t row = b + lane;
        const bool relv = row < r1 && rel[row] != 0.f;
        cnt += (uint32_t)__popcll(__ballot(relv));
        if (!relv && sh.s_raw && row >= sh.first && row < r1) {  // rows no update touches: shrunk here
            float *sr = sh.s_raw + 3 * row;
            const float x = expf(sr[0]), y = expf(sr[1]), z = expf(sr[2]);
            if (fmaxf(fmaxf(x, y), z) > sh.limit) {
                sr[0] = logf(x * 0.8f);
                sr[1] = logf(y * 0.8f);
                sr[2] = logf(z * 0.8f);
            }
        }
    }
    if (lane == 0) s_wc[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int k = 0; k < kCompactWaves; k++) tot += s_wc[k];
        s_base = tot ? atomicAdd(count, (int)tot) : 0;
    }
    __syncthreads();
    if (r0 >= r1) return;
    int at = s_base;
    for (int k = 0; k < w; k++) at += (int)s_wc[k];
    for (int64_t b = r0 + (int64_t)w * 64; b < r1; b += kCompactThreads) {
        const int64_t row = b + lane;
        const bool relv = row < r1 && rel[row] != 0.f;
        const uint64_t m = __ballot(relv);
        if (relv) list[at + (int)lane_prefix_u64(m)] = (int)row;
        at += __popcll(m);
    }
}

// Four listed rows per wave and trip: the four rows' list entries, then all their loads, then the
// updates -- one row at a time left each wave a chain of dependent round trips per row (~32 rows per
// resident wave at 3M rows, 8.5% relevant: 140 us per call in the config-3 chunk, r05e).
#ifndef GSR_ADAM_ROWS
#define GSR_ADAM_ROWS 1  // r05i: 4 rows per trip 42.9 / 163.4 us per call (1M / 3M rows), 1 row 38.0 / 161.5 us
#endif
constexpr int kAdamRowsPerTrip = GSR_ADAM_ROWS;
__global__ __launch_bounds__(256) void adam_rowlist_kernel(AdamArgs a, AdamLaneMap lm, const int *__restrict__ list,
                                                           const int *__restrict__ count, int64_t P,
                                                           const int *__restrict__ flag, float b1, float b2, float omb1,
                                                           float omb2, float eps, ShrinkArgs sh, DenseRows dr) {
    constexpr int R = kAdamRowsPerTrip;
    const int lane = threadIdx.x & 63;
    const bool dense = *flag == 0;
    const int64_t n = dense ? P : (int64_t)*count;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const bool act = lane < lm.lanes;
    const gsr_adam_group &G = a.g[act ? lm.group[lane] : 0];
    const int64_t col = act ? lm.col[lane] : 0;
    const bool shrink = sh.s_raw && lm.sh_lane0 >= 0;
    for (int64_t k0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * R; k0 < n; k0 += waves * R) {
        int64_t row[R];
        bool ok[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            ok[r] = k0 + r < n;
            row[r] = !ok[r] ? 0 : dense ? k0 + r : (int64_t)list[k0 + r];
        }
        float g[R], m0[R], v0[R], p0[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            g[r] = m0[r] = v0[r] = p0[r] = 0.f;
            if (act && ok[r]) {
                // the dense fallback over sparse rows: rows whose gradient reads as zero
                const bool z = dense && (row[r] < dr.skybox || (dr.live3 && dr.live3[3 * row[r] + 2] == 0.f));
                const int64_t e = row[r] * G.row_stride + col;
                g[r] = z ? 0.f : G.grad[e];
                m0[r] = G.exp_avg[e];
                v0[r] = G.exp_avg_sq[e];
                p0[r] = G.param[e];
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (!ok[r]) break;  // wave-uniform
            float p = 0.f;
            if (act) {
                const int64_t e = row[r] * G.row_stride + col;
                const float mm = m0[r] * b1 + omb1 * g[r];
                const float vv = v0[r] * b2 + omb2 * (g[r] * g[r]);
                const float denom = sqrtf(vv) / G.bias_correction2_sqrt + eps;
                G.exp_avg[e] = mm;
                G.exp_avg_sq[e] = vv;
                p = p0[r] + (-G.step_size) * (mm / denom);
                G.param[e] = p;
            }
            if (shrink && row[r] >= sh.first) {
                // the shrink of the row's freshly updated scales (shrink_scales_kernel's arithmetic)
                const float sx = __shfl(p, lm.sh_lane0, 64), sy = __shfl(p, lm.sh_lane0 + 1, 64),
                            sz = __shfl(p, lm.sh_lane0 + 2, 64);
                const float x = expf(sx), y = expf(sy), zz = expf(sz);
                if (fmaxf(fmaxf(x, y), zz) > sh.limit && lane >= lm.sh_lane0 && lane < lm.sh_lane0 + 3) {
                    const float c = lane == lm.sh_lane0 ? x : lane == lm.sh_lane0 + 1 ? y : zz;
                    sh.s_raw[3 * row[r] + (lane - lm.sh_lane0)] = logf(c * 0.8f);
                }
            }
        }
    }
}

// gsr_set_adam_kernel: 0 = flat runs for a dense step, the compacted row list for a sparse step whose
// row fits one wave, row blocks otherwise; 1 = the row-block kernel for every step; 2 = the
// element-per-thread kernel.  Same bits in every mode (tests/test_gpu_train.py).
enum AdamKernel { kAdamAuto = 0, kAdamRowBlocks = 1, kAdamElementwise = 2 };
std::atomic<int> g_adam_kernel{kAdamAuto};

// add_densification_stats for one visible row (radius r > 0; scene/gaussian_model.py:780-793 and
// train_single.py's max_radii2D update).  accum follows torch.max(norm, accum), which propagates a
// NaN from either side -- a row whose 2-D gradient went NaN keeps a NaN accumulator until
// densify_and_prune zeroes it, so it is neither cloned nor split at the next event; fmaxf would
// return the other operand.  n > a is false for a NaN a, which then stays.
__device__ inline void densify_stats_row(int64_t i, int r, const float *__restrict__ g2d, float *__restrict__ maxr,
                                         float *__restrict__ accum, float *__restrict__ denom) {
    const float gx = g2d[3 * i], gy = g2d[3 * i + 1];
    const float n = sqrtf(gx * gx + gy * gy);
    const float a = accum[i];
    maxr[i] = fmaxf(maxr[i], (float)r);
    accum[i] = (n > a || n != n) ? n : a;
    denom[i] = denom[i] + 1.f;
}

__global__ __launch_bounds__(256) void densify_stats_kernel(int64_t P, const int *__restrict__ radii,
                                                            const float *__restrict__ g2d, float *__restrict__ maxr,
                                                            float *__restrict__ accum, float *__restrict__ denom) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int r = radii[i];
    if (r <= 0) return;
    densify_stats_row(i, r, g2d, maxr, accum, denom);
}

// ---------------------------------------------------------------------------------------------
// Parameter activations (scene/gaussian_model.py:39-47, getters :125-156) and the per-step
// shrink of over-large Gaussians (train_single.py:235-241).  One lane per Gaussian; the
// backward follows torch's autograd formulas (exp: g*y; sigmoid: g*(1-y)*y; normalize =
// x / max(||x||, 1e-12): dx = g/d - x * (sum(g * ((x/d)/d)) / n)).

__global__ __launch_bounds__(256) void activate_fwd_kernel(int64_t P, const float *__restrict__ s_raw,
                                                           const float4 *__restrict__ q_raw,
                                                           const float *__restrict__ o_raw, float *__restrict__ scales,
                                                           float4 *__restrict__ rots, float *__restrict__ opac) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
#pragma unroll
    for (int k = 0; k < 3; k++) scales[3 * i + k] = act_scale(s_raw[3 * i + k]);
    rots[i] = act_rot(q_raw[i]);
    opac[i] = act_opacity(o_raw[i]);
}

__global__ __launch_bounds__(256) void activate_bwd_kernel(int64_t P, const float4 *__restrict__ q_raw,
                                                           const float *__restrict__ scales,
                                                           const float *__restrict__ opac,
                                                           const float *__restrict__ g_s,
                                                           const float4 *__restrict__ g_q,
                                                           const float *__restrict__ g_o, float *__restrict__ d_s,
                                                           float4 *__restrict__ d_q, float *__restrict__ d_o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
#pragma unroll
    for (int k = 0; k < 3; k++) d_s[3 * i + k] = g_s[3 * i + k] * scales[3 * i + k];
    const float4 x = q_raw[i], g = g_q[i];
    const float n = sqrtf(x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w);
    const float d = fmaxf(n, 1e-12f);
    const float gd = -(g.x * ((x.x / d) / d) + g.y * ((x.y / d) / d) + g.z * ((x.z / d) / d) + g.w * ((x.w / d) / d));
    const float gn = n >= 1e-12f && n != 0.f ? gd / n : 0.f;  // clamp_min and norm backward
    d_q[i] = make_float4(g.x / d + x.x * gn, g.y / d + x.y * gn, g.z / d + x.z * gn, g.w / d + x.w * gn);
    const float y = opac[i];
    d_o[i] = g_o[i] * (1.f - y) * y;
}

// The native step's form: also the skybox lock (rows below `skybox` get a zero opacity gradient,
// train_single.py:217-223), the sparse Adam's "any relevant row" flag (zeroed earlier in the step)
// and the densification statistics of the same row (densify_stats_row).
__global__ __launch_bounds__(256) void activate_bwd_step_kernel(
    int64_t P, const float4 *__restrict__ q_raw, const float *__restrict__ g_s, const float4 *__restrict__ g_q,
    const float *__restrict__ g_o, float *__restrict__ d_s, float4 *__restrict__ d_q, float *__restrict__ d_o,
    int64_t skybox, int *__restrict__ flag, const int *__restrict__ radii, const float *__restrict__ g2d,
    float *__restrict__ maxr, float *__restrict__ accum, float *__restrict__ denom, int sparse_rows,
    const float *__restrict__ s_raw, const float *__restrict__ o_raw) {
    // the rasterizer read the pre-activation parameters: the activations are recomputed here from
    // s_raw / o_raw, with the forward's expressions
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float go = 0.f;
    if (i < P) {
        const int r = radii[i];
        // sparse rows: only the rows the rasterizer backward wrote (liveness in g2d's third column;
        // invisible rows never are) have scale / rotation gradients -- the others are never relevant
        bool live = !sparse_rows;
        if (r > 0) {
            if (sparse_rows) live = g2d[3 * i + 2] != 0.f;
            densify_stats_row(i, r, g2d, maxr, accum, denom);
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < 3; k++) d_s[3 * i + k] = g_s[3 * i + k] * act_scale(s_raw[3 * i + k]);
            const float4 x = q_raw[i], g = g_q[i];
            const float n = sqrtf(x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w);
            const float d = fmaxf(n, 1e-12f);
            const float gd =
                -(g.x * ((x.x / d) / d) + g.y * ((x.y / d) / d) + g.z * ((x.z / d) / d) + g.w * ((x.w / d) / d));
            const float gn = n >= 1e-12f && n != 0.f ? gd / n : 0.f;
            d_q[i] = make_float4(g.x / d + x.x * gn, g.y / d + x.y * gn, g.z / d + x.z * gn, g.w / d + x.w * gn);
        }
        const float y = act_opacity(o_raw[i]);
        go = i < skybox ? 0.f : g_o[i] * (1.f - y) * y;
        d_o[i] = go;
    }
    if (__ballot(go != 0.f) != 0 && (threadIdx.x & 63) == 0) *flag = 1;
}

__global__ __launch_bounds__(256) void shrink_scales_kernel(int64_t P, int64_t first, float *__restrict__ s_raw,
                                                            float limit) {
    const int64_t i = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const float a = expf(s_raw[3 * i]), b = expf(s_raw[3 * i + 1]), c = expf(s_raw[3 * i + 2]);
    if (fmaxf(fmaxf(a, b), c) > limit) {
        s_raw[3 * i] = logf(a * 0.8f);
        s_raw[3 * i + 1] = logf(b * 0.8f);
        s_raw[3 * i + 2] = logf(c * 0.8f);
    }
}

}  // namespace

// opts.flag_ready: *flag_scratch already holds "some row is relevant" (the native step's
// activate_bwd_step_kernel computed it), so the any_nonzero pass is skipped.
int sparse_adam(int n_groups, const gsr_adam_group *groups, int64_t P, const float *relevance, int *flag_scratch,
                const AdamHyper &hyper, const SparseAdamOpts &opts, hipStream_t s) {
    float *const shrink_raw = opts.shrink_raw;
    const float *const live3 = opts.live3;
    const ShrinkArgs sha{shrink_raw, opts.shrink_first, opts.shrink_limit};
    const DenseRows rows{live3, opts.skybox};
    // torch applies python-float hyper-parameters as fp32 scalars: b, (1 - b) rounded from double
    const float b1 = (float)hyper.beta1, b2 = (float)hyper.beta2, eps = (float)hyper.eps;
    const float omb1 = (float)(1.0 - hyper.beta1), omb2 = (float)(1.0 - hyper.beta2);
    const int kernel = g_adam_kernel.load(std::memory_order_relaxed);  // read once: one choice per call
    if ((shrink_raw || live3) && kernel == kAdamElementwise) {
        set_last_error("sparse Adam: the fused scale shrink / sparse rows need the row-block kernel");
        return GSR_ERR_UNSUPPORTED;
    }
    if (n_groups < 0 || n_groups > kMaxGroups || P < 0 || (P > 0 && (!groups || (relevance && !flag_scratch)))) {
        set_last_error("gsr_sparse_adam_step: bad group count or NULL pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0 || n_groups == 0) return GSR_OK;
    AdamArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = n_groups;
    int64_t blocks = 0;
    for (int i = 0; i < n_groups; i++) {
        const gsr_adam_group &g = groups[i];
        if (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq || g.width <= 0 ||
            (g.row_stride != 0 && g.row_stride < g.width)) {
            set_last_error("gsr_sparse_adam_step: group has a NULL array, non-positive width or row_stride < width");
            return GSR_ERR_INVALID_ARGUMENT;
        }
        a.g[i] = g;
        if (a.g[i].row_stride == 0) a.g[i].row_stride = g.width;
        a.block_start[i] = blocks;
        blocks += (P * g.width + kAdamThreads - 1) / kAdamThreads;
    }
    a.block_start[n_groups] = blocks;
    if (blocks > 0x7fffffff) {
        set_last_error("gsr_sparse_adam_step: parameter set too large for one launch");
        return GSR_ERR_UNSUPPORTED;
    }
    // relevance NULL: a dense step (torch.optim.Adam over every row), one launch
    int *flag = relevance ? flag_scratch : nullptr;
    if (relevance && !opts.flag_ready) {
        (void)hipMemsetAsync(flag_scratch, 0, sizeof(int), s);
        hipLaunchKernelGGL(any_nonzero_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, relevance, P,
                           flag_scratch);
    }
    if (!relevance && !live3 && opts.skybox == 0 && !shrink_raw && kernel == kAdamAuto) {
        // the dense step: flat runs, and the row-block kernel for any group that is not one
        FlatAdamArgs fa;
        int rest[kMaxGroups], n_rest = 0;
        if (flat_adam_runs(n_groups, groups, P, fa, rest, n_rest) > 0)
            hipLaunchKernelGGL(dense_adam_flat_kernel, dim3((unsigned)fa.block_start[fa.n]), dim3(kAdamThreads), 0, s,
                               fa, b1, b2, omb1, omb2, eps);
        if (n_rest > 0) {
            AdamArgs ar;
            std::memset(&ar, 0, sizeof(ar));
            ar.n = n_rest;
            for (int j = 0; j < n_rest; j++) ar.g[j] = a.g[rest[j]];
            hipLaunchKernelGGL(sparse_adam_rows_kernel,
                               dim3((unsigned)((P + kAdamThreads - 1) / kAdamThreads), (unsigned)n_rest),
                               dim3(kAdamThreads), 0, s, ar, relevance, P, b1, b2, omb1, omb2, eps,
                               (const int *)nullptr, ShrinkArgs{nullptr, 0, 0.f}, DenseRows{nullptr, 0}, -1);
        }
    }
    else if (kernel != kAdamElementwise)
    {
        // the shrink reads the scales after their Adam update: it runs in the scaling group's wave
        int sh_group = -1;
        for (int i = 0; i < n_groups; i++)
            if (shrink_raw && groups[i].param == shrink_raw) sh_group = i;
        // the compacted form when the row's elements fit one wave (and the shrink, if any, has its
        // three scale lanes)
        AdamLaneMap lm;
        std::memset(&lm, 0, sizeof(lm));
        lm.sh_lane0 = -1;
        bool fits = relevance != nullptr && kernel == kAdamAuto &&
                    (!shrink_raw || (sh_group >= 0 && groups[sh_group].width == 3));
        for (int i = 0; fits && i < n_groups; i++) {
            if (lm.lanes + groups[i].width > kAdamListMaxLanes) {
                fits = false;
                break;
            }
            if (i == sh_group) lm.sh_lane0 = lm.lanes;
            for (int c = 0; c < (int)groups[i].width; c++) {
                lm.group[lm.lanes] = (uint8_t)i;
                lm.col[lm.lanes++] = (uint8_t)c;
            }
        }
        // the row list and its counter: the caller's scratch, or stream-ordered scratch of this call;
        // if that allocation fails the row-block kernel (which needs none) runs instead
        int *buf = opts.row_list;
        bool own = false;
        if (fits && P <= 0x7fffffff && !buf) {
            if (hipMallocAsync(reinterpret_cast<void **>(&buf), sizeof(int) * ((size_t)P + 64), s) == hipSuccess) own = true;
            else {
                (void)hipGetLastError();
                buf = nullptr;
            }
        }
        if (fits && P <= 0x7fffffff && buf) {
            int *count = buf, *list = buf + 64;
            (void)hipMemsetAsync(count, 0, sizeof(int), s);
            const unsigned cb = (unsigned)std::max<int64_t>(
                1, std::min<int64_t>((P + kCompactThreads - 1) / kCompactThreads, kCompactMaxBlocks));
            hipLaunchKernelGGL(adam_compact_kernel, dim3(cb), dim3(kCompactThreads), 0, s, relevance, P, flag, list,
                               count, sha);
            hipLaunchKernelGGL(adam_rowlist_kernel, dim3(4096), dim3(256), 0, s, a, lm, (const int *)list,
                               (const int *)count, P, flag, b1, b2, omb1, omb2, eps, sha, rows);
            if (own) (void)hipFreeAsync(buf, s);
        } else
            hipLaunchKernelGGL(sparse_adam_rows_kernel,
                               dim3((unsigned)((P + kAdamThreads - 1) / kAdamThreads), (unsigned)n_groups),
                               dim3(kAdamThreads), 0, s, a, relevance, P, b1, b2, omb1, omb2, eps, flag, sha, rows,
                               sh_group);
    }
    else
        hipLaunchKernelGGL(sparse_adam_kernel, dim3((unsigned)blocks), dim3(kAdamThreads), 0, s, a, relevance, P, b1,
                           b2, omb1, omb2, eps, flag);
    return launched("gsr_sparse_adam_step");
}

int step_activate_backward(int64_t P, const StepAct &act, const ActGrads &g, hipStream_t s) {
    hipLaunchKernelGGL(activate_bwd_step_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, act.q_raw,
                       g.d_scales, reinterpret_cast<const float4 *>(g.d_rots), g.d_opac, g.scaling_grad,
                       reinterpret_cast<float4 *>(g.rotation_grad), g.opacity_grad, act.skybox, act.flag, act.radii,
                       g.d_means2D, act.maxr, act.accum, act.denom, g.sparse_rows ? 1 : 0, act.s_raw, act.o_raw);
    return launched("step activation backward");
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_set_adam_kernel(int kernel) {
    if (kernel < kAdamAuto || kernel > kAdamElementwise) {
        set_last_error("gsr_set_adam_kernel: kernel 0 (default choice), 1 (row blocks) or 2 (element per thread)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return g_adam_kernel.exchange(kernel);
}

int gsr_sparse_adam_step(int n_groups, const gsr_adam_group *groups, int64_t P, const float *relevance,
                         double beta1, double beta2, double eps, int *flag_scratch, void *stream) {
    return sparse_adam(n_groups, groups, P, relevance, flag_scratch, AdamHyper{beta1, beta2, eps}, SparseAdamOpts{},
                       static_cast<hipStream_t>(stream));
}

int gsr_densify_stats(int64_t P, const int *radii, const float *dL_dmeans2D, float *max_radii2D, float *grad_accum,
                      float *denom, void *stream) {
    if (P < 0 || (P > 0 && (!radii || !dL_dmeans2D || !max_radii2D || !grad_accum || !denom))) {
        set_last_error("gsr_densify_stats: NULL pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return GSR_OK;
    hipLaunchKernelGGL(densify_stats_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), P, radii, dL_dmeans2D, max_radii2D, grad_accum, denom);
    return launched("gsr_densify_stats");
}

int gsr_activate_forward(int64_t P, const float *scaling_raw, const float *rotation_raw, const float *opacity_raw,
                         float *scales, float *rotations, float *opacities, void *stream) {
    if (P < 0 || (P > 0 && (!scaling_raw || !rotation_raw || !opacity_raw || !scales || !rotations || !opacities)) ||
        (P > 0 && ((reinterpret_cast<uintptr_t>(rotation_raw) | reinterpret_cast<uintptr_t>(rotations)) & 15))) {
        set_last_error("gsr_activate_forward: NULL or misaligned (rotations need 16 B) pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return GSR_OK;
    hipLaunchKernelGGL(activate_fwd_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), P, scaling_raw,
                       reinterpret_cast<const float4 *>(rotation_raw), opacity_raw, scales,
                       reinterpret_cast<float4 *>(rotations), opacities);
    return launched("gsr_activate_forward");
}

int gsr_activate_backward(int64_t P, const float *rotation_raw, const float *scales, const float *opacities,
                          const float *dL_dscales, const float *dL_drotations, const float *dL_dopacities,
                          float *dL_dscaling_raw, float *dL_drotation_raw, float *dL_dopacity_raw, void *stream) {
    if (P < 0 || (P > 0 && (!rotation_raw || !scales || !opacities || !dL_dscales || !dL_drotations ||
                            !dL_dopacities || !dL_dscaling_raw || !dL_drotation_raw || !dL_dopacity_raw)) ||
        (P > 0 && ((reinterpret_cast<uintptr_t>(rotation_raw) | reinterpret_cast<uintptr_t>(dL_drotations) |
                    reinterpret_cast<uintptr_t>(dL_drotation_raw)) & 15))) {
        set_last_error("gsr_activate_backward: NULL or misaligned (rotations need 16 B) pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return GSR_OK;
    hipLaunchKernelGGL(activate_bwd_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), P, reinterpret_cast<const float4 *>(rotation_raw), scales,
                       opacities, dL_dscales, reinterpret_cast<const float4 *>(dL_drotations), dL_dopacities,
                       dL_dscaling_raw, reinterpret_cast<float4 *>(dL_drotation_raw), dL_dopacity_raw);
    return launched("gsr_activate_backward");
}

int gsr_shrink_scales(int64_t P, int64_t first_row, float *scaling_raw, float max_scale, void *stream) {
    if (P < 0 || first_row < 0 || (P > 0 && !scaling_raw)) {
        set_last_error("gsr_shrink_scales: bad sizes or NULL pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (first_row >= P) return GSR_OK;
    const int64_t n = P - first_row;
    hipLaunchKernelGGL(shrink_scales_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), P, first_row, scaling_raw, max_scale);
    return launched("gsr_shrink_scales");
}

}  // extern "C"
