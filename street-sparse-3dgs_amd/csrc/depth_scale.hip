// depth_scale.hip -- the depth scale fit: per image the (scale, offset) that takes a 16-bit inverse depth
// map of unknown scale onto the inverse depths of the sparse points the image observes
// (include/gsr_depth_scale.h).
//
// One launch for the batch, one 256-thread workgroup per camera, three passes over the camera's segment:
//   gather   256 observations a turn, coalesced ids and positions (through obs_index when given):
//            id -> row -> point, z and inv in fp64, the map position in fp32, the validity tests, one
//            bilinear sample; min / max / NaN of the masked inv in registers; the valid (inv, v) pairs
//            compacted in observation order by a ballot per wave and a scan of the four wave counts
//   select   the one or two middle elements of inv (64-bit keys) and of v (32-bit keys): a radix select,
//            8 bits a round over the values' own bit patterns (all > 0 or >= 0, so they order as unsigned
//            integers), 256 LDS bins, the round's bin found by a block scan; for an even count the
//            upper middle is the lower one again or the smallest key above it (one counting round)
//   sums     |inv - t_colmap| and fl32(|v - t_mono|) in fp64: each thread its strided elements in
//            order, a shuffle tree per wave, the four waves in order
// A segment of up to kCap observations keeps its pairs in LDS (48 KiB: three workgroups per CU); a longer
// one keeps them in the scratch, reached through the same generic pointers by the same code.
// No atomic decides an order and no float is added by an atomic: reruns are bitwise equal.
#include <cmath>
#include <string>

#include "../../include/gsr.h"
#include "../../include/gsr_depth_scale.h"
#include "gsr_launch.h"

namespace gsr {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCap = 4096;  // 4096 x (8 + 4) B = 48 KiB of the 160: three workgroups (12 waves) per CU

struct FitArgs {
    const double *cams;
    const int64_t *offsets, *index;
    int64_t L, O;
    const double *xy;
    const int64_t *pid;
    int64_t N, T;
    const int32_t *table;
    const double *xyz;
    int64_t K;
    int Hd, Wd;
    const uint16_t *maps;
    int missing;
    double *spill_inv;
    float *spill_v;
    gsr_depth_scale_record *out;
};

struct Shared {
    double inv[kCap];
    float v[kCap];
    uint32_t hist[256];
    uint32_t wsum[2][kWaves];
    double red[3][kWaves];
    unsigned long long min_gt;
    uint32_t cnt_le, digit, rank, nan;
};

// Inclusive sum of c over the workgroup's 256 threads (thread order).  s.wsum[0] is free to use.
__device__ inline uint32_t block_scan_incl(uint32_t c, Shared &s) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) s.wsum[0][w] = x;
    __syncthreads();
    for (int i = 0; i < w; ++i) x += s.wsum[0][i];
    __syncthreads();
    return x;
}

// The key of rank k (0-based, ascending) among keys[0 .. n), k < n.  Every thread returns it.
template <typename K>
__device__ inline K radix_select(const K *keys, int n, uint32_t k, Shared &s) {
    constexpr int kBits = 8 * (int)sizeof(K);
    K prefix = 0;
    for (int shift = kBits - 8; shift >= 0; shift -= 8) {
        s.hist[threadIdx.x] = 0;
        __syncthreads();
        const K high = shift + 8 >= kBits ? (K)0 : (K)(~(K)0 << (shift + 8));
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const K key = keys[i];
            if ((key & high) == prefix) atomicAdd(&s.hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        const uint32_t c = s.hist[threadIdx.x];
        const uint32_t incl = block_scan_incl(c, s), excl = incl - c;
        if (excl <= k && k < incl) {  // exactly one thread: the counts of the prefix's keys sum to more than k
            s.digit = threadIdx.x;
            s.rank = k - excl;
        }
        __syncthreads();
        prefix |= (K)s.digit << shift;
        k = s.rank;
    }
    return prefix;
}

// The key of rank k + 1, given a = the key of rank k (k + 1 < n): a again when more than k + 1 keys are
// <= a, else the smallest key above a.
template <typename K>
__device__ inline K next_rank(const K *keys, int n, uint32_t k, K a, Shared &s) {
    if (threadIdx.x == 0) {
        s.cnt_le = 0;
        s.min_gt = ~0ull;
    }
    __syncthreads();
    uint32_t cnt = 0;
    unsigned long long mn = ~0ull;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const K key = keys[i];
        if (key <= a) {
            ++cnt;
        } else if ((unsigned long long)key < mn) {
            mn = key;
        }
    }
    if (cnt) atomicAdd(&s.cnt_le, cnt);
    if (mn != ~0ull) atomicMin(&s.min_gt, mn);  // a minimum: the order of the atomics does not matter
    __syncthreads();
    const K b = s.cnt_le > k + 1 ? a : (K)s.min_gt;
    __syncthreads();
    return b;
}

// Sum over the workgroup in a fixed order: shuffle tree per wave, then the waves in order.  slot: 0 .. 2.
__device__ inline double block_sum(double x, Shared &s, int slot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    if ((threadIdx.x & 63) == 0) s.red[slot][threadIdx.x >> 6] = x;
    __syncthreads();
    double r = s.red[slot][0];
    for (int i = 1; i < kWaves; ++i) r += s.red[slot][i];
    return r;
}

__global__ __launch_bounds__(kThreads) void depth_scale_fit_kernel(FitArgs a) {
    __shared__ Shared s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t m = blockIdx.x;
    const double *cam = a.cams + GSR_DEPTH_SCALE_CAMERA_DOUBLES * m;
    gsr_depth_scale_record rec{};
    const double dmap = cam[14];
    if (!(dmap >= 0.0 && dmap < (double)a.K)) {
        rec.flags = GSR_DEPTH_SCALE_NO_MAP;
        if (tid == 0) a.out[m] = rec;
        return;
    }
    const uint16_t *map = a.maps + (int64_t)dmap * a.Hd * a.Wd;
    int64_t b = a.offsets[m], e = a.offsets[m + 1];
    b = b < 0 ? 0 : (b > a.L ? a.L : b);
    e = e < b ? b : (e > a.L ? a.L : e);
    const int64_t n = e - b;
    double *const inv_buf = n <= kCap ? s.inv : a.spill_inv + b;
    float *const v_buf = n <= kCap ? s.v : a.spill_v + b;

    const double R20 = cam[6], R21 = cam[7], R22 = cam[8], t2 = cam[11];
    const double sc = (double)a.Hd / cam[13];
    const float bw = (float)(cam[12] * sc), bh = (float)(cam[13] * sc);

    // ---- gather ----
    const double kInf = __builtin_huge_val();
    double lo = kInf, hi = -kInf;
    bool nan_seen = false;
    uint32_t n_valid = 0;
    int turn = 0;
    for (int64_t base = 0; base < n; base += kThreads, turn ^= 1) {
        const int64_t i = base + tid;
        bool valid = false;
        double inv = 0.0;
        float v = 0.f;
        if (i < n) {
            const int64_t o = a.index ? a.index[b + i] : b + i;
            const int64_t q = (o >= 0 && o < a.O) ? a.pid[o] : -1;
            if (q >= 0 && q < a.T) {
                int r = a.table[q];
                if (r >= a.N) r = -1;
                if (r >= 0 || a.missing == 0) {  // masked
                    double X = 0.0, Y = 0.0, Z = 0.0;
                    if (r >= 0) {
                        X = a.xyz[3 * (int64_t)r];
                        Y = a.xyz[3 * (int64_t)r + 1];
                        Z = a.xyz[3 * (int64_t)r + 2];
                    }
                    const double z = ((R20 * X + R21 * Y) + R22 * Z) + t2;
                    inv = 1.0 / z;
                    if (inv != inv) nan_seen = true;
                    if (inv < lo) lo = inv;
                    if (inv > hi) hi = inv;
                    const float mx = (float)(a.xy[2 * o] * sc), my = (float)(a.xy[2 * o + 1] * sc);
                    valid = mx >= 0.f && my >= 0.f && mx < bw && my < bh && inv > 0.0;
                    if (valid) {
                        const float fsx = fminf(rintf(mx * 32.f), 1073741824.f);
                        const float fsy = fminf(rintf(my * 32.f), 1073741824.f);
                        const int sx = (int)fsx, sy = (int)fsy;
                        const int ix = sx >> 5, iy = sy >> 5;
                        const float fx = (float)(sx & 31) * 0.03125f, fy = (float)(sy & 31) * 0.03125f;
                        const int x0 = ix < a.Wd - 1 ? ix : a.Wd - 1, x1 = ix + 1 < a.Wd - 1 ? ix + 1 : a.Wd - 1;
                        const int y0 = iy < a.Hd - 1 ? iy : a.Hd - 1, y1 = iy + 1 < a.Hd - 1 ? iy + 1 : a.Hd - 1;
                        const uint16_t *r0 = map + (int64_t)y0 * a.Wd, *r1 = map + (int64_t)y1 * a.Wd;
                        const float k16 = 1.f / 65536.f;
                        const float S00 = (float)r0[x0] * k16, S01 = (float)r0[x1] * k16;
                        const float S10 = (float)r1[x0] * k16, S11 = (float)r1[x1] * k16;
                        const float w00 = (1.f - fy) * (1.f - fx), w01 = (1.f - fy) * fx;
                        const float w10 = fy * (1.f - fx), w11 = fy * fx;
                        v = ((S00 * w00 + S01 * w01) + S10 * w10) + S11 * w11;
                    }
                }
            }
        }
        const unsigned long long bal = __ballot(valid);
        if (lane == 0) s.wsum[turn][w] = (uint32_t)__popcll(bal);
        __syncthreads();  // one barrier a turn: the two wsum rows alternate
        uint32_t before = 0, all = 0;
        for (int j = 0; j < kWaves; ++j) {
            const uint32_t c = s.wsum[turn][j];
            before += j < w ? c : 0u;
            all += c;
        }
        if (valid) {  // pos < n: at most one valid per observation
            const uint32_t pos = n_valid + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            inv_buf[pos] = inv;
            v_buf[pos] = v;
        }
        n_valid += all;
    }
    if (tid == 0) s.nan = 0;
    __syncthreads();
    // min / max / NaN over the workgroup (order-free)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double x = __shfl_xor(lo, o), y = __shfl_xor(hi, o);
        lo = x < lo ? x : lo;
        hi = y > hi ? y : hi;
    }
    if (__ballot(nan_seen) && lane == 0) atomicOr(&s.nan, 1u);
    if (lane == 0) {
        s.red[0][w] = lo;
        s.red[1][w] = hi;
    }
    __threadfence();  // the spilled pairs of this workgroup, before other threads of it read them
    __syncthreads();
    for (int j = 0; j < kWaves; ++j) {
        lo = s.red[0][j] < lo ? s.red[0][j] : lo;
        hi = s.red[1][j] > hi ? s.red[1][j] : hi;
    }
    const bool any_nan = s.nan != 0;
    __syncthreads();
    rec.n_valid = (int32_t)n_valid;
    if (any_nan) rec.flags |= GSR_DEPTH_SCALE_NAN_SEEN;
    const bool fitted = n_valid > 10u && !any_nan && (hi - lo) > 1e-3;
    if (!fitted) {
        if (tid == 0) a.out[m] = rec;
        return;
    }

    // ---- select ----
    const int nv = (int)n_valid;
    const uint32_t k_lo = (uint32_t)(nv - 1) >> 1;
    const unsigned long long *ikeys = reinterpret_cast<const unsigned long long *>(inv_buf);
    const uint32_t *vkeys = reinterpret_cast<const uint32_t *>(v_buf);
    const unsigned long long ia = radix_select<unsigned long long>(ikeys, nv, k_lo, s);
    const uint32_t va = radix_select<uint32_t>(vkeys, nv, k_lo, s);
    double t_colmap = __longlong_as_double((long long)ia);
    float t_mono = __uint_as_float(va);
    if ((nv & 1) == 0) {
        const unsigned long long ib = next_rank<unsigned long long>(ikeys, nv, k_lo, ia, s);
        const uint32_t vb = next_rank<uint32_t>(vkeys, nv, k_lo, va, s);
        t_colmap = (t_colmap + __longlong_as_double((long long)ib)) / 2.0;
        t_mono = (t_mono + __uint_as_float(vb)) / 2.f;
    }

    // ---- sums ----
    double sum_c = 0.0, sum_m = 0.0;
    for (int i = tid; i < nv; i += kThreads) {
        sum_c += fabs(inv_buf[i] - t_colmap);
        sum_m += (double)fabsf(v_buf[i] - t_mono);
    }
    sum_c = block_sum(sum_c, s, 0);
    sum_m = block_sum(sum_m, s, 1);
    if (tid == 0) {
        rec.t_colmap = t_colmap;
        rec.t_mono = (double)t_mono;
        rec.s_colmap = sum_c / (double)nv;
        rec.s_mono = sum_m / (double)nv;
        rec.scale = rec.s_colmap / rec.s_mono;
        rec.offset = rec.t_colmap - rec.t_mono * rec.scale;
        rec.flags |= GSR_DEPTH_SCALE_FITTED;
        a.out[m] = rec;
    }
}

int fail(int rc, const std::string &msg) {
    set_last_error(msg);
    return rc;
}

size_t align16(size_t b) { return (b + 15) / 16 * 16; }

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_depth_scale_lds_capacity(void) { return kCap; }

size_t gsr_depth_scale_scratch_bytes(int64_t L) {
    if (L < 1) return 0;
    return align16(sizeof(double) * (size_t)L) + align16(sizeof(float) * (size_t)L);
}

int gsr_depth_scale_fit(int64_t M, const double *cams, const int64_t *obs_offsets, int64_t L, const int64_t *obs_index,
                        int64_t O, const double *obs_xy, const int64_t *obs_point_id, int64_t N, int64_t T,
                        const int32_t *table, const double *point_xyz, int64_t K, int Hd, int Wd, const uint16_t *maps,
                        int missing, void *scratch, gsr_depth_scale_record *records, void *stream) {
    const char *who = "gsr_depth_scale_fit";
    if (M < 0 || M >= (1LL << 31) || L < 0 || O < 0 || N < 0 || N >= (1LL << 31) || T < 0 || T > (1LL << 31) - 1 || K < 0)
        return fail(GSR_ERR_INVALID_ARGUMENT,
                    std::string(who) + ": bad sizes (0 <= M, N < 2^31, L, O, K >= 0, 0 <= T <= 2^31 - 1)");
    if (missing != 0 && missing != 1)
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": missing: expected 0 (origin) or 1 (skip)");
    if (M == 0) return GSR_OK;
    if (Hd < 1 || Wd < 1) return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": a map needs Hd, Wd >= 1");
    if (!obs_index && L > O)
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": without obs_index, L must not exceed O");
    if (!cams || !obs_offsets || !records || (L > 0 && !scratch) || (L > 0 && obs_index == nullptr && O == 0) || (O > 0 && (!obs_xy || !obs_point_id)) ||
        (T > 0 && !table) || (N > 0 && !point_xyz) || (K > 0 && !maps))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL pointer");
    FitArgs a{};
    a.cams = cams;
    a.offsets = obs_offsets;
    a.index = obs_index;
    a.L = L;
    a.O = O;
    a.xy = obs_xy;
    a.pid = obs_point_id;
    a.N = N;
    a.T = T;
    a.table = table;
    a.xyz = point_xyz;
    a.K = K;
    a.Hd = Hd;
    a.Wd = Wd;
    a.maps = maps;
    a.missing = missing;
    a.spill_inv = static_cast<double *>(scratch);
    a.spill_v = reinterpret_cast<float *>(static_cast<char *>(scratch) + align16(sizeof(double) * (size_t)L));
    a.out = records;
    hipLaunchKernelGGL(depth_scale_fit_kernel, dim3((unsigned)M), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched(who);
}

}  // extern "C"
