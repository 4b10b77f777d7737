// chunker.hip -- the scene partition: every chunk's points, cameras' counts, candidate cameras and kept
// observations from one pass over the calibration (include/gsr_chunker.h).
//
//   classify_points   one thread per point: the pbox cell of the fp64 position (cell64) and, for rows of
//                     C, of its fp32 rounding (cell32).  Per axis a floor estimate, then corrected
//                     against bx(e), bx(e + 1) themselves; the strict test on those values decides.
//   classify_centers  the same search without the outer extension, over camera and depth centres
//   id_range/id_table min / max id (wave reduction, one atomic per wave); table[id] = row by atomicCAS
//                     on a table of -1, a second claim of an entry raising the duplicate flag
//   camera_counts     one wave per camera, 64 observations a turn: id -> row -> cell32, then a peel loop
//                     (first pending lane's cell, ballot of the lanes that share it, one atomic add of
//                     the popcount); plain global atomics -- a grid may have more cells than LDS holds
//                     and a camera's observations fall in a handful
//   candidates        state of (cell, m) in ascending (cell, m): ballot per wave, rocPRIM scan, one write
//   obs_filter        one wave per (cell, camera) pair: count, rocPRIM scan, ordered write
//   points_by_cell    stable radix sort of (cell32 or `cells`, row), then a lower bound per cell
#include <algorithm>
#include <cmath>
#include <cstring>  // memset, for rocprim.hpp
#include <string>

#include <rocprim/rocprim.hpp>

#include "../../include/gsr.h"
#include "../../include/gsr_chunker.h"
#include "gsr_launch.h"

namespace gsr {
namespace {

constexpr double kFar = 1e12;
constexpr int kRangeBlocks = 1024;

// bx(i) / by(j): one rounded product, one rounded sum (the file is built with -ffp-contract=off)
__host__ __device__ inline double bound(double o, int i, double cs) { return o + (double)i * cs; }

// The index e with lo(e) < v < hi(e), or -1.  lo(e) = bound(e), hi(e) = bound(e + 1); with ext the
// outer two are -+1e12.  bound() is monotone in e, so after the two walks v lies in cell e or in none.
__device__ inline int axis_cell(double v, double o, double cs, int n, bool ext) {
    if (!(v == v)) return -1;
    const double t = floor((v - o) / cs);
    int e = !(t > 0.0) ? 0 : (t >= (double)(n - 1) ? n - 1 : (int)t);
    while (e > 0 && !(v > bound(o, e, cs))) --e;
    while (e < n - 1 && !(v < bound(o, e + 1, cs))) ++e;
    const double lo = (ext && e == 0) ? -kFar : bound(o, e, cs);
    const double hi = (ext && e == n - 1) ? kFar : bound(o, e + 1, cs);
    return (lo < v && v < hi) ? e : -1;
}

__device__ inline int cell_of(double x, double y, double z, const gsr_chunk_grid &g, bool ext) {
    if (!(-kFar < z && z < kFar)) return -1;
    const int i = axis_cell(x, g.x0, g.cs, g.n_w, ext);
    if (i < 0) return -1;
    const int j = axis_cell(y, g.y0, g.cs, g.n_h, ext);
    return j < 0 ? -1 : i * g.n_h + j;
}

__global__ __launch_bounds__(256) void classify_points_kernel(int64_t N, const double *__restrict__ xyz,
                                                              const float *__restrict__ error, gsr_chunk_grid g,
                                                              int32_t *__restrict__ cell32,
                                                              int32_t *__restrict__ cell64) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const double x = xyz[3 * r], y = xyz[3 * r + 1], z = xyz[3 * r + 2];
    cell64[r] = cell_of(x, y, z, g, true);
    int c = GSR_CHUNK_NOT_IN_C;
    if (error[r] < 10.f) c = cell_of((double)(float)x, (double)(float)y, (double)(float)z, g, true);
    cell32[r] = c;
}

__global__ __launch_bounds__(256) void classify_centers_kernel(int64_t M, const float *__restrict__ cam, int64_t D,
                                                               const double *__restrict__ depth, gsr_chunk_grid g,
                                                               int32_t *__restrict__ cam_cell,
                                                               int32_t *__restrict__ depth_cell) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < M) {
        cam_cell[t] = cell_of((double)cam[3 * t], (double)cam[3 * t + 1], (double)cam[3 * t + 2], g, false);
    } else if (t < M + D) {
        const int64_t d = t - M;
        depth_cell[d] = cell_of(depth[3 * d], depth[3 * d + 1], depth[3 * d + 2], g, false);
    }
}

// ---- ids ----

__global__ void id_range_init_kernel(long long *__restrict__ mm) {
    mm[0] = 0x7fffffffffffffffLL;
    mm[1] = -0x7fffffffffffffffLL - 1;
}

__global__ __launch_bounds__(256) void id_range_kernel(int64_t N, const int64_t *__restrict__ ids,
                                                       long long *__restrict__ mm) {
    long long lo = 0x7fffffffffffffffLL, hi = -0x7fffffffffffffffLL - 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const long long v = ids[i];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&mm[0], lo);
        atomicMax(&mm[1], hi);
    }
}

__global__ __launch_bounds__(256) void id_table_kernel(int64_t N, const int64_t *__restrict__ ids, int64_t T,
                                                       int32_t *__restrict__ table, int *__restrict__ flag) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const int64_t id = ids[r];
    if (id < 0 || id >= T) {
        atomicOr(flag, 1);
    } else if (atomicCAS(&table[id], -1, (int32_t)r) != -1) {
        atomicOr(flag, 2);
    }
}

// ---- per-camera counts ----

// id -> row, or -1
__device__ inline int row_of(int64_t q, int64_t T, const int32_t *__restrict__ table) {
    return (q >= 0 && q < T) ? table[q] : -1;
}

__global__ __launch_bounds__(256) void camera_counts_kernel(int64_t M, int64_t O, const int64_t *__restrict__ obs_ptr,
                                                            const int64_t *__restrict__ obs_id, int64_t T,
                                                            const int32_t *__restrict__ table,
                                                            const int32_t *__restrict__ cell32,
                                                            const double *__restrict__ xyz, int64_t cells,
                                                            int32_t *__restrict__ n_pts, int32_t *__restrict__ blend,
                                                            int32_t *__restrict__ total) {
    const int64_t m = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // one wave per camera
    const int lane = threadIdx.x & 63;
    if (m >= M) return;
    const int64_t b = std::max<int64_t>(obs_ptr[m], 0), e = std::min<int64_t>(obs_ptr[m + 1], O);
    int32_t *const np = n_pts + m * cells, *const bl = blend + m * cells;
    int tot = 0;
    for (int64_t base = b; base < e; base += 64) {
        const int64_t o = base + lane;
        int key = -1;
        bool vis = false;
        if (o < e) {
            const int r = row_of(obs_id[o], T, table);
            if (r >= 0) {
                const int c = cell32[r];
                if (c != GSR_CHUNK_NOT_IN_C) {
                    key = c;
                    vis = (float)xyz[3 * (int64_t)r] != 0.f || (float)xyz[3 * (int64_t)r + 1] != 0.f ||
                          (float)xyz[3 * (int64_t)r + 2] != 0.f;
                }
            }
        }
        tot += __popcll(__ballot(vis));
        bool todo = key >= 0 && key < cells;
        while (__ballot(todo)) {
            int c = 0;
            if (todo) c = __builtin_amdgcn_readfirstlane(key);
            const bool mine = todo && key == c;
            const unsigned long long same = __ballot(mine), seen = __ballot(mine && vis);
            if (mine && lane == __ffsll((long long)same) - 1) {
                atomicAdd(&bl[c], (int32_t)__popcll(same));
                if (seen) atomicAdd(&np[c], (int32_t)__popcll(seen));
            }
            todo = todo && !mine;
        }
    }
    if (lane == 0) total[m] = tot;
}

// ---- candidates ----

struct CandIn {
    int64_t M, cells;
    const float *cam;
    const int32_t *cam_cell, *n_pts;
    gsr_chunk_grid g;
    int add_far;
};

__device__ inline bool in_ebox_axis(double v, double lo, double hi) {
    const double c = (lo + hi) / 2, h = (hi - lo) / 2;
    return c - 2 * h < v && v < c + 2 * h;
}

// 0: none.  n: n_pts[m][cell]
__device__ inline int cand_state(const CandIn &in, int64_t t, int *n_out) {
    const int64_t cell = t / in.M, m = t - cell * in.M;
    const int n = in.n_pts[m * in.cells + cell];
    *n_out = n;
    if (in.cam_cell[m] == (int32_t)cell) return GSR_CHUNK_IN;
    if (n <= 10) return 0;  // neither NEAR (> 20) nor DRAW (> 10)
    const int i = (int)(cell / in.g.n_h), j = (int)(cell - (int64_t)i * in.g.n_h);
    const bool near = n > 20 &&
                      in_ebox_axis((double)in.cam[3 * m], bound(in.g.x0, i, in.g.cs), bound(in.g.x0, i + 1, in.g.cs)) &&
                      in_ebox_axis((double)in.cam[3 * m + 1], bound(in.g.y0, j, in.g.cs), bound(in.g.y0, j + 1, in.g.cs)) &&
                      in_ebox_axis((double)in.cam[3 * m + 2], -kFar, kFar);
    return near ? GSR_CHUNK_NEAR : (in.add_far ? GSR_CHUNK_DRAW : 0);
}

// a wave holds pairs 64 w .. 64 w + 63; cnt has one entry more than there are waves (zero)
__global__ __launch_bounds__(256) void cand_count_kernel(CandIn in, int64_t n, uint32_t *__restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int unused;
    const bool sel = t < n && cand_state(in, t, &unused) != 0;
    const unsigned long long b = __ballot(sel);
    if ((threadIdx.x & 63) == 0 && t < n) cnt[t >> 6] = (uint32_t)__popcll(b);
    if (t == 0) cnt[(n + 63) >> 6] = 0;
}

__global__ __launch_bounds__(256) void cand_write_kernel(CandIn in, int64_t n, const int32_t *__restrict__ total,
                                                         const uint32_t *__restrict__ pre, int32_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int np = 0;
    const int st = t < n ? cand_state(in, t, &np) : 0;
    const unsigned long long b = __ballot(st != 0);
    if (st == 0) return;
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)pre[t >> 6] + __popcll(b & ((1ull << lane) - 1ull));
    const int64_t cell = t / in.M, m = t - cell * in.M;
    int32_t *row = out + 5 * pos;
    row[0] = (int32_t)cell;
    row[1] = (int32_t)m;
    row[2] = st;
    row[3] = np;
    row[4] = total[m];
}

struct CandLayout {
    uint32_t *cnt, *pre;  // per wave (+ 1)
    void *tmp;
    size_t tmp_bytes, total;
};

CandLayout cand_layout(char *base, int64_t n) {
    CandLayout L{};
    Carve c(base);
    const size_t nw = (size_t)((std::max<int64_t>(n, 1) + 63) / 64) + 1;
    L.cnt = c.take<uint32_t>(sizeof(uint32_t) * nw);
    L.pre = c.take<uint32_t>(sizeof(uint32_t) * nw);
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, nw,
                                  rocprim::plus<uint32_t>());
    L.tmp_bytes = bytes;
    L.tmp = c.take(bytes);
    L.total = c.off;
    return L;
}

// ---- observation filter ----

struct ObsIn {
    int64_t P, M, O, T;
    const int32_t *pair_cell, *pair_cam;
    const int64_t *obs_ptr, *obs_id;
    const int32_t *table, *cell64;
};

__device__ inline bool obs_keep(const ObsIn &in, int64_t o, int64_t e, int cell) {
    if (o >= e) return false;
    const int r = row_of(in.obs_id[o], in.T, in.table);
    return r >= 0 && in.cell64[r] == cell;
}

// the pair's observation range, empty for a camera index out of range
__device__ inline void obs_range(const ObsIn &in, int64_t p, int64_t *b, int64_t *e) {
    const int64_t m = in.pair_cam[p];
    *b = *e = 0;
    if (m < 0 || m >= in.M) return;
    *b = std::max<int64_t>(in.obs_ptr[m], 0);
    *e = std::min<int64_t>(in.obs_ptr[m + 1], in.O);
}

// one wave per pair; counts has P + 1 entries (the last zero)
__global__ __launch_bounds__(256) void obs_count_kernel(ObsIn in, int64_t *__restrict__ counts) {
    const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (p >= in.P) return;
    int64_t b, e;
    obs_range(in, p, &b, &e);
    const int cell = in.pair_cell[p];
    int64_t n = 0;
    for (int64_t base = b; base < e; base += 64) n += __popcll(__ballot(obs_keep(in, base + lane, e, cell)));
    if (lane == 0) {
        counts[p] = n;
        if (p == 0) counts[in.P] = 0;
    }
}

__global__ __launch_bounds__(256) void obs_write_kernel(ObsIn in, const int64_t *__restrict__ offsets,
                                                        int64_t *__restrict__ out) {
    const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (p >= in.P) return;
    int64_t b, e;
    obs_range(in, p, &b, &e);
    const int cell = in.pair_cell[p];
    int64_t at = offsets[p];
    const int64_t end = offsets[p + 1];
    for (int64_t base = b; base < e; base += 64) {
        const bool k = obs_keep(in, base + lane, e, cell);
        const unsigned long long mask = __ballot(k);
        const int64_t pos = at + __popcll(mask & ((1ull << lane) - 1ull));
        if (k && pos < end) out[pos] = base + lane;
        at += __popcll(mask);
    }
}

struct ObsLayout {
    int64_t *counts;  // P + 1
    void *tmp;
    size_t tmp_bytes, total;
};

ObsLayout obs_layout(char *base, int64_t P) {
    ObsLayout L{};
    Carve c(base);
    const size_t n = (size_t)std::max<int64_t>(P, 0) + 1;
    L.counts = c.take<int64_t>(sizeof(int64_t) * n);
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, n,
                                  rocprim::plus<int64_t>());
    L.tmp_bytes = bytes;
    L.tmp = c.take(bytes);
    L.total = c.off;
    return L;
}

// ---- points by cell ----

__global__ __launch_bounds__(256) void cell_keys_kernel(int64_t N, const int32_t *__restrict__ cell32, uint32_t cells,
                                                        uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const int32_t c = cell32[r];
    key[r] = (c >= 0 && (uint32_t)c < cells) ? (uint32_t)c : cells;
    val[r] = (uint32_t)r;
}

// offsets[c] = the first sorted position whose key is >= c, for c in [0, cells]
__global__ __launch_bounds__(256) void cell_offsets_kernel(int64_t N, const uint32_t *__restrict__ key, int64_t cells,
                                                           int64_t *__restrict__ offsets) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > cells) return;
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)key[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    offsets[c] = lo;
}

struct CellLayout {
    uint32_t *kin, *kout, *vin;
    void *tmp;
    size_t tmp_bytes, total;
};

int key_bits(int64_t cells) {  // keys 0 .. cells
    int b = 1;
    while (b < 32 && (cells >> b) != 0) ++b;
    return b;
}

CellLayout cell_layout(char *base, int64_t N, int64_t cells) {
    CellLayout L{};
    Carve c(base);
    const size_t n = (size_t)std::max<int64_t>(N, 1);
    L.kin = c.take<uint32_t>(sizeof(uint32_t) * n);
    L.kout = c.take<uint32_t>(sizeof(uint32_t) * n);
    L.vin = c.take<uint32_t>(sizeof(uint32_t) * n);
    L.tmp_bytes = sort_pairs_temp_bytes(n, key_bits(cells));
    L.tmp = c.take(L.tmp_bytes);
    L.total = c.off;
    return L;
}

int fail(int rc, const std::string &msg) {
    set_last_error(msg);
    return rc;
}

int device_fail(const char *who, const char *what, hipError_t e) {
    return fail(GSR_ERR_DEVICE, std::string(who) + ": " + what + ": " + hipGetErrorString(e));
}

bool grid_ok(const gsr_chunk_grid *g) {
    if (!g || g->n_w < 1 || g->n_h < 1 || (int64_t)g->n_w * g->n_h >= (1LL << 31)) return false;
    if (!(std::isfinite(g->x0) && std::isfinite(g->y0) && std::isfinite(g->cs) && g->cs > 0.0)) return false;
    return -kFar < bound(g->x0, 0, g->cs) && bound(g->x0, g->n_w, g->cs) < kFar && -kFar < bound(g->y0, 0, g->cs) &&
           bound(g->y0, g->n_h, g->cs) < kFar;
}

const char *kGridMsg = ": bad grid (1 <= n_w, n_h, n_w n_h < 2^31, finite x0, y0, cs > 0, bounds inside +-1e12)";

unsigned blocks_for(int64_t threads) { return (unsigned)((threads + 255) / 256); }

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_chunk_classify_points(int64_t N, const double *xyz, const float *error, const gsr_chunk_grid *grid,
                              int32_t *cell32, int32_t *cell64, void *stream) {
    const char *who = "gsr_chunk_classify_points";
    if (!grid_ok(grid)) return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + kGridMsg);
    if (N < 0 || N >= (1LL << 31) || (N > 0 && (!xyz || !error || !cell32 || !cell64)))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": bad size (0 <= N < 2^31) or NULL pointer");
    if (N == 0) return GSR_OK;
    hipLaunchKernelGGL(classify_points_kernel, dim3(blocks_for(N)), dim3(256), 0, static_cast<hipStream_t>(stream), N,
                       xyz, error, *grid, cell32, cell64);
    return launched(who);
}

int gsr_chunk_classify_centers(int64_t M, const float *cam_centers, int64_t D, const double *depth_centers,
                               const gsr_chunk_grid *grid, int32_t *cam_cell, int32_t *depth_cell, void *stream) {
    const char *who = "gsr_chunk_classify_centers";
    if (!grid_ok(grid)) return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + kGridMsg);
    if (M < 0 || D < 0 || M + D >= (1LL << 31) || (M > 0 && (!cam_centers || !cam_cell)) ||
        (D > 0 && (!depth_centers || !depth_cell)))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": bad sizes (M, D >= 0, M + D < 2^31) or NULL pointer");
    if (M + D == 0) return GSR_OK;
    hipLaunchKernelGGL(classify_centers_kernel, dim3(blocks_for(M + D)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       M, cam_centers, D, depth_centers, *grid, cam_cell, depth_cell);
    return launched(who);
}

int gsr_chunk_id_range(int64_t N, const int64_t *ids, int64_t *min_max, void *stream) {
    const char *who = "gsr_chunk_id_range";
    if (N < 0 || !min_max || (N > 0 && !ids))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": bad size or NULL pointer");
    min_max[0] = 0;
    min_max[1] = -1;
    if (N == 0) return GSR_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long *mm = nullptr;
    hipError_t e = hipMalloc(&mm, 2 * sizeof(long long));
    if (e != hipSuccess) return device_fail(who, "hipMalloc", e);
    hipLaunchKernelGGL(id_range_init_kernel, dim3(1), dim3(1), 0, s, mm);
    const unsigned blocks = (unsigned)std::min<int64_t>((N + 255) / 256, kRangeBlocks);
    hipLaunchKernelGGL(id_range_kernel, dim3(blocks), dim3(256), 0, s, N, ids, mm);
    long long host[2];
    e = hipMemcpyAsync(host, mm, sizeof(host), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(mm);
    if (e != hipSuccess) return device_fail(who, "read", e);
    min_max[0] = host[0];
    min_max[1] = host[1];
    return launched(who);
}

int gsr_chunk_id_table(int64_t N, const int64_t *ids, int64_t T, int32_t *table, void *stream) {
    const char *who = "gsr_chunk_id_table";
    if (N < 0 || N >= (1LL << 31) || T < 0 || T > (1LL << 31) - 1 || (N > 0 && !ids) || (T > 0 && !table))
        return fail(GSR_ERR_INVALID_ARGUMENT,
                    std::string(who) + ": bad sizes (0 <= N < 2^31, 0 <= T <= 2^31 - 1: the largest id is below 2^31 - 1) "
                                       "or NULL pointer");
    if (N > 0 && T == 0) return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": a point id is negative");
    if (T == 0) return GSR_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(table, 0xFF, sizeof(int32_t) * (size_t)T, s);
    if (e != hipSuccess) return device_fail(who, "memset", e);
    if (N == 0) return GSR_OK;
    int *flag = nullptr;
    e = hipMalloc(&flag, sizeof(int));
    if (e != hipSuccess) return device_fail(who, "hipMalloc", e);
    e = hipMemsetAsync(flag, 0, sizeof(int), s);
    int host = 0;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(id_table_kernel, dim3(blocks_for(N)), dim3(256), 0, s, N, ids, T, table, flag);
        e = hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(flag);
    if (e != hipSuccess) return device_fail(who, "flag", e);
    if (host & 1) return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": a point id is negative or not below T");
    if (host & 2) return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": two points have the same id");
    return launched(who);
}

int gsr_chunk_camera_counts(int64_t M, const int64_t *obs_ptr, int64_t O, const int64_t *obs_point_id, int64_t T,
                            const int32_t *table, const int32_t *cell32, const double *xyz, int64_t cells,
                            int32_t *n_pts, int32_t *blend, int32_t *total, void *stream) {
    const char *who = "gsr_chunk_camera_counts";
    if (M < 0 || O < 0 || T < 0 || T > (1LL << 31) - 1 || cells < 1 || cells >= (1LL << 31) ||
        (M > 0 && M > ((1LL << 31) - 1) / cells))
        return fail(GSR_ERR_INVALID_ARGUMENT,
                    std::string(who) + ": bad sizes (M, O, T >= 0, 1 <= cells, M cells < 2^31)");
    if (M == 0) return GSR_OK;
    if (!obs_ptr || !n_pts || !blend || !total || (O > 0 && !obs_point_id) || (T > 0 && (!table || !cell32 || !xyz)))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t bytes = sizeof(int32_t) * (size_t)(M * cells);
    hipError_t e = hipMemsetAsync(n_pts, 0, bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(blend, 0, bytes, s);
    if (e != hipSuccess) return device_fail(who, "memset", e);
    hipLaunchKernelGGL(camera_counts_kernel, dim3(blocks_for(M * 64)), dim3(256), 0, s, M, O, obs_ptr, obs_point_id, T,
                       table, cell32, xyz, cells, n_pts, blend, total);
    return launched(who);
}

size_t gsr_chunk_candidates_scratch_bytes(int64_t n) {
    if (n < 0 || n >= (1LL << 31)) return 0;
    return cand_layout(nullptr, n).total;
}

static int cand_args(const char *who, int64_t M, const float *cam_centers, const int32_t *cam_cell, const int32_t *n_pts,
                     const gsr_chunk_grid *grid, const void *scratch, CandIn *in) {
    if (!grid_ok(grid)) return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + kGridMsg);
    const int64_t cells = (int64_t)grid->n_w * grid->n_h;
    if (M < 0 || (M > 0 && M > ((1LL << 31) - 1) / cells))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": bad sizes (M >= 0, M cells < 2^31)");
    if (!scratch || (M > 0 && (!cam_centers || !cam_cell || !n_pts)))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL pointer");
    *in = CandIn{M, cells, cam_centers, cam_cell, n_pts, *grid, 0};
    return GSR_OK;
}

int gsr_chunk_candidates_count(int64_t M, const float *cam_centers, const int32_t *cam_cell, const int32_t *n_pts,
                               const gsr_chunk_grid *grid, int add_far_cams, void *scratch, int64_t *count, void *stream) {
    const char *who = "gsr_chunk_candidates_count";
    CandIn in;
    const int rc = cand_args(who, M, cam_centers, cam_cell, n_pts, grid, scratch, &in);
    if (rc != GSR_OK) return rc;
    if (!count) return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL pointer");
    *count = 0;
    if (M == 0) return GSR_OK;
    in.add_far = add_far_cams != 0;
    const int64_t n = M * in.cells;
    const CandLayout L = cand_layout(static_cast<char *>(scratch), n);
    const size_t nw = (size_t)((n + 63) / 64) + 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cand_count_kernel, dim3(blocks_for(n)), dim3(256), 0, s, in, n, L.cnt);
    size_t tb = L.tmp_bytes;
    hipError_t e = rocprim::exclusive_scan(L.tmp, tb, L.cnt, L.pre, 0u, nw, rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return device_fail(who, "scan", e);
    uint32_t host = 0;
    e = hipMemcpyAsync(&host, L.pre + (nw - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_fail(who, "count", e);
    *count = host;
    return launched(who);
}

int gsr_chunk_candidates_write(int64_t M, const float *cam_centers, const int32_t *cam_cell, const int32_t *n_pts,
                               const int32_t *total, const gsr_chunk_grid *grid, int add_far_cams, const void *scratch,
                               int32_t *out, void *stream) {
    const char *who = "gsr_chunk_candidates_write";
    CandIn in;
    const int rc = cand_args(who, M, cam_centers, cam_cell, n_pts, grid, scratch, &in);
    if (rc != GSR_OK) return rc;
    if (M == 0) return GSR_OK;
    if (!total || !out) return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL pointer");
    in.add_far = add_far_cams != 0;
    const int64_t n = M * in.cells;
    const CandLayout L = cand_layout(const_cast<char *>(static_cast<const char *>(scratch)), n);
    hipLaunchKernelGGL(cand_write_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), in, n,
                       total, L.pre, out);
    return launched(who);
}

size_t gsr_chunk_obs_filter_scratch_bytes(int64_t P) {
    if (P < 0 || P >= (1LL << 31)) return 0;
    return obs_layout(nullptr, P).total;
}

static int obs_args(const char *who, int64_t P, const int32_t *pair_cell, const int32_t *pair_cam, int64_t M,
                    const int64_t *obs_ptr, int64_t O, const int64_t *obs_point_id, int64_t T, const int32_t *table,
                    const int32_t *cell64, ObsIn *in) {
    if (P < 0 || P >= (1LL << 31) || M < 0 || O < 0 || T < 0 || T > (1LL << 31) - 1)
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": bad sizes (0 <= P < 2^31, M, O, T >= 0)");
    if (P > 0 && (!pair_cell || !pair_cam || !obs_ptr || (O > 0 && !obs_point_id) || (T > 0 && (!table || !cell64))))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL pointer");
    *in = ObsIn{P, M, O, T, pair_cell, pair_cam, obs_ptr, obs_point_id, table, cell64};
    return GSR_OK;
}

int gsr_chunk_obs_filter_count(int64_t P, const int32_t *pair_cell, const int32_t *pair_cam, int64_t M,
                               const int64_t *obs_ptr, int64_t O, const int64_t *obs_point_id, int64_t T,
                               const int32_t *table, const int32_t *cell64, void *scratch, int64_t *offsets,
                               int64_t *n_kept, void *stream) {
    const char *who = "gsr_chunk_obs_filter_count";
    ObsIn in;
    const int rc = obs_args(who, P, pair_cell, pair_cam, M, obs_ptr, O, obs_point_id, T, table, cell64, &in);
    if (rc != GSR_OK) return rc;
    if (!scratch || !offsets || !n_kept) return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL pointer");
    *n_kept = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P == 0) {
        const hipError_t e = hipMemsetAsync(offsets, 0, sizeof(int64_t), s);
        return e == hipSuccess ? GSR_OK : device_fail(who, "memset", e);
    }
    const ObsLayout L = obs_layout(static_cast<char *>(scratch), P);
    hipLaunchKernelGGL(obs_count_kernel, dim3(blocks_for(P * 64)), dim3(256), 0, s, in, L.counts);
    size_t tb = L.tmp_bytes;
    hipError_t e = rocprim::exclusive_scan(L.tmp, tb, L.counts, offsets, (int64_t)0, (size_t)P + 1,
                                           rocprim::plus<int64_t>(), s);
    if (e != hipSuccess) return device_fail(who, "scan", e);
    int64_t host = 0;
    e = hipMemcpyAsync(&host, offsets + P, sizeof(int64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_fail(who, "count", e);
    *n_kept = host;
    return launched(who);
}

int gsr_chunk_obs_filter_write(int64_t P, const int32_t *pair_cell, const int32_t *pair_cam, int64_t M,
                               const int64_t *obs_ptr, int64_t O, const int64_t *obs_point_id, int64_t T,
                               const int32_t *table, const int32_t *cell64, const int64_t *offsets, int64_t *out_index,
                               void *stream) {
    const char *who = "gsr_chunk_obs_filter_write";
    ObsIn in;
    const int rc = obs_args(who, P, pair_cell, pair_cam, M, obs_ptr, O, obs_point_id, T, table, cell64, &in);
    if (rc != GSR_OK) return rc;
    if (P == 0) return GSR_OK;
    if (!offsets) return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL pointer");
    // out_index may be NULL when nothing is kept: the kernel then writes nothing (pos < end never holds)
    hipLaunchKernelGGL(obs_write_kernel, dim3(blocks_for(P * 64)), dim3(256), 0, static_cast<hipStream_t>(stream), in,
                       offsets, out_index);
    return launched(who);
}

size_t gsr_chunk_points_by_cell_scratch_bytes(int64_t N, int64_t cells) {
    if (N < 0 || N >= (1LL << 31) || cells < 1 || cells >= (1LL << 31)) return 0;
    return cell_layout(nullptr, N, cells).total;
}

int gsr_chunk_points_by_cell(int64_t N, const int32_t *cell32, int64_t cells, void *scratch, int32_t *out_rows,
                             int64_t *out_offsets, void *stream) {
    const char *who = "gsr_chunk_points_by_cell";
    if (N < 0 || N >= (1LL << 31) || cells < 1 || cells >= (1LL << 31))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": bad sizes (0 <= N < 2^31, 1 <= cells < 2^31)");
    if (!out_offsets || !scratch || (N > 0 && (!cell32 || !out_rows)))
        return fail(GSR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0) {
        const hipError_t e = hipMemsetAsync(out_offsets, 0, sizeof(int64_t) * (size_t)(cells + 1), s);
        return e == hipSuccess ? GSR_OK : device_fail(who, "memset", e);
    }
    const CellLayout L = cell_layout(static_cast<char *>(scratch), N, cells);
    hipLaunchKernelGGL(cell_keys_kernel, dim3(blocks_for(N)), dim3(256), 0, s, N, cell32, (uint32_t)cells, L.kin, L.vin);
    const hipError_t e = sort_pairs(L.tmp, L.tmp_bytes, L.kin, L.kout, L.vin, reinterpret_cast<uint32_t *>(out_rows),
                                    (size_t)N, key_bits(cells), s);
    if (e != hipSuccess) return device_fail(who, "sort", e);
    hipLaunchKernelGGL(cell_offsets_kernel, dim3(blocks_for(cells + 1)), dim3(256), 0, s, N, L.kout, cells, out_offsets);
    return launched(who);
}

}  // extern "C"
