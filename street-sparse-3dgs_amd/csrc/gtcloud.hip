// gtcloud.hip -- the ground-truth point cloud constraint of densification (include/gsr_gtcloud.h):
// "is any cloud point within thr of this Gaussian?" for every row, where the reference
// (scene/gaussian_model.py:853-962, compare_points_to_gt) copies the positions to the host and
// scans all G points per query with a FAISS flat index on every densification.
//
//   build (once per cloud, off the hot path): fp32 bounding box, a uniform grid with cell edge
//          h >= thr (and >= extent / 2^20, so a 64-bit key holds three cell coordinates), one key
//          per point, rocPRIM pair sort (sort.hip), the points gathered as float4 in key order --
//          a cell is one contiguous 16-byte-aligned run -- and the sorted table of the occupied
//          cells (key, first point) from rocPRIM's unique_by_key.  16 B per point + 12 B per
//          occupied cell stay; a dense table at 5 cm over a street block would not fit.
//   query: a lane per row.  Along x the cells of one (y, z) row have consecutive keys, so the
//          points of cells x0..x1 are ONE run of the sorted array: per (y, z) row one binary search
//          of the cell table and a walk of at most x1 - x0 + 1 entries.  A run of up to kLaneRun
//          points is scanned by its own lane (early exit at the first point within thr); longer
//          runs -- a scanner's own position or a wall can put tens of thousands of points in one
//          cell -- are taken one after the other by the whole wave: the owner's position and run
//          are broadcast, the 64 lanes read consecutive float4s (coalesced) and the wave leaves
//          the run at the first 64-point slice with a hit.  The row loop's trip count is
//          wave-uniform (__any), so the broadcasts run with every lane active.
//
// Exactness.  Write T for the largest fp32 <= thr^2 and d2 for the fp32 squared distance of
// gsr_gtcloud.h.  (1) If d2(p, g) <= T then, per axis, |g - p| <= reach, with reach an fp32 >=
// thr (1 + 2^-20): fp32 addition of non-negative terms never rounds below a term (rounding is
// monotone and the term is representable), so rn(dx*dx) <= T with dx = rn(g - p); hence
// |dx| <= thr (1 + 2^-24) and |g - p| <= |dx| (1 + 2^-24) < thr (1 + 2^-22).  (thr^2 is kept in the
// fp32 normal range, so the relative bounds hold.)  (2) lo = the fp32 below rn(p - reach) and
// hi = the fp32 above rn(p + reach) satisfy lo <= p - reach and p + reach <= hi as real numbers, so
// lo <= g <= hi.  (3) The cell coordinate cell_of(v) = clamp(floor(rn(rn(v - o) * inv_h))) is a
// composition of monotone non-decreasing fp32 operations and is evaluated by the same device
// function for cloud points and for lo / hi, so cell_of(lo) <= cell_of(g) <= cell_of(hi) whatever
// the rounding of each step did: a coordinate may be a cell off the real-number one at large
// coordinates, but it is off the same way for both.  The query visits every cell of
// [cell_of(lo), cell_of(hi)] on the three axes, so it tests every point that can have d2 <= T, and
// each test is the d2 rule itself: the mask equals the all-pairs result bit for bit.  An axis whose
// [lo, hi] misses the cloud's bounding box ends the search at once (no point can be in reach).
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gsr.h"
#include "../../include/gsr_gtcloud.h"
#include "grid_cell.h"  // cell_of: monotone non-decreasing in v (the exactness argument above)
#include "gsr_launch.h"

struct gsr_gt_index {
    uint64_t magic;
    gsr::GtGrid grid;
    int64_t G;
    size_t bytes;
    float4 *pts;
    uint64_t *cell_key;
    uint32_t *cell_start;
};

namespace gsr {
namespace {

constexpr uint64_t kGtMagic = 0x6773725f67746964ull;  // "gsr_gtid"
constexpr uint32_t kLaneRun = 16;  // longer runs are shared by the wave

__global__ void gt_bbox_init_kernel(uint32_t *bb) {
    if (threadIdx.x < 3) {
        bb[threadIdx.x] = 0xffffffffu;
        bb[3 + threadIdx.x] = 0u;
    }
}

__global__ __launch_bounds__(256) void gt_bbox_kernel(int64_t G, const float *__restrict__ p, uint32_t *bb) {
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float v = p[3 * i + k];
            mn[k] = fminf(mn[k], v);
            mx[k] = fmaxf(mx[k], v);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], o));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            atomicMin(&bb[k], f2ord(mn[k]));
            atomicMax(&bb[3 + k], f2ord(mx[k]));
        }
    }
}

__device__ __forceinline__ uint64_t cell_key_of(int cx, int cy, int cz, const GtGrid &g) {
    return ((uint64_t)cz * (uint64_t)g.n[1] + (uint64_t)cy) * (uint64_t)g.n[0] + (uint64_t)cx;
}

__global__ __launch_bounds__(256) void gt_key_kernel(int64_t G, const float *__restrict__ p, GtGrid g,
                                                     uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G) return;
    const int cx = cell_of(p[3 * i], g.lo[0], g.inv_h, g.n[0]);
    const int cy = cell_of(p[3 * i + 1], g.lo[1], g.inv_h, g.n[1]);
    const int cz = cell_of(p[3 * i + 2], g.lo[2], g.inv_h, g.n[2]);
    key[i] = cell_key_of(cx, cy, cz, g);
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void gt_gather_kernel(int64_t G, const float *__restrict__ p,
                                                        const uint32_t *__restrict__ idx, float4 *__restrict__ pts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G) return;
    const int64_t s = idx[i];
    pts[i] = make_float4(p[3 * s], p[3 * s + 1], p[3 * s + 2], 0.f);
}

// the d2 rule: (dx*dx + dy*dy) + dz*dz, d = g - p, each operation rounded to fp32.  "Not farther
// than thr" is !(d2 > T): a NaN (an infinite difference never arises from finite inputs short of
// overflow, which gives +Inf: far) counts as near, as "every d2 > thr^2" fails on it.
__device__ __forceinline__ bool gt_near(const float4 c, float qx, float qy, float qz, float T) {
    const float dx = __fsub_rn(c.x, qx), dy = __fsub_rn(c.y, qy), dz = __fsub_rn(c.z, qz);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    return !(d2 > T);
}

__global__ __launch_bounds__(256) void gt_far_mask_kernel(int64_t P, const float *__restrict__ xyz, GtGrid g, float T,
                                                          float reach, const uint8_t *__restrict__ skip,
                                                          uint8_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = i < P && (skip == nullptr || skip[i] == 0);
    float q[3] = {0.f, 0.f, 0.f};
    if (active) {
        q[0] = xyz[3 * i];
        q[1] = xyz[3 * i + 1];
        q[2] = xyz[3 * i + 2];
    }
    // the reference's XY bounds test (inclusive, fp32; NaN / Inf fail it); no z test
    const bool inside = active && q[0] >= g.lo[0] && q[0] <= g.hi[0] && q[1] >= g.lo[1] && q[1] <= g.hi[1];
    bool far = inside && !isnan(q[2]);  // until a point within thr is found
    bool search = far && !isinf(q[2]);  // an infinite z: every d2 is +Inf
    int c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float lo = nextafterf(__fsub_rn(q[k], reach), -INFINITY);
        const float hi = nextafterf(__fadd_rn(q[k], reach), INFINITY);
        if (hi < g.lo[k] || lo > g.hi[k]) search = false;  // no cloud point in reach along this axis
        c0[k] = cell_of(lo, g.lo[k], g.inv_h, g.n[k]);
        c1[k] = cell_of(hi, g.lo[k], g.inv_h, g.n[k]);
    }
    const int64_t ny = c1[1] - c0[1] + 1;
    const int64_t nrows = search ? ny * (int64_t)(c1[2] - c0[2] + 1) : 0;
    for (int64_t r = 0; __any(r < nrows && far); r++) {
        uint32_t s = 0, e = 0;
        if (r < nrows && far) {
            const int cz = c0[2] + (int)(r / ny), cy = c0[1] + (int)(r % ny);
            const uint64_t k0 = cell_key_of(c0[0], cy, cz, g), k1 = cell_key_of(c1[0], cy, cz, g);
            uint32_t a = 0, b = g.n_cells;
            while (a < b) {  // the first occupied cell with key >= k0
                const uint32_t m = (a + b) >> 1;
                if (g.cell_key[m] < k0) a = m + 1;
                else b = m;
            }
            uint32_t j = a;
            while (j < g.n_cells && g.cell_key[j] <= k1) j++;
            s = g.cell_start[a];  // cell_start[n_cells] = G
            e = g.cell_start[j];
        }
        if (e - s <= kLaneRun) {
            for (uint32_t j = s; j < e; j++) {
                if (gt_near(g.pts[j], q[0], q[1], q[2], T)) {
                    far = false;
                    break;
                }
            }
            s = e;
        }
        unsigned long long pending = __ballot(e > s);
        while (pending) {
            const int l = __ffsll((long long)pending) - 1;
            pending &= pending - 1;
            const float bx = __shfl(q[0], l), by = __shfl(q[1], l), bz = __shfl(q[2], l);
            const uint32_t bs = (uint32_t)__shfl((int)s, l), be = (uint32_t)__shfl((int)e, l);
            bool hit = false;
            for (uint32_t j = bs; j < be && !hit; j += 64) {
                const uint32_t jj = j + lane;
                const bool h = jj < be && gt_near(g.pts[jj], bx, by, bz, T);
                hit = __any(h);
            }
            if (hit && lane == l) far = false;
        }
    }
    if (i < P) out[i] = far ? 1 : 0;
}

}  // namespace

bool gt_grid_of(const void *index, GtGrid *out) {
    const gsr_gt_index *ix = static_cast<const gsr_gt_index *>(index);
    if (!ix || ix->magic != kGtMagic) return false;
    *out = ix->grid;
    return true;
}

bool gt_thresholds(double thr, float *T, float *reach) {
    if (!(thr > 0.0) || !std::isfinite(thr)) return false;
    const double t2 = thr * thr;
    if (!(t2 >= (double)FLT_MIN) || t2 > (double)FLT_MAX) return false;
    float t = (float)t2;
    if ((double)t > t2) t = std::nextafterf(t, 0.f);
    const double r = thr * (1.0 + 1.0 / 1048576.0);
    float rf = (float)r;
    if ((double)rf < r) rf = std::nextafterf(rf, INFINITY);
    if (!std::isfinite(rf)) return false;
    *T = t;
    *reach = rf;
    return true;
}

void launch_gt_far_mask(int64_t P, const float *xyz, const GtGrid &g, float T, float reach, const uint8_t *skip,
                        uint8_t *out, hipStream_t s) {
    if (P <= 0) return;
    hipLaunchKernelGGL(gt_far_mask_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, xyz, g, T, reach,
                       skip, out);
}

}  // namespace gsr

using namespace gsr;

extern "C" {

gsr_gt_index *gsr_gt_index_create(int64_t G, const float *points, double thr, void *stream) {
    float T, reach;
    if (G < 1 || G >= (1LL << 31) || !points || !gt_thresholds(thr, &T, &reach)) {
        set_last_error("gsr_gt_index_create: need 1 <= G < 2^31 points and a finite thr > 0 with thr^2 an fp32 normal");
        return nullptr;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<void *> held;
    auto fail = [&](const std::string &what, hipError_t e) {
        for (void *p : held) (void)hipFree(p);
        set_last_error("gsr_gt_index_create: " + what + ": " + hipGetErrorString(e));
        return static_cast<gsr_gt_index *>(nullptr);
    };
    auto alloc = [&](size_t bytes, hipError_t *e) {
        void *p = nullptr;
        *e = hipMalloc(&p, bytes ? bytes : 1);
        if (*e == hipSuccess) held.push_back(p);
        return p;
    };
    auto release = [&](void *p) {
        for (auto &h : held)
            if (h == p) {
                (void)hipFree(p);
                h = held.back();
                held.pop_back();
                return;
            }
    };
    hipError_t e;
    const size_t n = (size_t)G;
    const unsigned blocks = (unsigned)((n + 255) / 256);

    // 1. the fp32 bounding box
    uint32_t *bb = static_cast<uint32_t *>(alloc(6 * sizeof(uint32_t), &e));
    if (e != hipSuccess) return fail("allocation", e);
    hipLaunchKernelGGL(gt_bbox_init_kernel, dim3(1), dim3(64), 0, s, bb);
    hipLaunchKernelGGL(gt_bbox_kernel, dim3(blocks < 1024u ? blocks : 1024u), dim3(256), 0, s, G, points, bb);
    uint32_t hbb[6];
    e = hipMemcpyAsync(hbb, bb, sizeof(hbb), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail("bounding box", e);
    release(bb);
    GtGrid g{};
    float ext = 0.f;
    for (int k = 0; k < 3; k++) {
        g.lo[k] = ord2f(hbb[k]);
        g.hi[k] = ord2f(hbb[3 + k]);
        if (!std::isfinite(g.lo[k]) || !std::isfinite(g.hi[k]) || !std::isfinite(g.hi[k] - g.lo[k])) {
            for (void *p : held) (void)hipFree(p);
            set_last_error("gsr_gt_index_create: the cloud has a non-finite coordinate or extent");
            return nullptr;
        }
        ext = fmaxf(ext, g.hi[k] - g.lo[k]);
    }
    // 2. the grid: edge >= reach >= thr, at most 2^20 + 2 cells per axis (a 64-bit key holds three)
    const float h = fmaxf(reach, ext / 1048576.f);
    g.inv_h = 1.f / h;
    if (!std::isfinite(g.inv_h) || !(g.inv_h > 0.f)) {
        for (void *p : held) (void)hipFree(p);
        set_last_error("gsr_gt_index_create: cell edge out of the fp32 range");
        return nullptr;
    }
    uint64_t cells = 1;
    for (int k = 0; k < 3; k++) {
        // the device's cell_of(hi) without the clamp; cell_of clamps to n - 1, so the two agree
        const float t = floorf((g.hi[k] - g.lo[k]) * g.inv_h);
        g.n[k] = (int32_t)fminf(fmaxf(t, 0.f), 2097150.f) + 1;
        cells *= (uint64_t)g.n[k];
    }
    int end_bit = 1;
    while (end_bit < 64 && ((cells - 1) >> end_bit) != 0) end_bit++;

    // 3. keys, sort, the points in cell order, the occupied cells
    uint64_t *key_in = static_cast<uint64_t *>(alloc(n * 8, &e));
    if (e != hipSuccess) return fail("allocation", e);
    uint64_t *key = static_cast<uint64_t *>(alloc(n * 8, &e));
    if (e != hipSuccess) return fail("allocation", e);
    uint32_t *idx_in = static_cast<uint32_t *>(alloc(n * 4, &e));
    if (e != hipSuccess) return fail("allocation", e);
    uint32_t *idx = static_cast<uint32_t *>(alloc(n * 4, &e));
    if (e != hipSuccess) return fail("allocation", e);
    size_t tmp_bytes = sort_pairs64_temp_bytes(n, end_bit);
    void *tmp = alloc(tmp_bytes, &e);
    if (e != hipSuccess) return fail("allocation", e);
    hipLaunchKernelGGL(gt_key_kernel, dim3(blocks), dim3(256), 0, s, G, points, g, key_in, idx_in);
    e = sort_pairs64(tmp, tmp_bytes, key_in, key, idx_in, idx, n, end_bit, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail("sort", e);
    release(tmp);
    release(key_in);
    release(idx_in);
    float4 *pts = static_cast<float4 *>(alloc(n * sizeof(float4), &e));
    if (e != hipSuccess) return fail("allocation", e);
    hipLaunchKernelGGL(gt_gather_kernel, dim3(blocks), dim3(256), 0, s, G, points, idx, pts);
    uint64_t *run_key = static_cast<uint64_t *>(alloc(n * 8, &e));
    if (e != hipSuccess) return fail("allocation", e);
    uint32_t *run_start = static_cast<uint32_t *>(alloc(n * 4, &e));
    if (e != hipSuccess) return fail("allocation", e);
    uint32_t *n_runs = static_cast<uint32_t *>(alloc(4, &e));
    if (e != hipSuccess) return fail("allocation", e);
    tmp_bytes = key_runs_temp_bytes(n);
    tmp = alloc(tmp_bytes, &e);
    if (e != hipSuccess) return fail("allocation", e);
    e = key_runs(tmp, tmp_bytes, key, n, run_key, run_start, n_runs, s);
    uint32_t nc = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&nc, n_runs, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail("cell table", e);
    if (nc < 1 || nc > n) {
        for (void *p : held) (void)hipFree(p);
        set_last_error("gsr_gt_index_create: cell table: impossible cell count");
        return nullptr;
    }
    release(tmp);
    release(key);
    release(idx);
    release(n_runs);
    uint64_t *cell_key = static_cast<uint64_t *>(alloc((size_t)nc * 8, &e));
    if (e != hipSuccess) return fail("allocation", e);
    uint32_t *cell_start = static_cast<uint32_t *>(alloc(((size_t)nc + 1) * 4, &e));
    if (e != hipSuccess) return fail("allocation", e);
    const uint32_t G32 = (uint32_t)G;
    e = hipMemcpyAsync(cell_key, run_key, (size_t)nc * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(cell_start, run_start, (size_t)nc * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(cell_start + nc, &G32, 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail("cell table copy", e);
    release(run_key);
    release(run_start);

    g.pts = pts;
    g.cell_key = cell_key;
    g.cell_start = cell_start;
    g.n_cells = nc;
    gsr_gt_index *ix = new gsr_gt_index{};
    ix->magic = kGtMagic;
    ix->grid = g;
    ix->G = G;
    ix->bytes = n * sizeof(float4) + (size_t)nc * 8 + ((size_t)nc + 1) * 4;
    ix->pts = pts;
    ix->cell_key = cell_key;
    ix->cell_start = cell_start;
    return ix;
}

void gsr_gt_index_destroy(gsr_gt_index *index) {
    if (!index || index->magic != kGtMagic) return;
    index->magic = 0;
    (void)hipFree(index->pts);
    (void)hipFree(index->cell_key);
    (void)hipFree(index->cell_start);
    delete index;
}

int gsr_gt_index_bounds(const gsr_gt_index *index, float *bounds) {
    GtGrid g;
    if (!gt_grid_of(index, &g) || !bounds) {
        set_last_error("gsr_gt_index_bounds: not an index, or NULL output");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    bounds[0] = g.lo[0];
    bounds[1] = g.hi[0];
    bounds[2] = g.lo[1];
    bounds[3] = g.hi[1];
    return GSR_OK;
}

int gsr_gt_index_info(const gsr_gt_index *index, int64_t *info, int n) {
    GtGrid g;
    if (!gt_grid_of(index, &g) || !info || n < 0) {
        set_last_error("gsr_gt_index_info: not an index, or NULL output");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const int64_t v[6] = {index->G, (int64_t)g.n_cells, (int64_t)index->bytes, g.n[0], g.n[1], g.n[2]};
    for (int k = 0; k < n && k < 6; k++) info[k] = v[k];
    return GSR_OK;
}

int gsr_gt_far_mask(int64_t P, const float *xyz, const gsr_gt_index *index, double thr, const uint8_t *skip,
                    uint8_t *out_mask, void *stream) {
    GtGrid g;
    float T, reach;
    if (P < 0 || !gt_grid_of(index, &g) || !gt_thresholds(thr, &T, &reach) || (P > 0 && (!xyz || !out_mask))) {
        set_last_error("gsr_gt_far_mask: bad size, index, threshold or NULL pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    launch_gt_far_mask(P, xyz, g, T, reach, skip, out_mask, static_cast<hipStream_t>(stream));
    return launched("gsr_gt_far_mask");
}

}  // extern "C"
