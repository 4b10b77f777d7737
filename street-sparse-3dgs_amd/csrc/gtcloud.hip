// gtcloud.hip -- the ground-truth point cloud constraint of densification (include/gsr_gtcloud.h):
// "is any cloud point within thr of this Gaussian?" for every row, where the reference
// (scene/gaussian_model.py:853-962, compare_points_to_gt) copies the positions to the host and
// scans all G points per query with a FAISS flat index on every densification.
//
//   build (once per cloud, off the hot path): fp32 bounding box, a sparse cell grid (grid_cell.h)
//          with cell edge h >= thr (and >= extent / 2^20, so a 64-bit key holds three cell
//          coordinates), one key per point, the cell table's host build, and the points gathered as
//          float4 in key order: a cell is one contiguous 16-byte-aligned run.  16 B per point + 12 B
//          per occupied cell stay; a dense table at 5 cm over a street block would not fit.
//   query: a lane per row walks the cells within reach (grid_cell.h's cell_walk) with the d2 rule as
//          the predicate.
//
// Exactness.  Write T for the largest fp32 <= thr^2 and d2 for the fp32 squared distance of
// gsr_gtcloud.h.  (1) If d2(p, g) <= T then, per axis, |g - p| <= reach, with reach an fp32 >=
// thr (1 + 2^-20): fp32 addition of non-negative terms never rounds below a term (rounding is
// monotone and the term is representable), so rn(dx*dx) <= T with dx = rn(g - p); hence
// |dx| <= thr (1 + 2^-24) and |g - p| <= |dx| (1 + 2^-24) < thr (1 + 2^-22).  (thr^2 is kept in the
// fp32 normal range, so the relative bounds hold.)  (2) lo = the fp32 below rn(p - reach) and
// hi = the fp32 above rn(p + reach) satisfy lo <= p - reach and p + reach <= hi as real numbers, so
// lo <= g <= hi.  (3) The walk over [cell_of(lo), cell_of(hi)] then tests every point that can have
// d2 <= T, each by the d2 rule itself (grid_cell.h's argument): the mask equals the all-pairs result
// bit for bit.  An axis whose [lo, hi] misses the cloud's bounding box ends the search at once (no
// point can be in reach).
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "../../include/gsr.h"
#include "../../include/gsr_gtcloud.h"
#include "grid_cell.h"
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

__global__ void gt_bbox_init_kernel(uint32_t *bb) { bbox_words_init(bb); }

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
    if (cell_walk(g, c0, c1, search, q[0], q[1], q[2],
                  [&](uint32_t j, float x, float y, float z) { return gt_near(g.pts[j], x, y, z, T); }))
        far = false;
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
    const char *who = "gsr_gt_index_create";
    DeviceBufs bufs;
    const size_t n = (size_t)G;
    const unsigned blocks = (unsigned)((n + 255) / 256);

    // 1. the fp32 bounding box
    uint32_t *bb = bufs.alloc<uint32_t>(kBBoxWords);
    if (bufs.error() != hipSuccess) return build_stopped(who, {"allocation", bufs.error()});
    hipLaunchKernelGGL(gt_bbox_init_kernel, dim3(1), dim3(64), 0, s, bb);
    launch_bbox(G, points, nullptr, bb, s);
    uint32_t hbb[6];
    hipError_t e = hipMemcpyAsync(hbb, bb, sizeof(hbb), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return build_stopped(who, {"bounding box", e});
    bufs.release(bb);
    GtGrid g{};
    float ext = 0.f;
    if (!cell_grid_box(&g, hbb, &ext)) return build_stopped(who, {"the cloud has a non-finite coordinate or extent"});
    // 2. the grid: edge >= reach >= thr, at most 2^20 + 2 cells per axis (a 64-bit key holds three)
    uint64_t cells = 1;
    if (!cell_grid_dims(&g, fmaxf(reach, ext / 1048576.f), &cells))
        return build_stopped(who, {"cell edge out of the fp32 range"});
    const int end_bit = std::max(1, bits_for(cells));

    // 3. keys, the cell table, the points in cell order
    uint64_t *key_in = bufs.alloc<uint64_t>(n);
    uint32_t *idx_in = bufs.alloc<uint32_t>(n);
    if (bufs.error() != hipSuccess) return build_stopped(who, {"allocation", bufs.error()});
    hipLaunchKernelGGL(gt_key_kernel, dim3(blocks), dim3(256), 0, s, G, points, g, key_in, idx_in);
    CellTable t;
    if (const BuildStop stop = sort_cell_pairs(bufs, key_in, idx_in, (uint32_t)G, end_bit, s, &t))
        return build_stopped(who, stop);
    float4 *pts = bufs.alloc<float4>(n);
    if (bufs.error() != hipSuccess) return build_stopped(who, {"allocation", bufs.error()});
    hipLaunchKernelGGL(gt_gather_kernel, dim3(blocks), dim3(256), 0, s, G, points, t.values, pts);
    if (const BuildStop stop = finish_cell_table(bufs, (uint32_t)G, false, s, &t)) return build_stopped(who, stop);
    bufs.disown();

    g.pts = pts;
    g.cell_key = t.cell_key;
    g.cell_start = t.cell_start;
    g.n_cells = t.n_cells;
    gsr_gt_index *ix = new gsr_gt_index{};
    ix->magic = kGtMagic;
    ix->grid = g;
    ix->G = G;
    ix->bytes = n * sizeof(float4) + (size_t)t.n_cells * 8 + ((size_t)t.n_cells + 1) * 4;
    ix->pts = pts;
    ix->cell_key = t.cell_key;
    ix->cell_start = t.cell_start;
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
