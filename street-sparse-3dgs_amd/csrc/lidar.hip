// lidar.hip -- a chunk's LiDAR cloud on the device (include/gsr_lidar.h): the crop to the chunk's
// box and the filter "within max_distance of the mesh" in one pass, and the voxel mean that makes the
// initial points.  The reference (preprocess/ss_make_chunk.py:36-305) does the filter with an Open3D
// raycasting scene on the host, 100 000 points at a time, and the voxel mean with Open3D's hash map.
//
//   mesh index (once per mesh): the vertices' fp32 bounding box (non-finite vertices and face indices
//          out of range end the build), a uniform grid of edge h >= 2 reach, count -> scan -> fill:
//          each triangle counts the cells its bounding box grown by the reach touches, a scan gives
//          its first (cell key, triangle) pair, it writes them in (z, y, x) order; a stable rocPRIM
//          pair sort (sort.hip) puts the pairs in cell order with ascending triangle numbers inside
//          a cell, key_runs makes the sorted table of the occupied cells, and the triangles are
//          gathered as nine floats per reference: a cell is one contiguous run.  A triangle whose grown
//          box covers more than kMaxCells cells writes ONE pair under the key past the last cell, so
//          the sort leaves those triangles as the last run: the oversize list.
//   query: a lane per point.  crop, then grid_cell.h's cell_walk over the point's own cell (a range of
//          cells when max_distance exceeds the one the index was built for) with near() as the
//          predicate; then the oversize list, read at wave-uniform addresses by the lanes still
//          without a triangle.
//   voxel mean: ordered-integer bounding box of the kept points, one 64-bit key (iz, iy, ix) per point
//          (dropped points get the key past every voxel), the stable pair sort, key_runs, and one
//          lane per voxel summing its points in fp64 in input order; voxels longer than kLaneRun are
//          taken by the wave: lane l sums points l, l + 64, ... in order, then a butterfly adds the 64
//          partial sums.  No atomics on floats anywhere, so the output is a function of the input.
//
// Exactness of the grid (grid_cell.h has the part shared with gtcloud.hip).  near()
// holds only when !sep: on every axis some vertex v has rn(v - p) < reach and some vertex has
// rn(v - p) > -reach, hence (one rounding, monotone) min_k - reach (1 + 2^-23) <= p_k <=
// max_k + reach (1 + 2^-23) as real numbers.  The build grows the box by reach_b >= reach (1 + 2^-20)
// and steps the fp32 results outward (nextafter), so lo_k <= p_k <= hi_k, and cell_of is monotone and
// the same function for both: cell_of(lo_k) <= cell_of(p_k) <= cell_of(hi_k): the point's own cell
// lists the triangle.  For a larger query reach the point searches
// [cell_of(below(p - e)), cell_of(above(p + e))] with e >= reach_q (1 + 2^-20) - reach_b, which meets
// the triangle's cell range on every axis by the same argument.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>

#include "../../include/gsr.h"
#include "../../include/gsr_lidar.h"
#include "grid_cell.h"
#include "gsr_launch.h"

namespace gsr {

// what the kernels need of a mesh index: cell_start[n_cells] = over_start
struct MeshGrid : CellGrid {
    const float *tri;               // nine floats per reference, cell order, the oversize list last
    uint32_t over_start, over_end;  // the oversize list as references [over_start, over_end)
};

}  // namespace gsr

struct gsr_mesh_index {
    uint64_t magic;
    gsr::MeshGrid grid;
    int64_t V, F, refs;
    size_t bytes;
    float reach_b;  // what the triangles' boxes were grown by
    float *tri;
    uint64_t *cell_key;
    uint32_t *cell_start;
};

namespace gsr {
namespace {

constexpr uint64_t kMeshMagic = 0x6773725f6d657368ull;  // "gsr_mesh"
constexpr uint64_t kMaxCells = 512;  // a triangle covering more cells goes to the oversize list
constexpr uint32_t kSideSteps = 65536;

// ---- the mesh index ----------------------------------------------------------------------------

constexpr uint32_t kMeshBadFace = 2u;  // beside kBBoxNonFinite in the flag word: a face index out of range

__global__ void mesh_words_init_kernel(uint32_t *w, unsigned long long *sums) {
    bbox_words_init(w);
    if (threadIdx.x < 2) sums[threadIdx.x] = 0ull;
}

// the nine floats of triangle t; false when a face index is out of range (nothing is read then)
__device__ __forceinline__ bool tri_fetch(int64_t V, const float *__restrict__ vert, const int32_t *__restrict__ faces,
                                          int64_t t, float v[9]) {
    const int32_t i0 = faces[3 * t], i1 = faces[3 * t + 1], i2 = faces[3 * t + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        v[k] = vert[3 * (int64_t)i0 + k];
        v[3 + k] = vert[3 * (int64_t)i1 + k];
        v[6 + k] = vert[3 * (int64_t)i2 + k];
    }
    return true;
}

// checks every face index and sums the triangles' longest bounding-box sides, each cut at `cap` and
// counted in kSideSteps-ths of it (integers: the sum does not depend on the order of the adds)
__global__ __launch_bounds__(256) void mesh_side_kernel(int64_t V, const float *__restrict__ vert, int64_t F,
                                                        const int32_t *__restrict__ faces, float cap, uint32_t *w,
                                                        unsigned long long *sums) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t q = 0;
    bool bad = false;
    if (t < F) {
        float v[9];
        if (tri_fetch(V, vert, faces, t, v)) {
            float side = 0.f;
#pragma unroll
            for (int k = 0; k < 3; k++)
                side = fmaxf(side, fmaxf(v[k], fmaxf(v[3 + k], v[6 + k])) - fminf(v[k], fminf(v[3 + k], v[6 + k])));
            const float r = fminf(side / cap, 1.f);  // NaN (a non-finite vertex: the build fails anyway) -> 1
            q = (uint32_t)(r * (float)kSideSteps);
        } else {
            bad = true;
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&w[kBBoxFlags], kMeshBadFace);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if ((threadIdx.x & 63) == 0 && q) atomicAdd(&sums[0], (unsigned long long)q);
}

struct TriCells {
    int c0[3], c1[3];
    uint64_t n;
};

__device__ __forceinline__ TriCells tri_cells(const float v[9], const MeshGrid &g, float reach_b) {
    TriCells c;
    c.n = 1;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float mn = fminf(v[k], fminf(v[3 + k], v[6 + k])), mx = fmaxf(v[k], fmaxf(v[3 + k], v[6 + k]));
        const float lo = nextafterf(__fsub_rn(mn, reach_b), -INFINITY);
        const float hi = nextafterf(__fadd_rn(mx, reach_b), INFINITY);
        c.c0[k] = cell_of(lo, g.lo[k], g.inv_h, g.n[k]);
        c.c1[k] = cell_of(hi, g.lo[k], g.inv_h, g.n[k]);
        c.n *= (uint64_t)(c.c1[k] - c.c0[k] + 1);
    }
    return c;
}

// count: the pairs triangle t writes (1 for an oversize one); sums[1]: their total
__global__ __launch_bounds__(256) void mesh_count_kernel(int64_t V, const float *__restrict__ vert, int64_t F,
                                                         const int32_t *__restrict__ faces, MeshGrid g, float reach_b,
                                                         uint32_t *__restrict__ cnt, unsigned long long *sums) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = 0;
    if (t < F) {
        float v[9];
        if (tri_fetch(V, vert, faces, t, v)) {
            const TriCells tc = tri_cells(v, g, reach_b);
            c = tc.n > kMaxCells ? 1u : (uint32_t)tc.n;
        }
        cnt[t] = c;
    }
    uint32_t q = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if ((threadIdx.x & 63) == 0 && q) atomicAdd(&sums[1], (unsigned long long)q);
}

// fill: triangle t's pairs at off[t] .. off[t] + cnt[t], cells in (z, y, x) order
__global__ __launch_bounds__(256) void mesh_fill_kernel(int64_t V, const float *__restrict__ vert, int64_t F,
                                                        const int32_t *__restrict__ faces, MeshGrid g, float reach_b,
                                                        uint64_t over_key, const uint32_t *__restrict__ off, uint32_t R,
                                                        uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= F) return;
    float v[9];
    if (!tri_fetch(V, vert, faces, t, v)) return;
    const TriCells tc = tri_cells(v, g, reach_b);
    uint32_t j = off[t];
    if (tc.n > kMaxCells) {
        if (j < R) {
            key[j] = over_key;
            val[j] = (uint32_t)t;
        }
        return;
    }
    for (int cz = tc.c0[2]; cz <= tc.c1[2]; cz++)
        for (int cy = tc.c0[1]; cy <= tc.c1[1]; cy++)
            for (int cx = tc.c0[0]; cx <= tc.c1[0]; cx++, j++) {
                if (j >= R) return;  // cannot happen: the same function counted the cells
                key[j] = cell_key_of(cx, cy, cz, g);
                val[j] = (uint32_t)t;
            }
}

__global__ __launch_bounds__(256) void mesh_gather_kernel(int64_t V, const float *__restrict__ vert,
                                                          const int32_t *__restrict__ faces, uint32_t R,
                                                          const uint32_t *__restrict__ val, float *__restrict__ tri) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    float v[9];
    if (!tri_fetch(V, vert, faces, val[i], v)) return;
#pragma unroll
    for (int k = 0; k < 9; k++) tri[9 * i + k] = v[k];
}

// ---- the query -----------------------------------------------------------------------------------

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

// a b - c d with the rounding error of c d put back (Kahan): the triangle's normal is a difference of
// products that cancels on a needle, and its direction decides the distance to the face
__device__ __forceinline__ float diff_of_products(float a, float b, float c, float d) {
    const float w = __fmul_rn(c, d);
    const float e = __fmaf_rn(-c, d, w), f = __fmaf_rn(a, b, -w);
    return __fadd_rn(f, e);
}

// the squared distance from the origin to the segment u .. u + e
__device__ __forceinline__ float seg_d2(float ux, float uy, float uz, float ex, float ey, float ez) {
    const float ee = dot3(ex, ey, ez, ex, ey, ez), ue = dot3(ux, uy, uz, ex, ey, ez);
    const float t = ee > 0.f ? fminf(fmaxf(__fdiv_rn(-ue, ee), 0.f), 1.f) : 0.f;
    const float qx = __fadd_rn(ux, __fmul_rn(t, ex)), qy = __fadd_rn(uy, __fmul_rn(t, ey)),
                qz = __fadd_rn(uz, __fmul_rn(t, ez));
    return dot3(qx, qy, qz, qx, qy, qz);
}

// near() of gsr_lidar.h for the triangle at t (nine floats) and the point q
__device__ __forceinline__ bool tri_near(const float *__restrict__ t, float qx, float qy, float qz, float T,
                                         float reach) {
    const float ax = __fsub_rn(t[0], qx), ay = __fsub_rn(t[1], qy), az = __fsub_rn(t[2], qz);
    const float bx = __fsub_rn(t[3], qx), by = __fsub_rn(t[4], qy), bz = __fsub_rn(t[5], qz);
    const float cx = __fsub_rn(t[6], qx), cy = __fsub_rn(t[7], qy), cz = __fsub_rn(t[8], qz);
    const float mnx = fminf(ax, fminf(bx, cx)), mny = fminf(ay, fminf(by, cy)), mnz = fminf(az, fminf(bz, cz));
    const float mxx = fmaxf(ax, fmaxf(bx, cx)), mxy = fmaxf(ay, fmaxf(by, cy)), mxz = fmaxf(az, fmaxf(bz, cz));
    if (mnx >= reach || mny >= reach || mnz >= reach || mxx <= -reach || mxy <= -reach || mxz <= -reach) return false;
    const float abx = __fsub_rn(bx, ax), aby = __fsub_rn(by, ay), abz = __fsub_rn(bz, az);
    const float bcx = __fsub_rn(cx, bx), bcy = __fsub_rn(cy, by), bcz = __fsub_rn(cz, bz);
    const float acx = __fsub_rn(cx, ax), acy = __fsub_rn(cy, ay), acz = __fsub_rn(cz, az);
    float d2 = fminf(seg_d2(ax, ay, az, abx, aby, abz),
                     fminf(seg_d2(bx, by, bz, bcx, bcy, bcz), seg_d2(ax, ay, az, acx, acy, acz)));
    // n = ab x ac; the origin projects inside when n.(b x c), n.(c x a), n.(a x b) are all >= 0
    const float nx = diff_of_products(aby, acz, abz, acy);
    const float ny = diff_of_products(abz, acx, abx, acz);
    const float nz = diff_of_products(abx, acy, aby, acx);
    const float nn = dot3(nx, ny, nz, nx, ny, nz);
    if (nn > 0.f) {
        const float u = dot3(nx, ny, nz, __fsub_rn(__fmul_rn(by, cz), __fmul_rn(bz, cy)),
                             __fsub_rn(__fmul_rn(bz, cx), __fmul_rn(bx, cz)),
                             __fsub_rn(__fmul_rn(bx, cy), __fmul_rn(by, cx)));
        const float v = dot3(nx, ny, nz, __fsub_rn(__fmul_rn(cy, az), __fmul_rn(cz, ay)),
                             __fsub_rn(__fmul_rn(cz, ax), __fmul_rn(cx, az)),
                             __fsub_rn(__fmul_rn(cx, ay), __fmul_rn(cy, ax)));
        const float w = dot3(nx, ny, nz, __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by)),
                             __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz)),
                             __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx)));
        if (u >= 0.f && v >= 0.f && w >= 0.f) {
            const float na = dot3(nx, ny, nz, ax, ay, az);
            d2 = fminf(d2, __fdiv_rn(__fmul_rn(na, na), nn));
        }
    }
    return d2 <= T;
}

struct CropBox {
    float x_lo, x_hi, y_lo, y_hi;
    int on;
};

__global__ __launch_bounds__(256) void mesh_near_mask_kernel(int64_t P, const float *__restrict__ xyz, MeshGrid g,
                                                             int has_index, float T, float reach, float ext, CropBox box,
                                                             uint8_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float q[3] = {0.f, 0.f, 0.f};
    if (i < P) {
        q[0] = xyz[3 * i];
        q[1] = xyz[3 * i + 1];
        q[2] = xyz[3 * i + 2];
    }
    bool ok = i < P && isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
    if (box.on) ok = ok && box.x_lo < q[0] && q[0] < box.x_hi && box.y_lo < q[1] && q[1] < box.y_hi;
    if (!has_index) {  // the crop alone
        if (i < P) out[i] = ok ? 1 : 0;
        return;
    }
    if (!ok) q[0] = q[1] = q[2] = 0.f;
    bool search = ok;
    int c0[3], c1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        // no vertex within reach along this axis: every triangle is separated (sep of gsr_lidar.h)
        if (nextafterf(__fadd_rn(q[k], reach), INFINITY) < g.lo[k] || nextafterf(__fsub_rn(q[k], reach), -INFINITY) > g.hi[k])
            search = false;
        const float lo = ext > 0.f ? nextafterf(__fsub_rn(q[k], ext), -INFINITY) : q[k];
        const float hi = ext > 0.f ? nextafterf(__fadd_rn(q[k], ext), INFINITY) : q[k];
        c0[k] = cell_of(lo, g.lo[k], g.inv_h, g.n[k]);
        c1[k] = cell_of(hi, g.lo[k], g.inv_h, g.n[k]);
    }
    bool near = cell_walk(g, c0, c1, search, q[0], q[1], q[2], [&](uint32_t j, float x, float y, float z) {
        return tri_near(g.tri + 9 * (size_t)j, x, y, z, T, reach);
    });
    // the oversize list: the same triangle for every lane of the wave
    for (uint32_t j = g.over_start; j < g.over_end && __any(search && !near); j++)
        if (search && !near && tri_near(g.tri + 9 * (size_t)j, q[0], q[1], q[2], T, reach)) near = true;
    if (i < P) out[i] = near ? 1 : 0;
}

// ---- the voxel mean --------------------------------------------------------------------------------

struct VoxGrid {
    double o[3];  // lo - s/2
    double s;
    int bits_x, bits_xy;  // key = iz << bits_xy | iy << bits_x | ix
    uint64_t drop_key;    // 1 << (bits of all three): sorts after every voxel
};

// the words of launch_bbox over the kept points, then 8: the number of voxels (key_runs)
__global__ void vox_words_init_kernel(uint32_t *w) {
    bbox_words_init(w);
    if (threadIdx.x == 8) w[8] = 0u;
}

// the voxel coordinate along one axis (gsr_lidar.h): fp64, every operation rounded once
__host__ __device__ __forceinline__ double vox_coord(double p, double o, double s) { return floor((p - o) / s); }

__global__ __launch_bounds__(256) void vox_key_kernel(int64_t P, const float *__restrict__ p,
                                                      const uint8_t *__restrict__ keep, VoxGrid g,
                                                      uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    uint64_t k = g.drop_key;
    if (keep == nullptr || keep[i] != 0) {
        const uint64_t ix = (uint64_t)vox_coord((double)p[3 * i], g.o[0], g.s);
        const uint64_t iy = (uint64_t)vox_coord((double)p[3 * i + 1], g.o[1], g.s);
        const uint64_t iz = (uint64_t)vox_coord((double)p[3 * i + 2], g.o[2], g.s);
        k = (iz << g.bits_xy) | (iy << g.bits_x) | ix;
    }
    key[i] = k;
    idx[i] = (uint32_t)i;
}

struct VoxSum {
    double v[6];
};

__device__ __forceinline__ void vox_add(VoxSum &a, const float *__restrict__ xyz, const float *__restrict__ col,
                                        uint32_t row) {
#pragma unroll
    for (int k = 0; k < 3; k++) a.v[k] += (double)xyz[3 * (size_t)row + k];
    if (col != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.v[3 + k] += (double)col[3 * (size_t)row + k];
    }
}

__device__ __forceinline__ void vox_store(const VoxSum &a, uint32_t n, uint32_t r, float *__restrict__ out_xyz,
                                          float *__restrict__ out_col, int32_t *__restrict__ out_cnt) {
    const double d = (double)n;
#pragma unroll
    for (int k = 0; k < 3; k++) out_xyz[3 * (size_t)r + k] = (float)(a.v[k] / d);
    if (out_col != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; k++) out_col[3 * (size_t)r + k] = (float)(a.v[3 + k] / d);
    }
    out_cnt[r] = (int32_t)n;
}

// a lane per voxel r: its points are idx[run_start[r] .. run_start[r + 1]) (the last voxel ends at K)
__global__ __launch_bounds__(256) void vox_mean_kernel(uint32_t n_runs, uint32_t K, const uint32_t *__restrict__ run_start,
                                                       const uint32_t *__restrict__ idx, const float *__restrict__ xyz,
                                                       const float *__restrict__ col, float *__restrict__ out_xyz,
                                                       float *__restrict__ out_col, int32_t *__restrict__ out_cnt) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t s = 0, e = 0;
    if (r < n_runs) {
        s = run_start[r];
        e = r + 1 < n_runs ? run_start[r + 1] : K;
    }
    if (e > s && e - s <= kLaneRun) {
        VoxSum a{};
        for (uint32_t j = s; j < e; j++) vox_add(a, xyz, col, idx[j]);
        vox_store(a, e - s, r, out_xyz, col != nullptr ? out_col : nullptr, out_cnt);
        s = e;
    }
    unsigned long long pending = __ballot(e > s);
    while (pending) {
        const int l = __ffsll((long long)pending) - 1;
        pending &= pending - 1;
        const uint32_t bs = (uint32_t)__shfl((int)s, l), be = (uint32_t)__shfl((int)e, l);
        VoxSum a{};
        for (uint32_t j = bs + lane; j < be; j += 64) vox_add(a, xyz, col, idx[j]);
#pragma unroll
        for (int k = 0; k < 6; k++) {
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) a.v[k] += __shfl_xor(a.v[k], o);
        }
        if (lane == l) vox_store(a, be - bs, r, out_xyz, col != nullptr ? out_col : nullptr, out_cnt);
    }
}

struct VoxScratch {
    uint64_t *key_in, *key_out;  // key_in is the voxels' keys after the sort
    uint32_t *idx_in, *idx_out;  // idx_in is the voxels' first positions after the sort
    uint32_t *words;
    void *tmp;
    size_t tmp_bytes, total;
};

VoxScratch vox_carve(void *base, size_t P) {
    VoxScratch v{};
    Carve c(base);
    v.key_in = c.take<uint64_t>(P * 8);
    v.key_out = c.take<uint64_t>(P * 8);
    v.idx_in = c.take<uint32_t>(P * 4);
    v.idx_out = c.take<uint32_t>(P * 4);
    v.words = c.take<uint32_t>(64);
    const size_t a = sort_pairs64_temp_bytes(P, 64), b = key_runs_temp_bytes(P);
    v.tmp_bytes = a > b ? a : b;
    v.tmp = c.take(v.tmp_bytes);
    v.total = c.off;
    return v;
}

bool mesh_grid_of(const gsr_mesh_index *ix, MeshGrid *out) {
    if (!ix || ix->magic != kMeshMagic) return false;
    *out = ix->grid;
    return true;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

gsr_mesh_index *gsr_mesh_index_create(int64_t V, const float *vertices, int64_t F, const int32_t *faces,
                                      double max_distance, void *stream) {
    float T, reach;
    if (V < 1 || F < 1 || F >= (1LL << 31) || V >= (1LL << 31) || !vertices || !faces ||
        !gt_thresholds(max_distance, &T, &reach)) {
        set_last_error("gsr_mesh_index_create: need 1 <= V, F < 2^31 and a finite max_distance > 0 with its square an "
                       "fp32 normal");
        return nullptr;
    }
    // what the boxes grow by: covers the one rounding of v - p in the query (the exactness argument)
    const double rb = (double)reach * (1.0 + 1.0 / 1048576.0);
    float reach_b = (float)rb;
    if ((double)reach_b < rb) reach_b = std::nextafterf(reach_b, INFINITY);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const char *who = "gsr_mesh_index_create";
    DeviceBufs bufs;
    const unsigned fblocks = (unsigned)(((size_t)F + 255) / 256);

    // 1. the vertices' bounding box, the face indices, the triangles' mean side
    uint32_t *words = bufs.alloc<uint32_t>(kBBoxWords);
    unsigned long long *sums = bufs.alloc<unsigned long long>(2);
    if (bufs.error() != hipSuccess) return build_stopped(who, {"allocation", bufs.error()});
    const float cap = 8.f * reach_b;
    if (!std::isfinite(cap)) return build_stopped(who, {"max_distance out of the fp32 range"});
    hipLaunchKernelGGL(mesh_words_init_kernel, dim3(1), dim3(64), 0, s, words, sums);
    launch_bbox(V, vertices, nullptr, words, s);
    hipLaunchKernelGGL(mesh_side_kernel, dim3(fblocks), dim3(256), 0, s, V, vertices, F, faces, cap, words, sums);
    uint32_t hw[kBBoxWords];
    unsigned long long hs[2];
    hipError_t e = hipMemcpyAsync(hw, words, sizeof(hw), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(hs, sums, sizeof(hs), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return build_stopped(who, {"bounding box", e});
    if (hw[kBBoxFlags] & kBBoxNonFinite)
        return build_stopped(who, {"the mesh has a vertex with a NaN or Inf coordinate"});
    if (hw[kBBoxFlags] & kMeshBadFace) return build_stopped(who, {"a face index is out of range (0 <= index < V)"});
    MeshGrid g{};
    float ext = 0.f;
    if (!cell_grid_box(&g, hw, &ext)) return build_stopped(who, {"the mesh's extent is out of the fp32 range"});
    // 2. the grid: edge >= 2 reach and about a triangle's side, at most 2^20 + 2 cells per axis
    const float mean_side = (float)((double)cap * (double)hs[0] / ((double)kSideSteps * (double)F));
    uint64_t cells = 1;
    if (!cell_grid_dims(&g, fmaxf(fmaxf(2.f * reach_b, mean_side), ext / 1048576.f), &cells))
        return build_stopped(who, {"cell edge out of the fp32 range"});
    const uint64_t over_key = cells;  // past every cell's key
    const int end_bit = std::max(1, bits_for(cells + 1));

    // 3. count, scan, fill
    uint32_t *cnt = bufs.alloc<uint32_t>((size_t)F);
    uint32_t *off = bufs.alloc<uint32_t>((size_t)F);
    if (bufs.error() != hipSuccess) return build_stopped(who, {"allocation", bufs.error()});
    hipLaunchKernelGGL(mesh_count_kernel, dim3(fblocks), dim3(256), 0, s, V, vertices, F, faces, g, reach_b, cnt, sums);
    e = hipMemcpyAsync(hs, sums, sizeof(hs), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return build_stopped(who, {"count", e});
    if (hs[1] < 1 || hs[1] >= (1ull << 31))
        return build_stopped(who, {"the index would hold more than 2^31 - 1 triangle references"});
    const uint32_t R = (uint32_t)hs[1];
    const unsigned rblocks = (unsigned)(((size_t)R + 255) / 256);
    const size_t tmp_bytes = scan_u32_temp_bytes((size_t)F);
    void *tmp = bufs.alloc<char>(tmp_bytes);
    if (bufs.error() != hipSuccess) return build_stopped(who, {"allocation", bufs.error()});
    e = scan_u32(tmp, tmp_bytes, cnt, off, (size_t)F, s);
    if (e != hipSuccess) return build_stopped(who, {"scan", e});
    uint64_t *key_in = bufs.alloc<uint64_t>(R);
    uint32_t *val_in = bufs.alloc<uint32_t>(R);
    if (bufs.error() != hipSuccess) return build_stopped(who, {"allocation", bufs.error()});
    e = hipMemsetAsync(val_in, 0, (size_t)R * 4, s);  // every slot is written below; a triangle number in any case
    if (e != hipSuccess) return build_stopped(who, {"fill", e});
    hipLaunchKernelGGL(mesh_fill_kernel, dim3(fblocks), dim3(256), 0, s, V, vertices, F, faces, g, reach_b, over_key, off,
                       R, key_in, val_in);
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return build_stopped(who, {"fill", e});
    bufs.release(tmp);
    bufs.release(cnt);
    bufs.release(off);

    // 4. cell order (stable: ascending triangle numbers inside a cell), the triangles, the cell table
    CellTable t;
    if (const BuildStop stop = sort_cell_pairs(bufs, key_in, val_in, R, end_bit, s, &t))
        return build_stopped(who, stop);
    float *tri = bufs.alloc<float>((size_t)R * 9);
    if (bufs.error() != hipSuccess) return build_stopped(who, {"allocation", bufs.error()});
    hipLaunchKernelGGL(mesh_gather_kernel, dim3(rblocks), dim3(256), 0, s, V, vertices, faces, R, t.values, tri);
    if (const BuildStop stop = finish_cell_table(bufs, R, true, s, &t)) return build_stopped(who, stop);
    bufs.release(words);
    bufs.release(sums);
    bufs.disown();

    // the oversize list is the run under over_key, the last one: the cell table ends before it, and
    // cell_start[n_cells] is then its first reference
    const uint32_t nc = t.n_cells;
    const bool has_over = t.last_key == over_key;
    g.tri = tri;
    g.cell_key = t.cell_key;
    g.cell_start = t.cell_start;
    g.n_cells = has_over ? nc - 1 : nc;
    g.over_start = has_over ? t.last_start : R;
    g.over_end = R;
    gsr_mesh_index *ix = new gsr_mesh_index{};
    ix->magic = kMeshMagic;
    ix->grid = g;
    ix->V = V;
    ix->F = F;
    ix->refs = (int64_t)g.over_start;
    ix->bytes = (size_t)R * 9 * sizeof(float) + (size_t)nc * 8 + ((size_t)nc + 1) * 4;
    ix->reach_b = reach_b;
    ix->tri = tri;
    ix->cell_key = t.cell_key;
    ix->cell_start = t.cell_start;
    return ix;
}

void gsr_mesh_index_destroy(gsr_mesh_index *index) {
    if (!index || index->magic != kMeshMagic) return;
    index->magic = 0;
    (void)hipFree(index->tri);
    (void)hipFree(index->cell_key);
    (void)hipFree(index->cell_start);
    delete index;
}

int gsr_mesh_index_info(const gsr_mesh_index *index, int64_t *info, int n) {
    MeshGrid g;
    if (!mesh_grid_of(index, &g) || !info || n < 0) {
        set_last_error("gsr_mesh_index_info: not an index, or NULL output");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const int64_t v[9] = {index->V, index->F, (int64_t)g.n_cells, index->refs, (int64_t)(g.over_end - g.over_start),
                          (int64_t)index->bytes, g.n[0], g.n[1], g.n[2]};
    for (int k = 0; k < n && k < 9; k++) info[k] = v[k];
    return GSR_OK;
}

int gsr_mesh_near_mask(int64_t P, const float *xyz, const gsr_mesh_index *index, double max_distance, const float *box,
                       uint8_t *out_mask, void *stream) {
    MeshGrid g{};
    float T = 0.f, reach = 0.f, ext = 0.f;
    if (P < 0 || (index && !mesh_grid_of(index, &g)) || (index && !gt_thresholds(max_distance, &T, &reach)) ||
        (P > 0 && (!xyz || !out_mask))) {
        set_last_error("gsr_mesh_near_mask: bad size, index, max_distance or NULL pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return GSR_OK;
    if (index) {
        // a reach above the one the boxes were grown by: search the cells within the difference
        const double need = (double)reach * (1.0 + 1.0 / 1048576.0) - (double)index->reach_b;
        if (need > 0.0) {
            ext = (float)need;
            if ((double)ext < need) ext = std::nextafterf(ext, INFINITY);
        }
    }
    CropBox cb{};
    if (box) cb = CropBox{box[0], box[1], box[2], box[3], 1};
    hipLaunchKernelGGL(mesh_near_mask_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), P, xyz, g, index ? 1 : 0, T, reach, ext, cb, out_mask);
    return launched("gsr_mesh_near_mask");
}

size_t gsr_voxel_mean_scratch_bytes(int64_t P) {
    if (P < 1 || P >= (1LL << 31)) return 0;
    return vox_carve(nullptr, (size_t)P).total;
}

int gsr_voxel_mean(int64_t P, const float *xyz, const float *colors, const uint8_t *keep_mask, double voxel_size,
                   void *scratch, float *out_xyz, float *out_colors, int32_t *out_count, int64_t *n_out, void *stream) {
    if (P < 0 || P >= (1LL << 31) || !n_out || !(voxel_size > 0.0) || !std::isfinite(voxel_size) ||
        (P > 0 && (!xyz || !scratch || !out_xyz || !out_count || (colors && !out_colors)))) {
        set_last_error("gsr_voxel_mean: bad size, voxel_size or NULL pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    *n_out = 0;
    if (P == 0) return GSR_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const VoxScratch sc = vox_carve(scratch, (size_t)P);
    const unsigned blocks = (unsigned)(((size_t)P + 255) / 256);
    auto device_error = [&](const char *what, hipError_t e) {
        set_last_error(std::string("gsr_voxel_mean: ") + what + ": " + hipGetErrorString(e));
        return GSR_ERR_DEVICE;
    };

    // 1. the kept points' bounding box (exact in fp32, widened below) and their number
    hipLaunchKernelGGL(vox_words_init_kernel, dim3(1), dim3(64), 0, s, sc.words);
    launch_bbox(P, xyz, keep_mask, sc.words, s);
    uint32_t hw[kBBoxWords];
    hipError_t e = hipMemcpyAsync(hw, sc.words, sizeof(hw), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("bounding box", e);
    if (hw[kBBoxFlags]) {
        set_last_error("gsr_voxel_mean: a kept point has a NaN or Inf coordinate");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const uint32_t K = hw[kBBoxKept];
    if (K == 0) return GSR_OK;

    // 2. the voxel grid and the key layout
    VoxGrid g{};
    g.s = voxel_size;
    int bits[3];
    for (int k = 0; k < 3; k++) {
        const double lo = (double)ord2f(hw[k]), hi = (double)ord2f(hw[3 + k]);
        g.o[k] = lo - voxel_size / 2.0;
        const double top = vox_coord(hi, g.o[k], g.s);  // the largest coordinate: vox_coord is monotone in p
        if (!(top >= 0.0) || !(top <= 2147483646.0)) {
            set_last_error("gsr_voxel_mean: voxel_size too small for the cloud: an axis needs more than 2^31 - 1 voxels");
            return GSR_ERR_INVALID_ARGUMENT;
        }
        bits[k] = bits_for((uint64_t)top + 1);
    }
    if (bits[0] + bits[1] + bits[2] > 63) {
        set_last_error("gsr_voxel_mean: voxel_size too small for the cloud: the three voxel coordinates need more than "
                       "63 key bits");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    g.bits_x = bits[0];
    g.bits_xy = bits[0] + bits[1];
    const int voxel_bits = bits[0] + bits[1] + bits[2];
    g.drop_key = 1ull << voxel_bits;

    // 3. keys, the stable sort (input order inside a voxel), the voxels' first positions
    hipLaunchKernelGGL(vox_key_kernel, dim3(blocks), dim3(256), 0, s, P, xyz, keep_mask, g, sc.key_in, sc.idx_in);
    e = sort_pairs64(sc.tmp, sc.tmp_bytes, sc.key_in, sc.key_out, sc.idx_in, sc.idx_out, (size_t)P, voxel_bits + 1, s);
    if (e != hipSuccess) return device_error("sort", e);
    uint64_t *run_key = sc.key_in;
    uint32_t *run_start = sc.idx_in, *n_runs = sc.words + 8;
    e = key_runs(sc.tmp, sc.tmp_bytes, sc.key_out, (size_t)K, run_key, run_start, n_runs, s);
    uint32_t nv = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&nv, n_runs, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("voxel table", e);
    if (nv < 1 || nv > K) {
        set_last_error("gsr_voxel_mean: voxel table: impossible voxel count");
        return GSR_ERR_DEVICE;
    }

    // 4. the means
    hipLaunchKernelGGL(vox_mean_kernel, dim3((nv + 255) / 256), dim3(256), 0, s, nv, K, run_start, sc.idx_out, xyz,
                       colors, out_xyz, colors ? out_colors : nullptr, out_count);
    e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return device_error("means", e);
    *n_out = (int64_t)nv;
    return GSR_OK;
}

}  // extern "C"
