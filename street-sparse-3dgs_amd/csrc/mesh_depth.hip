// mesh_depth.hip -- a chunk's depth supervision maps on the device (include/gsr_mesh_depth.h): the
// reconstructed mesh ray cast from a batch of pinhole cameras, and the 16-bit normalised inverse depth
// maps with their per-image scale / offset.  The reference does the first with an embree binary in a
// container (render_depth_gaussians) and the second with numpy on the host, image by image
// (ss_utils/depth_scripts/depth_map_to_distances.py).
//
//   cameras: a lane per camera turns qvec / tvec / intrinsics (fp64) into the fp32 record the rule
//          is stated on: R, C as hi + lo, fx, fy, cx, cy.  A camera that is not finite, or whose
//          focal lengths are not > 0, gets a NaN record: every triangle is then non-finite in its
//          space and skipped, its map is 0.
//   bin:   count -> scan -> fill -> sort, as lidar.hip's mesh index, on screen tiles instead of cells.
//          A lane per (camera, triangle) takes the triangle to camera space, drops it when no vertex
//          has z > 0 or its pixel bounds miss the frame, and counts the 16 x 16 tiles the bounds
//          touch; a scan gives its first (key, triangle) pair, key = camera T + tile (T tiles per
//          camera), and the stable rocPRIM pair sort (sort.hip) makes every tile's triangles one
//          contiguous run.  A triangle whose bounds cover more than max(4, T / 2) tiles writes ONE
//          pair under the key K T + camera: the per-camera oversize list, sorted after every tile.
//   cast:  one 256-thread workgroup per tile of every camera, a lane per pixel.  It finds its own run
//          and its camera's oversize run by binary search of the sorted keys, stages the two runs'
//          triangles through LDS 256 at a time -- the staging lane does everything that does not
//          depend on the pixel: camera space, the three ordered cross products, the normal and n.a --
//          and every lane tests every staged triangle and keeps its minimum.  The trip counts are
//          the workgroup's, no lane leaves early, there is no cross-lane operation in the loop.
//          A tile without triangles writes 0.
//
// Why the bounds are conservative.  Over the part of a triangle with z > 0, x / z is a
// linear-fractional function on a convex set: its extremes are at vertices with z > 0, or it runs off to
// +-infinity where the triangle meets the plane z = 0, towards the sign of x there.  So the bound on an
// axis is the min / max over the vertices in front, opened to +-infinity for every edge that crosses
// z = 0 at x >= 0 / x <= 0 (both when x is within rounding of 0).  The fp32 result is then grown
// outward by one pixel and 1e-5 of its size -- rounding moves it by a few 2^-24 of its size -- and
// only then cut to the frame.  The per-pixel test is the rule itself, a triangle listed for a tile it
// misses changes nothing, so the map equals the all-pairs one wherever the rule's own rounding at a
// triangle's edge is below a pixel (it is 2^-24 distance fx / edge length pixels: a millimetre edge at
// 60 m under fx = 256).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/gsr.h"
#include "../../include/gsr_mesh_depth.h"
#include "gsr_launch.h"

namespace gsr {
namespace {

constexpr int kTilePx = 16;            // a tile is kTilePx x kTilePx pixels, a lane each
constexpr int kBatch = 256;          // triangles staged per pass: one per lane, 16 KB of LDS
constexpr uint32_t kMinOverTiles = 4;  // a triangle over max(kMinOverTiles, T / 2) tiles is oversize

struct CamRec {
    float R[9];
    float c_hi[3], c_lo[3];
    float fx, fy, cx, cy;
    float pad;
};

struct Frame {
    int W, H, gx, gy;
    uint32_t T;         // tiles per camera
    uint32_t over_cap;  // more tiles than this: the oversize list
};

// ---- cameras -------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void cam_setup_kernel(int64_t K, const double *__restrict__ cams, CamRec *__restrict__ rec) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const double *c = cams + 11 * k;
    double w = c[0], x = c[1], y = c[2], z = c[3];
    const double nq = sqrt(w * w + x * x + y * y + z * z);
    w /= nq;
    x /= nq;
    y /= nq;
    z /= nq;
    double R[9] = {1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z,     2 * z * x + 2 * w * y,
                   2 * x * y + 2 * w * z,     1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                   2 * z * x - 2 * w * y,     2 * y * z + 2 * w * x,     1 - 2 * x * x - 2 * y * y};
    const double t[3] = {c[4], c[5], c[6]};
    double C[3];
    bool ok = nq > 0.0 && c[7] > 0.0 && c[8] > 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) C[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
#pragma unroll
    for (int i = 0; i < 9; i++) ok = ok && isfinite(R[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) ok = ok && isfinite(C[i]) && isfinite((float)C[i]);
#pragma unroll
    for (int i = 7; i < 11; i++) ok = ok && isfinite((float)c[i]);
    CamRec r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.R[i] = ok ? (float)R[i] : NAN;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        r.c_hi[i] = ok ? (float)C[i] : NAN;
        r.c_lo[i] = ok ? (float)(C[i] - (double)r.c_hi[i]) : NAN;
    }
    r.fx = ok ? (float)c[7] : NAN;
    r.fy = ok ? (float)c[8] : NAN;
    r.cx = ok ? (float)c[9] : NAN;
    r.cy = ok ? (float)c[10] : NAN;
    r.pad = 0.f;
    rec[k] = r;
}

// ---- camera space --------------------------------------------------------------------------------

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

// a = R ((v - C_hi) - C_lo)
__device__ __forceinline__ void to_camera(const CamRec &c, const float *__restrict__ v, float a[3]) {
    const float ex = __fsub_rn(__fsub_rn(v[0], c.c_hi[0]), c.c_lo[0]);
    const float ey = __fsub_rn(__fsub_rn(v[1], c.c_hi[1]), c.c_lo[1]);
    const float ez = __fsub_rn(__fsub_rn(v[2], c.c_hi[2]), c.c_lo[2]);
    a[0] = dot3(c.R[0], c.R[1], c.R[2], ex, ey, ez);
    a[1] = dot3(c.R[3], c.R[4], c.R[5], ex, ey, ez);
    a[2] = dot3(c.R[6], c.R[7], c.R[8], ex, ey, ez);
}

// triangle t in camera c's space; false (nothing usable) for a face index out of range or a vertex
// that is not finite there
__device__ __forceinline__ bool tri_camera(const CamRec &c, int64_t V, const float *__restrict__ vert,
                                           const int32_t *__restrict__ faces, int64_t t, float a[3], float b[3],
                                           float cc[3]) {
    const int32_t i0 = faces[3 * t], i1 = faces[3 * t + 1], i2 = faces[3 * t + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;
    to_camera(c, vert + 3 * (int64_t)i0, a);
    to_camera(c, vert + 3 * (int64_t)i1, b);
    to_camera(c, vert + 3 * (int64_t)i2, cc);
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; k++) fin = fin && isfinite(a[k]) && isfinite(b[k]) && isfinite(cc[k]);
    return fin;
}

// ---- binning -------------------------------------------------------------------------------------

// one vertex's part of an axis bound: p = f (x / z) + c - 0.5, the pixel coordinate in which pixel i's
// centre is i
__device__ __forceinline__ void bound_vertex(float x, float z, float f, float c, float &lo, float &hi) {
    if (z > 0.f) {
        const float p = __fsub_rn(__fadd_rn(__fmul_rn(f, __fdiv_rn(x, z)), c), 0.5f);
        lo = fminf(lo, p);
        hi = fmaxf(hi, p);
    }
}

// an edge that crosses z = 0 opens the bound towards the sign of x at the crossing
__device__ __forceinline__ void bound_edge(float xa, float za, float xb, float zb, float &lo, float &hi) {
    if ((za > 0.f) == (zb > 0.f)) return;
    const float t = __fdiv_rn(-za, __fsub_rn(zb, za));
    const float x0 = __fadd_rn(xa, __fmul_rn(t, __fsub_rn(xb, xa)));
    const float tol = __fadd_rn(__fmul_rn(1e-5f, __fadd_rn(fabsf(xa), fabsf(xb))), FLT_MIN);
    if (!(x0 < -tol)) hi = INFINITY;  // also when x0 is NaN
    if (!(x0 > tol)) lo = -INFINITY;
}

// the pixels [i0, i1] of an axis of n pixels the bound [lo, hi] may touch, grown outward; false: none
__device__ __forceinline__ bool bound_pixels(float lo, float hi, int n, int &i0, int &i1) {
    if (!(lo < (float)n + 2.f) || !(hi > -3.f)) return false;  // also +-infinity on the wrong side
    const float glo = __fsub_rn(__fsub_rn(lo, 1.f), __fmul_rn(1e-5f, fabsf(lo)));
    const float ghi = __fadd_rn(__fadd_rn(hi, 1.f), __fmul_rn(1e-5f, fabsf(hi)));
    if (glo > (float)(n - 1) || ghi < 0.f) return false;
    i0 = glo <= 0.f ? 0 : (int)floorf(glo);
    i1 = ghi >= (float)(n - 1) ? n - 1 : (int)ceilf(ghi);
    return i0 <= i1;
}

struct TileBox {
    int x0, x1, y0, y1;
    uint32_t n;  // tiles; 0: none
};

__device__ __forceinline__ TileBox tile_box(const CamRec &c, const Frame &fr, const float a[3], const float b[3],
                                            const float cc[3]) {
    TileBox tb{0, 0, 0, 0, 0};
    if (!(a[2] > 0.f) && !(b[2] > 0.f) && !(cc[2] > 0.f)) return tb;  // nothing in front of the camera
    int px0, px1, py0, py1;
    {
        float lo = INFINITY, hi = -INFINITY;
        bound_vertex(a[0], a[2], c.fx, c.cx, lo, hi);
        bound_vertex(b[0], b[2], c.fx, c.cx, lo, hi);
        bound_vertex(cc[0], cc[2], c.fx, c.cx, lo, hi);
        bound_edge(a[0], a[2], b[0], b[2], lo, hi);
        bound_edge(b[0], b[2], cc[0], cc[2], lo, hi);
        bound_edge(cc[0], cc[2], a[0], a[2], lo, hi);
        if (!bound_pixels(lo, hi, fr.W, px0, px1)) return tb;
    }
    {
        float lo = INFINITY, hi = -INFINITY;
        bound_vertex(a[1], a[2], c.fy, c.cy, lo, hi);
        bound_vertex(b[1], b[2], c.fy, c.cy, lo, hi);
        bound_vertex(cc[1], cc[2], c.fy, c.cy, lo, hi);
        bound_edge(a[1], a[2], b[1], b[2], lo, hi);
        bound_edge(b[1], b[2], cc[1], cc[2], lo, hi);
        bound_edge(cc[1], cc[2], a[1], a[2], lo, hi);
        if (!bound_pixels(lo, hi, fr.H, py0, py1)) return tb;
    }
    tb.x0 = px0 / kTilePx;
    tb.x1 = px1 / kTilePx;
    tb.y0 = py0 / kTilePx;
    tb.y1 = py1 / kTilePx;
    tb.n = (uint32_t)(tb.x1 - tb.x0 + 1) * (uint32_t)(tb.y1 - tb.y0 + 1);
    return tb;
}

// words (64-bit): 0 references, 1 of which oversize, 2 the longest walk of a tile, 3 tiles with a run
__global__ __launch_bounds__(256) void bin_count_kernel(int64_t V, const float *__restrict__ vert, int64_t F,
                                                        const int32_t *__restrict__ faces, int64_t K,
                                                        const CamRec *__restrict__ cams, Frame fr,
                                                        uint32_t *__restrict__ cnt, unsigned long long *words) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = 0, over = 0;
    if (g < K * F) {
        const int64_t k = g / F, t = g - k * F;
        const CamRec cam = cams[k];
        float a[3], b[3], cc[3];
        if (tri_camera(cam, V, vert, faces, t, a, b, cc)) {
            const TileBox tb = tile_box(cam, fr, a, b, cc);
            over = tb.n > fr.over_cap ? 1u : 0u;
            c = over ? 1u : tb.n;
        }
        cnt[g] = c;
    }
    uint32_t q = c, o = over;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        q += __shfl_xor(q, s);
        o += __shfl_xor(o, s);
    }
    if ((threadIdx.x & 63) == 0 && q) atomicAdd(&words[0], (unsigned long long)q);
    if ((threadIdx.x & 63) == 0 && o) atomicAdd(&words[1], (unsigned long long)o);
}

__global__ __launch_bounds__(256) void bin_fill_kernel(int64_t V, const float *__restrict__ vert, int64_t F,
                                                       const int32_t *__restrict__ faces, int64_t K,
                                                       const CamRec *__restrict__ cams, Frame fr,
                                                       const uint32_t *__restrict__ off, uint32_t R,
                                                       uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= K * F) return;
    const int64_t k = g / F, t = g - k * F;
    const CamRec cam = cams[k];
    float a[3], b[3], cc[3];
    if (!tri_camera(cam, V, vert, faces, t, a, b, cc)) return;
    const TileBox tb = tile_box(cam, fr, a, b, cc);
    if (tb.n == 0) return;
    uint32_t j = off[g];
    if (tb.n > fr.over_cap) {
        if (j < R) {
            key[j] = (uint64_t)K * fr.T + (uint64_t)k;
            val[j] = (uint32_t)t;
        }
        return;
    }
    for (int ty = tb.y0; ty <= tb.y1; ty++)
        for (int tx = tb.x0; tx <= tb.x1; tx++, j++) {
            if (j >= R) return;  // cannot happen: the same function counted the tiles
            key[j] = (uint64_t)k * fr.T + (uint64_t)(ty * fr.gx + tx);
            val[j] = (uint32_t)t;
        }
}

// ---- the ray cast --------------------------------------------------------------------------------

__device__ __forceinline__ bool lex_less(const float p[3], const float q[3]) {
    if (p[0] != q[0]) return p[0] < q[0];
    if (p[1] != q[1]) return p[1] < q[1];
    return p[2] < q[2];
}

__device__ __forceinline__ void cross3(const float p[3], const float q[3], float x[3]) {
    x[0] = __fsub_rn(__fmul_rn(p[1], q[2]), __fmul_rn(p[2], q[1]));
    x[1] = __fsub_rn(__fmul_rn(p[2], q[0]), __fmul_rn(p[0], q[2]));
    x[2] = __fsub_rn(__fmul_rn(p[0], q[1]), __fmul_rn(p[1], q[0]));
}

// a b - c d with the rounding error of c d put back (Kahan), as lidar.hip's normal: on a needle the
// normal is a difference of products that cancels, and the hit's distance is n.a / n.d
__device__ __forceinline__ float diff_of_products(float a, float b, float c, float d) {
    const float w = __fmul_rn(c, d);
    const float e = __fmaf_rn(-c, d, w), f = __fmaf_rn(a, b, -w);
    return __fadd_rn(f, e);
}

__device__ __forceinline__ void cross3_exact(const float p[3], const float q[3], float x[3]) {
    x[0] = diff_of_products(p[1], q[2], p[2], q[1]);
    x[1] = diff_of_products(p[2], q[0], p[0], q[2]);
    x[2] = diff_of_products(p[0], q[1], p[1], q[0]);
}

// X(p, q) from the pair in ascending order, negated when that swapped them: the two triangles that
// share the edge get exact negatives (negating X negates E exactly: rounding is symmetric)
__device__ __forceinline__ void edge_cross(const float p[3], const float q[3], float x[3]) {
    if (lex_less(q, p)) {
        cross3(q, p, x);
        x[0] = -x[0];
        x[1] = -x[1];
        x[2] = -x[2];
    } else {
        cross3(p, q, x);
    }
}

// the first position in the sorted keys[0, n) whose key is >= k
__device__ __forceinline__ uint32_t lower_bound(const uint64_t *__restrict__ keys, uint32_t n, uint64_t k) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (keys[m] < k) a = m + 1;
        else b = m;
    }
    return a;
}

__global__ __launch_bounds__(256) void mesh_raycast_kernel(int64_t V, const float *__restrict__ vert,
                                                           const int32_t *__restrict__ faces, int64_t K,
                                                           const CamRec *__restrict__ cams, Frame fr, uint32_t R,
                                                           const uint64_t *__restrict__ keys,
                                                           const uint32_t *__restrict__ vals, float tnear, float tfar,
                                                           int mode, float *__restrict__ out,
                                                           unsigned long long *words) {
    __shared__ float4 tri[kBatch][4];
    const uint32_t blk = blockIdx.x;
    const uint32_t k = blk / fr.T, tile = blk - k * fr.T;
    const int tid = threadIdx.x;
    const int ix = (int)(tile % (uint32_t)fr.gx) * kTilePx + (tid & (kTilePx - 1));
    const int iy = (int)(tile / (uint32_t)fr.gx) * kTilePx + (tid / kTilePx);
    const CamRec cam = cams[k];
    const uint64_t key = (uint64_t)k * fr.T + tile, okey = (uint64_t)K * fr.T + k;
    uint32_t s0 = 0, n0 = 0, s1 = 0, n1 = 0;
    if (R > 0) {  // block-uniform
        s0 = lower_bound(keys, R, key);
        n0 = lower_bound(keys, R, key + 1) - s0;
        s1 = lower_bound(keys, R, okey);
        n1 = lower_bound(keys, R, okey + 1) - s1;
    }
    const uint32_t total = n0 + n1;
    if (tid == 0 && total) {
        atomicMax(&words[2], (unsigned long long)total);
        if (n0) atomicAdd(&words[3], 1ull);
    }
    const float dx = __fdiv_rn(__fsub_rn(__fadd_rn((float)ix, 0.5f), cam.cx), cam.fx);
    const float dy = __fdiv_rn(__fsub_rn(__fadd_rn((float)iy, 0.5f), cam.cy), cam.fy);
    const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), 1.f));
    float best = INFINITY;
    for (uint32_t base = 0; base < total; base += kBatch) {
        const uint32_t nb = total - base < (uint32_t)kBatch ? total - base : (uint32_t)kBatch;
        __syncthreads();  // the previous batch has been read
        if ((uint32_t)tid < nb) {
            const uint32_t j = base + tid;
            const uint32_t t = vals[j < n0 ? s0 + j : s1 + (j - n0)];
            float a[3], b[3], c[3], U[3] = {0.f, 0.f, 0.f}, Vx[3] = {0.f, 0.f, 0.f}, Wx[3] = {0.f, 0.f, 0.f},
                                    n[3] = {0.f, 0.f, 0.f}, na = 0.f;
            if (tri_camera(cam, V, vert, faces, t, a, b, c)) {  // always: the binning listed it
                edge_cross(b, c, U);
                edge_cross(c, a, Vx);
                edge_cross(a, b, Wx);
                const float ab[3] = {__fsub_rn(b[0], a[0]), __fsub_rn(b[1], a[1]), __fsub_rn(b[2], a[2])};
                const float ac[3] = {__fsub_rn(c[0], a[0]), __fsub_rn(c[1], a[1]), __fsub_rn(c[2], a[2])};
                cross3_exact(ab, ac, n);
                na = dot3(n[0], n[1], n[2], a[0], a[1], a[2]);
            }
            tri[tid][0] = make_float4(U[0], U[1], U[2], Vx[0]);
            tri[tid][1] = make_float4(Vx[1], Vx[2], Wx[0], Wx[1]);
            tri[tid][2] = make_float4(Wx[2], n[0], n[1], n[2]);
            tri[tid][3] = make_float4(na, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        for (uint32_t j = 0; j < nb; j++) {  // the same address for every lane: LDS broadcasts
            const float4 q0 = tri[j][0], q1 = tri[j][1], q2 = tri[j][2];
            const float na = tri[j][3].x;
            const float U = __fadd_rn(__fadd_rn(__fmul_rn(dx, q0.x), __fmul_rn(dy, q0.y)), q0.z);
            const float Vv = __fadd_rn(__fadd_rn(__fmul_rn(dx, q0.w), __fmul_rn(dy, q1.x)), q1.y);
            const float Wv = __fadd_rn(__fadd_rn(__fmul_rn(dx, q1.z), __fmul_rn(dy, q1.w)), q2.x);
            const float nd = __fadd_rn(__fadd_rn(__fmul_rn(q2.y, dx), __fmul_rn(q2.z, dy)), q2.w);
            const bool same = (U >= 0.f && Vv >= 0.f && Wv >= 0.f) || (U <= 0.f && Vv <= 0.f && Wv <= 0.f);
            const bool some = !(U == 0.f && Vv == 0.f && Wv == 0.f);
            if (same && some && nd != 0.f) {
                const float s = __fdiv_rn(na, nd);
                const float t = __fmul_rn(s, len);
                if (s > 0.f && tnear < t && t <= tfar) best = fminf(best, mode ? s : t);
            }
        }
    }
    if (ix < fr.W && iy < fr.H) out[((size_t)k * fr.H + iy) * fr.W + ix] = best < INFINITY ? best : 0.f;
}

// ---- the encode ----------------------------------------------------------------------------------

// depth and background of one distance (gsr_mesh_depth.h); false: background
__device__ __forceinline__ bool enc_depth(float d, int quantize, double *depth) {
    if (!quantize) {
        *depth = (double)d;
        return d != 0.f;
    }
    const double mm = 1000.0 * (double)d;
    if (!(mm >= 1.0) || mm > 1048576.0) return false;
    const int sh = mm <= 65536.0 ? 2 : (mm <= 262144.0 ? 4 : 6);
    const uint32_t units = (uint32_t)(mm / (double)(1 << sh));
    *depth = (double)((uint64_t)(units & 0x3FFFu) << sh) / 1000.0;
    return true;
}

// 1 / depth of a valid pixel; false: not valid
__device__ __forceinline__ bool enc_inv(float d, int quantize, double min_depth, double max_depth, double *inv) {
    double depth;
    if (!enc_depth(d, quantize, &depth)) return false;
    if (!(depth > min_depth) || (max_depth > 0.0 && !(depth < max_depth))) return false;
    *inv = 1.0 / depth;
    return true;
}

__global__ void enc_init_kernel(int64_t K, unsigned long long *mm) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) {
        mm[2 * k] = ~0ull;
        mm[2 * k + 1] = 0ull;
    }
}

// inv > 0: the bit patterns order as the doubles do
__global__ __launch_bounds__(256) void enc_minmax_kernel(int64_t npix, const float *__restrict__ dist, int quantize,
                                                         double min_depth, double max_depth, unsigned long long *mm) {
    const int64_t k = blockIdx.y;
    const float *d = dist + (size_t)k * npix;
    unsigned long long lo = ~0ull, hi = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        double inv;
        if (enc_inv(d[i], quantize, min_depth, max_depth, &inv)) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(inv);
            lo = b < lo ? b : lo;
            hi = b > hi ? b : hi;
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long l2 = __shfl_xor(lo, s), h2 = __shfl_xor(hi, s);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0 && hi != 0ull) {
        atomicMin(&mm[2 * k], lo);
        atomicMax(&mm[2 * k + 1], hi);
    }
}

__global__ __launch_bounds__(256) void enc_write_kernel(int64_t npix, const float *__restrict__ dist, int quantize,
                                                        double min_depth, double max_depth,
                                                        const unsigned long long *__restrict__ mm,
                                                        uint16_t *__restrict__ out, double *__restrict__ so) {
    const int64_t k = blockIdx.y;
    const unsigned long long blo = mm[2 * k], bhi = mm[2 * k + 1];
    const bool any = bhi != 0ull;
    const double lo = any ? __longlong_as_double((long long)blo) : 0.0;
    const double hi = any ? __longlong_as_double((long long)bhi) : 0.0;
    const double scale = hi > lo ? hi - lo : 0.0, offset = lo;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        so[2 * k] = scale;
        so[2 * k + 1] = offset;
    }
    const float *d = dist + (size_t)k * npix;
    uint16_t *o = out + (size_t)k * npix;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        double inv;
        uint16_t u = 0;
        if (scale > 0.0 && enc_inv(d[i], quantize, min_depth, max_depth, &inv)) {
            double x = (inv - offset) / scale;
            x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
            u = (uint16_t)(x * 65535.0);
        }
        o[i] = u;
    }
}

// ---- host ----------------------------------------------------------------------------------------

struct CastScratch {
    CamRec *cams;
    uint32_t *cnt, *off;
    unsigned long long *words;
    void *tmp;
    size_t tmp_bytes, total;
};

CastScratch cast_carve(void *base, size_t K, size_t F) {
    CastScratch c{};
    Carve cv(base);
    c.cams = cv.take<CamRec>(K * sizeof(CamRec));
    c.cnt = cv.take<uint32_t>(K * F * 4);
    c.off = cv.take<uint32_t>(K * F * 4);
    c.words = cv.take<unsigned long long>(4 * sizeof(unsigned long long));
    c.tmp_bytes = scan_u32_temp_bytes(K * F);
    c.tmp = cv.take(c.tmp_bytes);
    c.total = cv.off;
    return c;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_mesh_distance_scratch_bytes(int64_t K, int64_t F) {
    if (K < 1 || F < 1 || K >= (1LL << 31) || F >= (1LL << 31) || K * F >= (1LL << 31)) return 0;
    return cast_carve(nullptr, (size_t)K, (size_t)F).total;
}

int gsr_mesh_distance_maps(int64_t V, const float *vertices, int64_t F, const int32_t *faces, int64_t K,
                           const double *cams, int W, int H, double tnear, double tfar, int mode, void *scratch,
                           float *out, int64_t *stats, void *stream) {
    const float tn = (float)tnear, tf = (float)tfar;
    if (V < 0 || F < 0 || K < 0 || W < 0 || H < 0 || W > 32768 || H > 32768 || (mode != 0 && mode != 1) ||
        !(tnear >= 0.0) || !(tfar > tnear) || !std::isfinite(tf) || K >= (1LL << 31) || F >= (1LL << 31) ||
        V >= (1LL << 31)) {
        set_last_error("gsr_mesh_distance_maps: bad size, mode, or not 0 <= tnear < tfar < Inf");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (stats)
        for (int i = 0; i < 6; i++) stats[i] = 0;
    if (K == 0 || W == 0 || H == 0) return GSR_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto device_error = [&](const char *what, hipError_t e) {
        set_last_error(std::string("gsr_mesh_distance_maps: ") + what + ": " + hipGetErrorString(e));
        return GSR_ERR_DEVICE;
    };
    if (!out) {
        set_last_error("gsr_mesh_distance_maps: NULL output");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const size_t out_bytes = (size_t)K * (size_t)H * (size_t)W * sizeof(float);
    if (F == 0) {
        const hipError_t e = hipMemsetAsync(out, 0, out_bytes, s);
        return e == hipSuccess ? GSR_OK : device_error("clear", e);
    }
    Frame fr{};
    fr.W = W;
    fr.H = H;
    fr.gx = (W + kTilePx - 1) / kTilePx;
    fr.gy = (H + kTilePx - 1) / kTilePx;
    const uint64_t T = (uint64_t)fr.gx * (uint64_t)fr.gy;
    if (K * F >= (1LL << 31) || (uint64_t)K * T >= (1ull << 31) || !vertices || !faces || !cams || !scratch || V < 1) {
        set_last_error("gsr_mesh_distance_maps: NULL pointer, no vertices, or K F or K tiles >= 2^31 (pass fewer "
                       "cameras per call)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    fr.T = (uint32_t)T;
    fr.over_cap = fr.T / 2 > kMinOverTiles ? fr.T / 2 : kMinOverTiles;
    const CastScratch sc = cast_carve(scratch, (size_t)K, (size_t)F);
    const size_t KF = (size_t)K * (size_t)F;
    const unsigned kf_blocks = (unsigned)((KF + 255) / 256);

    // stats: device events around the binning and the ray cast (none otherwise)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    auto drop_events = [&]() {
        for (hipEvent_t &x : ev)
            if (x) {
                (void)hipEventDestroy(x);
                x = nullptr;
            }
    };
    if (stats) {
        for (hipEvent_t &x : ev)
            if (hipEventCreate(&x) != hipSuccess) x = nullptr;
        if (!ev[0] || !ev[1] || !ev[2]) drop_events();
    }
    if (ev[0]) (void)hipEventRecord(ev[0], s);

    // 1. cameras, counts
    hipError_t e = hipMemsetAsync(sc.words, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) {
        drop_events();
        return device_error("clear", e);
    }
    hipLaunchKernelGGL(cam_setup_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, s, K, cams, sc.cams);
    hipLaunchKernelGGL(bin_count_kernel, dim3(kf_blocks), dim3(256), 0, s, V, vertices, F, faces, K, sc.cams, fr, sc.cnt,
                       sc.words);
    unsigned long long hw[4] = {0, 0, 0, 0};
    e = hipMemcpyAsync(hw, sc.words, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        drop_events();
        return device_error("count", e);
    }
    if (hw[0] >= (1ull << 31)) {
        drop_events();
        set_last_error("gsr_mesh_distance_maps: more than 2^31 - 1 (camera, tile, triangle) references: pass fewer "
                       "cameras per call");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const uint32_t R = (uint32_t)hw[0];
    if (R == 0) {  // nothing in any frame
        drop_events();
        e = hipMemsetAsync(out, 0, out_bytes, s);
        return e == hipSuccess ? GSR_OK : device_error("clear", e);
    }

    // 2. scan, fill, sort
    const int end_bit = std::max(1, bits_for((uint64_t)K * T + (uint64_t)K));
    const size_t sort_bytes = sort_pairs64_temp_bytes(R, end_bit);
    const size_t k8 = align_up((size_t)R * 8, 256), v4 = align_up((size_t)R * 4, 256);
    char *pairs = nullptr;
    e = hipMalloc(reinterpret_cast<void **>(&pairs), 2 * k8 + 2 * v4 + align_up(sort_bytes, 256));
    if (e != hipSuccess) {
        drop_events();
        set_last_error(std::string("gsr_mesh_distance_maps: allocation of the references: ") + hipGetErrorString(e));
        return GSR_ERR_ALLOCATION;
    }
    uint64_t *key_in = reinterpret_cast<uint64_t *>(pairs), *key = reinterpret_cast<uint64_t *>(pairs + k8);
    uint32_t *val_in = reinterpret_cast<uint32_t *>(pairs + 2 * k8), *val = reinterpret_cast<uint32_t *>(pairs + 2 * k8 + v4);
    void *sort_tmp = pairs + 2 * k8 + 2 * v4;
    auto fail = [&](const char *what, hipError_t err) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(pairs);
        drop_events();
        return device_error(what, err);
    };
    e = scan_u32(sc.tmp, sc.tmp_bytes, sc.cnt, sc.off, KF, s);
    if (e != hipSuccess) return fail("scan", e);
    e = hipMemsetAsync(val_in, 0, (size_t)R * 4, s);  // every slot is written below; a triangle number in any case
    if (e == hipSuccess) e = hipMemsetAsync(key_in, 0, (size_t)R * 8, s);
    if (e != hipSuccess) return fail("fill", e);
    hipLaunchKernelGGL(bin_fill_kernel, dim3(kf_blocks), dim3(256), 0, s, V, vertices, F, faces, K, sc.cams, fr, sc.off, R,
                       key_in, val_in);
    e = sort_pairs64(sort_tmp, sort_bytes, key_in, key, val_in, val, R, end_bit, s);
    if (e != hipSuccess) return fail("sort", e);

    // 3. the ray cast: a workgroup per tile of every camera
    if (ev[1]) (void)hipEventRecord(ev[1], s);
    hipLaunchKernelGGL(mesh_raycast_kernel, dim3((unsigned)((uint64_t)K * T)), dim3(256), 0, s, V, vertices, faces, K,
                       sc.cams, fr, R, key, val, tn, tf, mode, out, sc.words);
    e = hipGetLastError();
    if (ev[2]) (void)hipEventRecord(ev[2], s);
    if (e == hipSuccess && stats) e = hipMemcpyAsync(hw, sc.words, sizeof(hw), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail("ray cast", e);
    (void)hipFree(pairs);
    if (stats) {
        for (int i = 0; i < 4; i++) stats[i] = (int64_t)hw[i];
        float ms = 0.f;
        if (ev[0] && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) stats[4] = (int64_t)(ms * 1000.f);
        if (ev[0] && hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) stats[5] = (int64_t)(ms * 1000.f);
    }
    drop_events();
    return GSR_OK;
}

size_t gsr_depth_encode_scratch_bytes(int64_t K) {
    if (K < 1) return 0;
    return align_up((size_t)K * 16, 256) * 2;
}

int gsr_depth_encode(int64_t K, int H, int W, const float *distance, int quantize, double min_depth, double max_depth,
                     void *scratch, uint16_t *out_u16, double *scale, double *offset, void *stream) {
    if (K < 0 || H < 0 || W < 0 || K > 65535 || !(min_depth >= 0.0) || !std::isfinite(min_depth) || std::isnan(max_depth)) {
        set_last_error("gsr_depth_encode: bad size (K <= 65535), or min_depth not finite and >= 0");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (K == 0 || H == 0 || W == 0) {
        for (int64_t k = 0; k < K && scale && offset; k++) scale[k] = offset[k] = 0.0;
        return GSR_OK;
    }
    if (!distance || !scratch || !out_u16 || !scale || !offset) {
        set_last_error("gsr_depth_encode: NULL pointer");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long *mm = static_cast<unsigned long long *>(scratch);
    double *so = reinterpret_cast<double *>(static_cast<char *>(scratch) + align_up((size_t)K * 16, 256));
    const int64_t npix = (int64_t)H * W;
    const int64_t want = (npix + 256 * 8 - 1) / (256 * 8);  // about eight pixels a lane
    const unsigned bx = (unsigned)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
    const int q = quantize ? 1 : 0;
    hipLaunchKernelGGL(enc_init_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, K, mm);
    hipLaunchKernelGGL(enc_minmax_kernel, dim3(bx, (unsigned)K), dim3(256), 0, s, npix, distance, q, min_depth, max_depth, mm);
    hipLaunchKernelGGL(enc_write_kernel, dim3(bx, (unsigned)K), dim3(256), 0, s, npix, distance, q, min_depth, max_depth, mm,
                       out_u16, so);
    std::vector<double> h((size_t)K * 2);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), so, (size_t)K * 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_last_error(std::string("gsr_depth_encode: ") + hipGetErrorString(e));
        return GSR_ERR_DEVICE;
    }
    for (int64_t k = 0; k < K; k++) {
        scale[k] = h[2 * k];
        offset[k] = h[2 * k + 1];
    }
    return GSR_OK;
}

}  // extern "C"
