// hier_build.hip -- the LOD hierarchy of a trained chunk (include/gsr_hier_build.h): what the
// reference's pipeline runs as the GaussianHierarchyCreator tool between train_single.py and
// train_post.py (scripts/full_train.py:152,203-216).
//
// The gaussianhierarchy tool is not vendored in the reference, so this is a restatement of the
// published method (Kerbl et al. 2024, "A Hierarchical 3D Gaussian Representation for Real-Time
// Rendering of Very Large Datasets", sec. 5) over an LBVH, and the rule is this project's own
// definition (DESIGN.md "Hierarchy builder"); parity is pinned to the numpy restatement
// tests/hier_build_ref.py, not to the unvendored tool ("parity unpinned" against gaussianhierarchy
// itself).  In short:
//   A. order     63-bit Morton keys of the positions quantised to 2^21 cells per axis over one cube
//                (double arithmetic, every operation correctly rounded), stable sort by (key, row)
//   B. topology  Karras 2012 over the sorted leaves, delta(a, b) = clz64(key_a ^ key_b), equal keys
//                split by position: 64 + clz32(a ^ b)
//   C. layout    node ids = breadth-first positions, left child first; Gaussian row n = node n
//   D. leaves    bit copies of the input rows; box = mean +- 3 sqrt(diag(Sigma))
//   E. interior  children merged with weights w = opacity x surface (Thomsen's ellipsoid surface,
//                p = 1.6075): weighted mean and SH, mixture covariance, fp32 Jacobi for the scales
//                and the rotation, opacity = W / surface, box = union of the children's boxes
//
// MI355X mapping.  Launches are the only ordering between dependent nodes; nothing waits on another
// workgroup inside a launch:
//   sort       bounds (block reduce + ordered-uint atomics), keys, rocPRIM pair sort (sort.hip)
//   topology   one independent thread per interior range (two binary searches over the keys)
//   numbering  a frontier expansion (hier_level.h, shared with hier_merge.hip), one level per step:
//              the level's interior flags counted per 1024-node tile, the tile sums scanned by one
//              workgroup, the node rows written and the children placed at level_end + 2 rank; the
//              host reads the level's interior count (one word per level, at most 96 levels)
//   merge      the leaves' rows first, then one launch per depth, deepest first.  A level is a
//              contiguous node range and its children the contiguous range after it, so a launch is
//              a coalesced sweep with no atomics.  A workgroup takes 256 nodes: a thread per node for
//              the 20 small floats and the 3x3 Jacobi, then the workgroup's lanes across the
//              256 x 3M SH values (the bandwidth part: up to 192 B per row, two rows read per row
//              written).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/gsr.h"
#include "../../include/gsr_hier_build.h"
#include "grid_cell.h"  // ord2f, the bounding box's words
#include "gsr_launch.h"
#include "hier_level.h"

namespace gsr {
namespace {

constexpr int64_t kMaxRows = (int64_t)1 << 30;
constexpr int kThreads = 256;
constexpr float kSurfaceP = 1.6075f;
constexpr float kMinEigen = 1e-14f;
constexpr int kJacobiSweeps = 8;

// ---- A. order ------------------------------------------------------------------------------

__global__ void hb_init_kernel(uint32_t *bb, uint64_t *ctl) {
    bbox_words_init(bb);
    if (threadIdx.x < 8) ctl[threadIdx.x] = 0ull;
}

__device__ __forceinline__ uint64_t spread21(uint64_t x) {  // 21 bits -> every third bit
    x &= 0x1fffffull;
    x = (x | (x << 32)) & 0x1f00000000ffffull;
    x = (x | (x << 16)) & 0x1f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// Rule A: one cube scale for the three axes, every operation a correctly rounded double operation
// (the build's -ffp-contract=off keeps the subtraction and the product apart).
__global__ __launch_bounds__(kThreads) void hb_keys_kernel(int64_t P, const float *__restrict__ xyz,
                                                           const uint32_t *__restrict__ bb, uint64_t *__restrict__ key,
                                                           uint32_t *__restrict__ row) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    double lo[3], ext = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = (double)ord2f(bb[k]);
        ext = fmax(ext, (double)ord2f(bb[3 + k]) - lo[k]);
    }
    uint64_t code = 0;
    if (ext > 0.0) {
        const double scale = 2097152.0 / ext;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double t = floor(((double)xyz[3 * i + k] - lo[k]) * scale);
            const uint64_t q = t >= 2097151.0 ? 2097151ull : (t > 0.0 ? (uint64_t)t : 0ull);
            code |= spread21(q) << k;
        }
    }
    key[i] = code;
    row[i] = (uint32_t)i;
}

// ---- B. topology ---------------------------------------------------------------------------

// delta over the sorted leaves, -1 outside [0, P)
__device__ __forceinline__ int hb_delta(const uint64_t *__restrict__ key, int64_t P, int64_t a, uint64_t ka, int64_t b) {
    if (b < 0 || b >= P) return -1;
    const uint64_t kb = key[b];
    return ka != kb ? __clzll((long long)(ka ^ kb)) : 64 + __clz((int)((uint32_t)a ^ (uint32_t)b));
}

// Interior node i of Karras's numbering covers a range with i at one end; its children are the
// interior node or the leaf at the split.  child ids: interior j -> j, leaf j -> P - 1 + j.
__global__ __launch_bounds__(kThreads) void hb_topology_kernel(int64_t P, const uint64_t *__restrict__ key,
                                                               int2 *__restrict__ kids) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P - 1) return;
    const uint64_t ki = key[i];
    const int d = hb_delta(key, P, i, ki, i + 1) > hb_delta(key, P, i, ki, i - 1) ? 1 : -1;
    const int dmin = hb_delta(key, P, i, ki, i - d);
    int64_t lmax = 2;
    while (hb_delta(key, P, i, ki, i + lmax * d) > dmin) lmax <<= 1;  // ends: delta is -1 outside the array
    int64_t len = 0;
    for (int64_t t = lmax >> 1; t > 0; t >>= 1)
        if (hb_delta(key, P, i, ki, i + (len + t) * d) > dmin) len += t;
    const int64_t j = i + len * d;
    const int64_t f = d > 0 ? i : j, l = d > 0 ? j : i;
    // the split of [f, l]: the largest g in [f, l) with g == f or delta(f, g) > delta(f, l)
    const uint64_t kf = key[f];
    const int dnode = hb_delta(key, P, f, kf, l);
    int64_t g = f, step = l - f;
    do {
        step = (step + 1) >> 1;
        const int64_t c = g + step;
        if (c < l && hb_delta(key, P, f, kf, c) > dnode) g = c;
    } while (step > 1);
    const int64_t left = g == f ? P - 1 + g : g;
    const int64_t right = g + 1 == l ? P - 1 + g + 1 : g + 1;
    kids[i] = make_int2((int)left, (int)right);
}

// ---- C. layout -----------------------------------------------------------------------------
// The frontier expansion of hier_level.h over Karras's numbering: kid[n] is node n's id in the
// topology (interior j -> j, leaf j -> P - 1 + j).

struct BuildTopo {
    int64_t P;
    const int2 *kids;
    const uint32_t *sorted_row;
    int *leaf_rows;
    __device__ __forceinline__ bool interior(int id) const { return (int64_t)id < P - 1; }
    __device__ __forceinline__ int2 children(int id) const { return kids[id]; }
    __device__ __forceinline__ void emit(int64_t n, int id, bool inner) const {
        const int64_t leaf = (int64_t)id - (P - 1);
        leaf_rows[n] = inner || leaf >= P ? -1 : (int)sorted_row[leaf];
    }
};

// ---- D, E. attributes ----------------------------------------------------------------------

struct Sym3 {
    float xx, xy, xz, yy, yz, zz;
};

__device__ __forceinline__ float4 unit_quat(float4 q) {
    const float d = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);
    return make_float4(q.x / d, q.y / d, q.z / d, q.w / d);
}

// Sigma = R diag(s^2) R^T of a stored row: s = exp(log-scale), R from q / |q|
__device__ __forceinline__ Sym3 row_cov(float3 ls, float4 q_raw, float s[3]) {
    const Rot3 R = quat_to_rot(unit_quat(q_raw));
    s[0] = expf(ls.x);
    s[1] = expf(ls.y);
    s[2] = expf(ls.z);
    const float v0 = s[0] * s[0], v1 = s[1] * s[1], v2 = s[2] * s[2];
    Sym3 c;
    c.xx = R.m[0][0] * R.m[0][0] * v0 + R.m[0][1] * R.m[0][1] * v1 + R.m[0][2] * R.m[0][2] * v2;
    c.xy = R.m[0][0] * R.m[1][0] * v0 + R.m[0][1] * R.m[1][1] * v1 + R.m[0][2] * R.m[1][2] * v2;
    c.xz = R.m[0][0] * R.m[2][0] * v0 + R.m[0][1] * R.m[2][1] * v1 + R.m[0][2] * R.m[2][2] * v2;
    c.yy = R.m[1][0] * R.m[1][0] * v0 + R.m[1][1] * R.m[1][1] * v1 + R.m[1][2] * R.m[1][2] * v2;
    c.yz = R.m[1][0] * R.m[2][0] * v0 + R.m[1][1] * R.m[2][1] * v1 + R.m[1][2] * R.m[2][2] * v2;
    c.zz = R.m[2][0] * R.m[2][0] * v0 + R.m[2][1] * R.m[2][1] * v1 + R.m[2][2] * R.m[2][2] * v2;
    return c;
}

// Thomsen's ellipsoid surface without the 4 pi, scaled by the largest axis so that the powers stay
// in the fp32 range for small Gaussians: S(s) = m^2 S(s / m)
__device__ __forceinline__ float surface(const float s[3]) {
    const float m = fmaxf(s[0], fmaxf(s[1], s[2]));
    if (!(m > 0.f) || !(m <= FLT_MAX)) return m * m;  // 0, inf or NaN
    const float a = s[0] / m, b = s[1] / m, c = s[2] / m;
    const float t = (powf(a * b, kSurfaceP) + powf(a * c, kSurfaceP) + powf(b * c, kSurfaceP)) / 3.f;
    return m * m * powf(t, 1.f / kSurfaceP);
}

template <int p, int q>
__device__ __forceinline__ void jacobi_rotate(float (&a)[3][3], float (&v)[3][3]) {
    constexpr int r = 3 - p - q;
    const float apq = a[p][q];
    if (apq == 0.f) return;
    const float theta = (a[q][q] - a[p][p]) / (2.f * apq);
    const float t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
    const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
    a[p][p] -= t * apq;
    a[q][q] += t * apq;
    a[p][q] = a[q][p] = 0.f;
    const float arp = a[r][p], arq = a[r][q];
    a[r][p] = a[p][r] = c * arp - s * arq;
    a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float vp = v[k][p], vq = v[k][q];
        v[k][p] = c * vp - s * vq;
        v[k][q] = s * vp + c * vq;
    }
}

// Sigma = V diag(lam) V^T by cyclic Jacobi with a fixed sweep count.  V is a product of plane
// rotations from the identity: a proper rotation (det = +1) by construction.
__device__ __forceinline__ void jacobi3(const Sym3 &c, float lam[3], float (&v)[3][3]) {
    float a[3][3] = {{c.xx, c.xy, c.xz}, {c.xy, c.yy, c.yz}, {c.xz, c.yz, c.zz}};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.f : 0.f;
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        jacobi_rotate<0, 1>(a, v);
        jacobi_rotate<0, 2>(a, v);
        jacobi_rotate<1, 2>(a, v);
    }
    lam[0] = a[0][0];
    lam[1] = a[1][1];
    lam[2] = a[2][2];
}

// rotation matrix -> unit quaternion (r, x, y, z), the branch with the largest divisor
__device__ __forceinline__ float4 rot_to_quat(const float (&m)[3][3]) {
    const float tr = m[0][0] + m[1][1] + m[2][2];
    float r, x, y, z;
    if (tr > 0.f) {
        const float s = 2.f * sqrtf(tr + 1.f);
        r = 0.25f * s;
        x = (m[2][1] - m[1][2]) / s;
        y = (m[0][2] - m[2][0]) / s;
        z = (m[1][0] - m[0][1]) / s;
    } else if (m[0][0] > m[1][1] && m[0][0] > m[2][2]) {
        const float s = 2.f * sqrtf(fmaxf(1.f + m[0][0] - m[1][1] - m[2][2], 0.f));
        r = (m[2][1] - m[1][2]) / s;
        x = 0.25f * s;
        y = (m[0][1] + m[1][0]) / s;
        z = (m[0][2] + m[2][0]) / s;
    } else if (m[1][1] > m[2][2]) {
        const float s = 2.f * sqrtf(fmaxf(1.f + m[1][1] - m[0][0] - m[2][2], 0.f));
        r = (m[0][2] - m[2][0]) / s;
        x = (m[0][1] + m[1][0]) / s;
        y = 0.25f * s;
        z = (m[1][2] + m[2][1]) / s;
    } else {
        const float s = 2.f * sqrtf(fmaxf(1.f + m[2][2] - m[0][0] - m[1][1], 0.f));
        r = (m[1][0] - m[0][1]) / s;
        x = (m[0][2] + m[2][0]) / s;
        y = (m[1][2] + m[2][1]) / s;
        z = 0.25f * s;
    }
    const float d = sqrtf(r * r + x * x + y * y + z * z);
    return make_float4(r / d, x / d, y / d, z / d);
}

using Rows = HierRows;

__device__ __forceinline__ float3 load3(const float *p, int64_t i) {
    return make_float3(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}
__device__ __forceinline__ void store3(float *p, int64_t i, float3 v) {
    p[3 * i] = v.x;
    p[3 * i + 1] = v.y;
    p[3 * i + 2] = v.z;
}
__device__ __forceinline__ void store_box(float *boxes, int64_t n, float3 mn, float3 mx) {
    const float size = fmaxf(mx.x - mn.x, fmaxf(mx.y - mn.y, mx.z - mn.z));
    float4 *b = reinterpret_cast<float4 *>(boxes) + 2 * n;
    b[0] = make_float4(mn.x, mn.y, mn.z, size);
    b[1] = make_float4(mx.x, mx.y, mx.z, 0.f);
}

// D: every leaf node's row copied from its input row, and its box.  A workgroup takes kThreads
// nodes: a thread per node for the small attributes, then the lanes across the SH values.
__global__ __launch_bounds__(kThreads) void hb_leaf_kernel(int64_t N, int64_t P, int M3, const int *__restrict__ leaf_rows,
                                                           const float *__restrict__ xyz, const float *__restrict__ ls,
                                                           const float *__restrict__ rot, const float *__restrict__ op,
                                                           const float *__restrict__ shs, Rows out) {
    __shared__ int s_row[kThreads];
    const int64_t n0 = (int64_t)blockIdx.x * kThreads, n = n0 + threadIdx.x;
    int r = n < N ? leaf_rows[n] : -1;
    if ((int64_t)r >= P) r = -1;
    s_row[threadIdx.x] = r;
    if (r >= 0) {
        const float3 mu = load3(xyz, r), l = load3(ls, r);
        const float4 q = reinterpret_cast<const float4 *>(rot)[r];
        store3(out.xyz, n, mu);
        store3(out.ls, n, l);
        reinterpret_cast<float4 *>(out.rot)[n] = q;
        out.op[n] = op[r];
        float s[3];
        const Sym3 c = row_cov(l, q, s);
        const float hx = 3.f * sqrtf(c.xx), hy = 3.f * sqrtf(c.yy), hz = 3.f * sqrtf(c.zz);
        store_box(out.boxes, n, make_float3(mu.x - hx, mu.y - hy, mu.z - hz), make_float3(mu.x + hx, mu.y + hy, mu.z + hz));
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < kThreads * M3; idx += kThreads) {
        const int t = idx / M3, j = idx - t * M3;
        const int rr = s_row[t];
        if (rr >= 0) out.shs[(size_t)(n0 + t) * M3 + j] = shs[(size_t)rr * M3 + j];
    }
}

// E: the interior nodes of one level [s, e), their children (rows of the next level) complete.
__global__ __launch_bounds__(kThreads) void hb_merge_kernel(int64_t N, int64_t s, int64_t e, int M3,
                                                            const int *__restrict__ nodes, Rows out, bool abs_opacity) {
    __shared__ int s_child[kThreads];
    __shared__ float2 s_wt[kThreads];
    const int64_t n0 = s + (int64_t)blockIdx.x * kThreads, n = n0 + threadIdx.x;
    int64_t a = -1;
    if (n < e && nodes[7 * n + 6] == 2) a = nodes[7 * n + 5];
    if (a < 0 || a + 1 >= N) a = -1;
    float2 wt = make_float2(0.f, 0.f);
    if (a >= 0) {
        const int64_t b = a + 1;
        const float3 ma = load3(out.xyz, a), mb = load3(out.xyz, b);
        float sa[3], sb[3];
        const Sym3 ca = row_cov(load3(out.ls, a), reinterpret_cast<const float4 *>(out.rot)[a], sa);
        const Sym3 cb = row_cov(load3(out.ls, b), reinterpret_cast<const float4 *>(out.rot)[b], sb);
        const float oa = abs_opacity ? fabsf(out.op[a]) : out.op[a], ob = abs_opacity ? fabsf(out.op[b]) : out.op[b];
        const float wa = oa * surface(sa), wb = ob * surface(sb);
        const float W = wa + wb;
        const bool ok = W > 0.f && W <= FLT_MAX;
        const float ua = ok ? wa / W : 0.5f, ub = ok ? wb / W : 0.5f;
        wt = make_float2(ua, ub);
        const float3 mu = make_float3(ua * ma.x + ub * mb.x, ua * ma.y + ub * mb.y, ua * ma.z + ub * mb.z);
        // sum_c u_c (mu_c - mu)(mu_c - mu)^T = u_a u_b d d^T with d = mu_a - mu_b (u_a + u_b = 1),
        // which does not subtract the rounded mean from the children
        const float dx = ma.x - mb.x, dy = ma.y - mb.y, dz = ma.z - mb.z, uu = ua * ub;
        Sym3 c;
        c.xx = ua * ca.xx + ub * cb.xx + uu * dx * dx;
        c.xy = ua * ca.xy + ub * cb.xy + uu * dx * dy;
        c.xz = ua * ca.xz + ub * cb.xz + uu * dx * dz;
        c.yy = ua * ca.yy + ub * cb.yy + uu * dy * dy;
        c.yz = ua * ca.yz + ub * cb.yz + uu * dy * dz;
        c.zz = ua * ca.zz + ub * cb.zz + uu * dz * dz;
        float lam[3], v[3][3];
        jacobi3(c, lam, v);
        float sm[3];
#pragma unroll
        for (int k = 0; k < 3; k++) sm[k] = sqrtf(fmaxf(lam[k], kMinEigen));
        store3(out.xyz, n, mu);
        store3(out.ls, n, make_float3(logf(sm[0]), logf(sm[1]), logf(sm[2])));
        reinterpret_cast<float4 *>(out.rot)[n] = rot_to_quat(v);
        out.op[n] = ok ? W / surface(sm) : 0.f;
        const float4 *ba = reinterpret_cast<const float4 *>(out.boxes) + 2 * a;
        const float4 a0 = ba[0], a1 = ba[1], b0 = ba[2], b1 = ba[3];
        store_box(out.boxes, n, make_float3(fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z)),
                  make_float3(fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y), fmaxf(a1.z, b1.z)));
    }
    s_child[threadIdx.x] = (int)a;
    s_wt[threadIdx.x] = wt;
    __syncthreads();
    // consecutive interior nodes' children are consecutive rows: coalesced reads and writes
    for (int idx = threadIdx.x; idx < kThreads * M3; idx += kThreads) {
        const int t = idx / M3, j = idx - t * M3;
        const int c = s_child[t];
        if (c >= 0) {
            const float2 u = s_wt[t];
            const float *src = out.shs + (size_t)c * M3 + j;
            out.shs[(size_t)(n0 + t) * M3 + j] = u.x * src[0] + u.y * src[M3];
        }
    }
}

// ---- host ----------------------------------------------------------------------------------

struct BuildScratch {
    uint64_t *ctl;       // [8]: [0] the level's interior count
    uint32_t *bb;        // [8]: ordered-uint bounds
    uint64_t *key_in;    // [P]; kid (N ints) once the keys are sorted
    uint64_t *key;       // [P] sorted keys
    uint32_t *row_in;    // [P]
    uint32_t *row;       // [P] input row of each sorted leaf
    int2 *kids;          // [P - 1] children of each interior range
    uint32_t *tile_sum;  // [ntiles]
    uint64_t *tile_off;  // [ntiles]
    void *sort_tmp;
};

using hlevel::level_tiles;  // a level holds at most P nodes

size_t build_scratch(int64_t P, size_t sort_bytes, BuildScratch *sc, char *base) {
    Carve c(base);
    const size_t p = (size_t)P, nt = (size_t)level_tiles(P);
    BuildScratch b{};
    b.ctl = c.take<uint64_t>(8 * 8);
    b.bb = c.take<uint32_t>(kBBoxWords * 4);
    b.key_in = c.take<uint64_t>(8 * p);
    b.key = c.take<uint64_t>(8 * p);
    b.row_in = c.take<uint32_t>(4 * p);
    b.row = c.take<uint32_t>(4 * p);
    b.kids = c.take<int2>(8 * p);
    b.tile_sum = c.take<uint32_t>(4 * nt);
    b.tile_off = c.take<uint64_t>(8 * nt);
    b.sort_tmp = c.take(sort_bytes);
    if (sc) *sc = b;
    return c.off;
}

int fail_build(int code, const std::string &m) {
    set_last_error("gsr_hier_build: " + m);
    return code;
}

thread_local float t_stage_ms[4] = {0.f, 0.f, 0.f, 0.f};
thread_local hipEvent_t *t_marks = nullptr;  // gsr_hier_build's own events: [0] after the sort, [1] after the topology

}  // namespace

int hier_build_tree(int64_t P, const float *xyz, int *nodes, int *leaf_rows, std::vector<int64_t> *level_start,
                    void *scratch, size_t scratch_bytes, hipStream_t s, const char *who) {
    const auto fail = [&](int code, const std::string &m) {
        set_last_error(std::string(who) + ": " + m);
        return code;
    };
    const auto dev_fail = [&](const char *what, hipError_t err) {
        return fail(GSR_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(err));
    };
    const size_t sort_bytes = sort_pairs64_temp_bytes((size_t)P, 63);
    if (scratch_bytes < build_scratch(P, sort_bytes, nullptr, nullptr) + 256)
        return fail(GSR_ERR_INVALID_ARGUMENT, "scratch too small");
    BuildScratch sc;
    (void)build_scratch(P, sort_bytes, &sc, reinterpret_cast<char *>(align_up(reinterpret_cast<uintptr_t>(scratch), 256)));
    int *kid = reinterpret_cast<int *>(sc.key_in);  // N ints in the 2 P ints of the unsorted keys
    const auto blocks = [](int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); };

    // A. order
    hipLaunchKernelGGL(hb_init_kernel, dim3(1), dim3(64), 0, s, sc.bb, sc.ctl);
    launch_bbox(P, xyz, nullptr, sc.bb, s, 2048);
    hipLaunchKernelGGL(hb_keys_kernel, blocks(P, kThreads), dim3(kThreads), 0, s, P, xyz, sc.bb, sc.key_in, sc.row_in);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = sort_pairs64(sc.sort_tmp, sort_bytes, sc.key_in, sc.key, sc.row_in, sc.row, (size_t)P, 63, s);
    if (e != hipSuccess) return dev_fail("sort", e);
    if (t_marks) (void)hipEventRecord(t_marks[0], s);

    // B. topology
    if (P > 1) hipLaunchKernelGGL(hb_topology_kernel, blocks(P - 1, kThreads), dim3(kThreads), 0, s, P, sc.key, sc.kids);
    if (t_marks) (void)hipEventRecord(t_marks[1], s);

    // C. layout: one level per step; the root is interior 0, or the only leaf when P == 1
    const BuildTopo topo{P, sc.kids, sc.row, leaf_rows};
    std::string why;
    e = hlevel::expand_levels(topo, P, 0, kid, nodes, sc.tile_sum, sc.tile_off, sc.ctl, s, level_start, &why);
    if (e != hipSuccess) return dev_fail("numbering", e);
    if (!why.empty()) return fail(GSR_ERR_DEVICE, why);
    return GSR_OK;
}

void hier_build_merge_level(int64_t N, int64_t a, int64_t b, int M3, const int *nodes, const HierRows &rows,
                            bool abs_opacity, hipStream_t s) {
    if (b <= a) return;
    hipLaunchKernelGGL(hb_merge_kernel, dim3((unsigned)((b - a + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, N, a, b,
                       M3, nodes, rows, abs_opacity);
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_hier_build_scratch_bytes(int64_t P) {
    if (P < 1 || P > kMaxRows) return 0;
    return build_scratch(P, sort_pairs64_temp_bytes((size_t)P, 63), nullptr, nullptr) + 256;
}

int gsr_hier_build_stage_ms(float *out, int n) {
    if (!out || n <= 0) return 0;
    const int m = n < 4 ? n : 4;
    for (int k = 0; k < m; k++) out[k] = t_stage_ms[k];
    return m;
}

int gsr_hier_build(int64_t P, int M, const float *xyz, const float *log_scales, const float *rotations,
                   const float *opacities, const float *shs, float *out_xyz, float *out_log_scales,
                   float *out_rotations, float *out_opacities, float *out_shs, int *nodes, float *boxes,
                   int *leaf_rows, int *levels, void *scratch, size_t scratch_bytes, void *stream) {
    if (levels) *levels = 0;
    if (P < 1 || P > kMaxRows) return fail_build(GSR_ERR_INVALID_ARGUMENT, "P must be in 1 .. 2^30");
    if (M < 1 || M > 16) return fail_build(GSR_ERR_INVALID_ARGUMENT, "M must be in 1 .. 16");
    if (!xyz || !log_scales || !rotations || !opacities || !shs || !out_xyz || !out_log_scales || !out_rotations ||
        !out_opacities || !out_shs || !nodes || !boxes || !leaf_rows || !levels || !scratch)
        return fail_build(GSR_ERR_INVALID_ARGUMENT, "NULL pointer");
    for (const void *p : {(const void *)rotations, (const void *)out_rotations, (const void *)boxes})
        if (reinterpret_cast<uintptr_t>(p) % 16)
            return fail_build(GSR_ERR_INVALID_ARGUMENT, "rotations, out_rotations and boxes must be 16-byte aligned");
    const size_t sort_bytes = sort_pairs64_temp_bytes((size_t)P, 63);
    if (scratch_bytes < build_scratch(P, sort_bytes, nullptr, nullptr) + 256)
        return fail_build(GSR_ERR_INVALID_ARGUMENT, "scratch too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t N = 2 * P - 1;
    const Rows out{out_xyz, out_log_scales, out_rotations, out_opacities, out_shs, boxes};
    const int M3 = 3 * M;

    hipEvent_t ev[5] = {};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 5 && e == hipSuccess; k++) e = hipEventCreate(&ev[k]);
    const auto done = [&](int code, const std::string &m) {
        t_marks = nullptr;
        for (int k = 0; k < 5; k++)
            if (ev[k]) (void)hipEventDestroy(ev[k]);
        return code == GSR_OK ? GSR_OK : fail_build(code, m);
    };
    const auto dev_fail = [&](const char *what, hipError_t err) {
        return done(GSR_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(err));
    };
    if (e != hipSuccess) return dev_fail("events", e);
    const auto blocks = [](int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); };

    // A, B, C. order, topology, layout
    (void)hipEventRecord(ev[0], s);
    std::vector<int64_t> level_start;
    t_marks = &ev[1];
    const int rc = hier_build_tree(P, xyz, nodes, leaf_rows, &level_start, scratch, scratch_bytes, s, "gsr_hier_build");
    if (rc != GSR_OK) {
        const std::string m = gsr_last_error();
        (void)done(GSR_OK, "");
        set_last_error(m);
        return rc;
    }
    const int L = (int)level_start.size() - 1;
    (void)hipEventRecord(ev[3], s);

    // D, E. the leaves, then the interior nodes of each level, deepest first
    hipLaunchKernelGGL(hb_leaf_kernel, blocks(N, kThreads), dim3(kThreads), 0, s, N, P, M3, leaf_rows, xyz, log_scales,
                       rotations, opacities, shs, out);
    for (int d = L - 2; d >= 0; d--) hier_build_merge_level(N, level_start[d], level_start[d + 1], M3, nodes, out, false, s);
    e = hipGetLastError();
    (void)hipEventRecord(ev[4], s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return dev_fail("merge", e);
    for (int k = 0; k < 4; k++) {
        float ms = 0.f;
        t_stage_ms[k] = hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess ? ms : 0.f;
    }
    *levels = L;
    return done(GSR_OK, "");
}

}  // extern "C"
