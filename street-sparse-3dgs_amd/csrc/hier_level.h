// hier_level.h -- the breadth-first numbering of a binary tree by frontier expansion, shared by the
// hierarchy builder (hier_build.hip) and the hierarchy merger (hier_merge.hip), and the builder's
// entry points the merger's top tree reuses (DESIGN.md "Hierarchy builder" 14.2, "Hierarchy merger").
//
// kid[n] is node n's id in the caller's topology.  A level [s, e) is expanded in three launches: the
// level's interior nodes counted per 1024-node tile, the tile sums' exclusive scan (one workgroup; the
// level's total to ctl[0], which the host reads: one word per level), and the rows of the level
// written with its children's ids, depths and parents at e + 2 rank.  Launches are the only ordering:
// no workgroup reads what another wrote in the same launch.
//
// Topo, passed by value to the kernels:
//   __device__ bool interior(int id) const        does the node have two children
//   __device__ int2 children(int id) const        their ids, left first (interior nodes only)
//   __device__ void emit(int64_t n, int id, bool interior) const   per-node extras (leaf_rows, source)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "gsr_device.h"

namespace gsr {
namespace hlevel {

constexpr int kMaxLevels = 96;  // the builder's bound: 63 key bits + 32 position bits + the root
constexpr int kThreads = 256;
constexpr int kLvlItems = 4, kLvl = kThreads * kLvlItems;  // nodes per workgroup
constexpr int kLvlWaves = kThreads / kWave;
constexpr int kScanThreads = 1024;

inline int64_t level_tiles(int64_t width) { return (width + kLvl - 1) / kLvl; }  // tiles of the widest level

static __global__ void root_kernel(int root_id, int *__restrict__ kid, int *__restrict__ nodes) {
    if (threadIdx.x == 0) {
        kid[0] = root_id;
        nodes[0] = 0;
        nodes[1] = -1;
    }
}

template <class Topo>
__global__ __launch_bounds__(kThreads) void level_count_kernel(int64_t s, int64_t e, const int *__restrict__ kid,
                                                               uint32_t *__restrict__ tile_sum, Topo topo) {
    __shared__ uint32_t s_w[kLvlWaves];
    const int64_t t0 = s + (int64_t)blockIdx.x * kLvl;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kLvlItems; k++) {
        const int64_t n = t0 + k * kThreads + threadIdx.x;
        c += n < e && topo.interior(kid[n]) ? 1u : 0u;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int k = 0; k < kLvlWaves; k++) tot += s_w[k];
        tile_sum[blockIdx.x] = tot;
    }
}

static __global__ __launch_bounds__(kScanThreads) void level_scan_kernel(int64_t ntiles,
                                                                         const uint32_t *__restrict__ tile_sum,
                                                                         uint64_t *__restrict__ tile_off,
                                                                         uint64_t *__restrict__ ctl) {
    __shared__ uint64_t s_w[kScanThreads / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    uint64_t carry = 0;
    for (int64_t b0 = 0; b0 < ntiles; b0 += kScanThreads) {
        const int64_t gi = b0 + tid;
        const uint64_t v = gi < ntiles ? tile_sum[gi] : 0ull;
        uint64_t inc = v;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint64_t u = __shfl_up(inc, o, kWave);
            if (lane >= o) inc += u;
        }
        __syncthreads();  // the previous round's reads of s_w are done
        if (lane == kWave - 1) s_w[w] = inc;
        __syncthreads();
        uint64_t before = 0, tot = 0;
        for (int k = 0; k < kScanThreads / kWave; k++) {
            before += k < w ? s_w[k] : 0ull;
            tot += s_w[k];
        }
        if (gi < ntiles) tile_off[gi] = carry + before + inc - v;
        carry += tot;
    }
    if (tid == 0) ctl[0] = carry;  // read by the host
}

template <class Topo>
__global__ __launch_bounds__(kThreads) void level_write_kernel(int64_t N, int64_t s, int64_t e, int depth,
                                                               int *__restrict__ kid,
                                                               const uint64_t *__restrict__ tile_off,
                                                               int *__restrict__ nodes, Topo topo) {
    __shared__ uint32_t s_w[kLvlWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    // thread tid holds the tile's nodes kLvlItems tid .. + kLvlItems - 1, in node order
    const int64_t n0 = s + (int64_t)blockIdx.x * kLvl + (int64_t)kLvlItems * tid;
    int id[kLvlItems];
    bool inner[kLvlItems];
    uint32_t own = 0;
#pragma unroll
    for (int k = 0; k < kLvlItems; k++) {
        id[k] = n0 + k < e ? kid[n0 + k] : 0;
        inner[k] = n0 + k < e && topo.interior(id[k]);
        own += inner[k] ? 1u : 0u;
    }
    uint32_t incl = own;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o, kWave);
        if (lane >= o) incl += t;
    }
    if (lane == kWave - 1) s_w[w] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int k = 0; k < kLvlWaves; k++) before += k < w ? s_w[k] : 0u;
    uint64_t rank = tile_off[blockIdx.x] + before + incl - own;
#pragma unroll
    for (int k = 0; k < kLvlItems; k++) {
        const int64_t n = n0 + k;
        if (n >= e) break;
        const bool interior = inner[k];
        int *row = nodes + 7 * n;  // depth and parent were written with the parent's row
        row[2] = (int)n;
        row[3] = interior ? 0 : 1;
        row[4] = interior ? 1 : 0;
        int64_t c = -1;
        if (interior) {
            c = e + 2 * (int64_t)rank;
            rank++;
            if (c + 1 >= N) c = -1;  // cannot happen in a tree of (N + 1) / 2 leaves; nothing is stored past N
        }
        row[5] = (int)c;
        row[6] = c >= 0 ? 2 : 0;
        topo.emit(n, id[k], interior);
        if (c >= 0) {
            const int2 ch = topo.children(id[k]);
            kid[c] = ch.x;
            kid[c + 1] = ch.y;
            nodes[7 * c] = depth + 1;
            nodes[7 * c + 1] = (int)n;
            nodes[7 * (c + 1)] = depth + 1;
            nodes[7 * (c + 1) + 1] = (int)n;
        }
    }
}

// The numbering of a tree of `leaves` leaves, N = 2 leaves - 1 nodes, from the root's id: nodes (N, 7)
// and the per-node extras of topo.emit; level_start receives each level's first node and N.  kid: N
// ints; tile_sum / tile_off: level_tiles(leaves) entries; ctl: one device word.  One host read per
// level.  Returns hipSuccess with *why empty, a HIP error, or hipSuccess with *why set (the topology
// is not a tree of that many leaves).
template <class Topo>
hipError_t expand_levels(const Topo &topo, int64_t leaves, int root_id, int *kid, int *nodes, uint32_t *tile_sum,
                         uint64_t *tile_off, uint64_t *ctl, hipStream_t s, std::vector<int64_t> *level_start,
                         std::string *why) {
    const int64_t N = 2 * leaves - 1;
    why->clear();
    level_start->clear();
    hipLaunchKernelGGL(root_kernel, dim3(1), dim3(64), 0, s, root_id, kid, nodes);
    int64_t ls = 0, le = 1;
    for (;;) {
        if ((int)level_start->size() >= kMaxLevels) {
            *why = "more than 96 levels";
            return hipSuccess;
        }
        const int depth = (int)level_start->size();
        level_start->push_back(ls);
        const int64_t ntiles = (le - ls + kLvl - 1) / kLvl;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(level_count_kernel<Topo>), dim3((unsigned)ntiles), dim3(kThreads), 0, s, ls, le,
                           kid, tile_sum, topo);
        hipLaunchKernelGGL(level_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, ntiles, tile_sum, tile_off, ctl);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(level_write_kernel<Topo>), dim3((unsigned)ntiles), dim3(kThreads), 0, s, N, ls,
                           le, depth, kid, tile_off, nodes, topo);
        hipError_t e = hipGetLastError();
        uint64_t interior = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&interior, ctl, sizeof(interior), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        if (interior == 0) break;
        // a level of a tree of that many leaves holds at most `leaves` nodes (the tile arrays' size) and ends within N
        if ((int64_t)interior > (N - le) / 2 || 2 * (int64_t)interior > leaves) {
            *why = "inconsistent topology";
            return hipSuccess;
        }
        ls = le;
        le += 2 * (int64_t)interior;
    }
    if (le != N) {
        *why = "inconsistent topology";
        return hipSuccess;
    }
    level_start->push_back(N);
    return hipSuccess;
}

}  // namespace hlevel

// ---- hier_build.hip's steps over device arrays, for the merger's top tree ---------------------------

struct HierRows {
    float *xyz, *ls, *rot, *op, *shs, *boxes;
};

// Rules A and B of the builder on P positions: sorted keys, the input row of each sorted leaf and the
// children of each interior range.  Scratch for P rows as gsr_hier_build_scratch_bytes(P) sizes it.
// Then rule C into nodes / leaf_rows (2 P - 1), level_start as expand_levels gives it.
// Returns 0, or a GSR error with gsr_last_error set under `who`.
int hier_build_tree(int64_t P, const float *xyz, int *nodes, int *leaf_rows, std::vector<int64_t> *level_start,
                    void *scratch, size_t scratch_bytes, hipStream_t s, const char *who);
// Rule E over the level [a, b) of rows laid out by `nodes`, the children's rows complete.
// abs_opacity: a child's weight is |o| S(s) (rows a post-optimisation has moved may store a negative
// opacity); the builder itself passes false.
void hier_build_merge_level(int64_t N, int64_t a, int64_t b, int M3, const int *nodes, const HierRows &rows,
                            bool abs_opacity, hipStream_t s);

}  // namespace gsr
