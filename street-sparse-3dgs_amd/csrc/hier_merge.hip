// hier_merge.hip -- trained chunk hierarchies merged into one scene hierarchy
// (include/gsr_hier_merge.h): what the reference's pipeline runs last, as the GaussianHierarchyMerger
// tool over every chunk's hierarchy.hier_opt (scripts/full_train.py:259-282).
//
// The reference vendors no merger source and no file the tool wrote is available, so the rule is this
// project's own definition (DESIGN.md "Hierarchy merger"), a restatement of the published method's
// consolidation: each chunk keeps the Gaussians nearer to its own centre than to any other chunk's,
// and the chunk trees are joined under a new upper tree.  It is PARITY-UNPINNED against
// gaussianhierarchy; the kernels are pinned to the numpy restatement tests/hier_merge_ref.py.  In short:
//   A. ownership  a leaf belongs to the chunk whose centre is nearest in fp32 (uncontracted
//                 (dx dx + dy dy) + dz dz, ties to the lowest chunk, non-finite never wins); a
//                 chunk's leaf survives iff the chunk owns it
//   B. splicing   a node survives iff a leaf below it does; interior nodes with two surviving
//                 children are retained, those with one are spliced out
//   C. top tree   the retained roots' rows are the leaves of the builder's LBVH (its rules A, B, E
//                 with |opacity|), their stored boxes kept
//   D. layout     breadth-first ids over the top tree with each top leaf replaced by its chunk's
//                 retained tree; source[n] = {chunk, old id} or {-1, -1}
//   E. rows       retained rows and boxes are bit copies
//
// MI355X mapping.  Launches are the only ordering; no workgroup reads what another wrote in the same
// launch and nothing waits:
//   validate   a thread per input node checks its row and its parent's / children's rows against the
//              builder's layout (indices are range-checked before they are followed); the lowest
//              offending node goes to one flag word by an integer atomicMin, read by the host before
//              any kernel walks a chain
//   ownership  a thread per node, the centres staged through LDS in batches of 256
//   survive    each surviving leaf walks up and sets its ancestors' flags with a relaxed integer
//              atomicOr, stopping at the first that was set; the flags are read by later launches only
//   splice     a thread per node: retained or not, and for a retained interior node its two
//              retained descendants (a read-only walk down through the spliced nodes)
//   top        the builder's sort, topology, numbering and merge step over the C' root rows
//   numbering  the builder's frontier expansion (hier_level.h) over the joined topology
//   gather     one sweep writes the N rows (59 floats and the box, 268 B) from `source`: the bandwidth part
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/gsr.h"
#include "../../include/gsr_hier_build.h"
#include "../../include/gsr_hier_merge.h"
#include "gsr_launch.h"
#include "hier_level.h"

namespace gsr {
namespace {

constexpr int64_t kMaxNodes = 2147483647;
constexpr int kThreads = 256;
constexpr int kBatch = GSR_HIER_MERGE_CENTRE_BATCH;

// the chunk of input node g: the largest c with first[c] <= g
__device__ __forceinline__ int chunk_of(const int64_t *__restrict__ first, int C, int64_t g) {
    int lo = 0, hi = C - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void hm_init_kernel(uint64_t *ctl, uint64_t *kc, int *root, int64_t C, int *top_node, int64_t R) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 8) ctl[i] = i == 1 ? ~0ull : 0ull;
    if (i < C) {
        kc[i] = 0ull;
        root[i] = -1;
    }
    if (i < R) top_node[i] = -1;
}

// Every row against the builder's layout.  Another row is read only at an index that
// was range-checked first.  ctl[1]: the lowest offending input node.
__global__ __launch_bounds__(kThreads) void hm_validate_kernel(int64_t T, int C, const int64_t *__restrict__ first,
                                                               const int *__restrict__ nodes, uint64_t *ctl) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= T) return;
    const int c = chunk_of(first, C, g);
    const int64_t base = first[c], Nc = first[c + 1] - base, n = g - base;
    const int *r = nodes + 7 * g;
    bool bad = (int64_t)r[2] != n;
    if (n == 0) {
        bad |= r[0] != 0 || r[1] != -1;
    } else {
        const int64_t p = r[1];
        if (p < 0 || p >= n) {
            bad = true;
        } else {
            const int *pr = nodes + 7 * (base + p);
            bad |= pr[6] != 2 || !((int64_t)pr[5] == n || (int64_t)pr[5] == n - 1) || r[0] != pr[0] + 1;
        }
        bad |= r[0] < nodes[7 * (g - 1)];  // breadth-first: depths do not decrease
    }
    const bool leaf = r[3] == 1 && r[4] == 0 && r[5] == -1 && r[6] == 0;
    if (!leaf) {
        const int64_t fc = r[5];
        if (r[3] != 0 || r[4] != 1 || r[6] != 2 || fc <= n || fc + 1 >= Nc) bad = true;
        else bad |= (int64_t)nodes[7 * (base + fc) + 1] != n || (int64_t)nodes[7 * (base + fc + 1) + 1] != n;
    }
    if (bad) atomicMin(reinterpret_cast<unsigned long long *>(ctl + 1), (unsigned long long)g);
}

// Rule A.  flag[g] = 1 for a leaf its own chunk owns, else 0 (interior nodes too: the survive
// launch's starting state).  The build's -ffp-contract=off keeps the products and sums apart.
__global__ __launch_bounds__(kThreads) void hm_own_kernel(int64_t T, int C, const int64_t *__restrict__ first,
                                                          const float *__restrict__ centres,
                                                          const int *__restrict__ nodes, const float *__restrict__ xyz,
                                                          uint32_t *__restrict__ flag) {
    __shared__ float s_c[3 * kBatch];
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool leaf = g < T && nodes[7 * g + 6] == 0;
    float x = 0.f, y = 0.f, z = 0.f;
    if (leaf) {
        x = xyz[3 * g];
        y = xyz[3 * g + 1];
        z = xyz[3 * g + 2];
    }
    float best = __uint_as_float(0x7f800000u);  // +inf: a NaN or infinite d2 never wins
    int owner = -1;
    for (int c0 = 0; c0 < C; c0 += kBatch) {
        const int nb = min(kBatch, C - c0);
        __syncthreads();  // the previous batch's reads are done
        for (int i = threadIdx.x; i < 3 * nb; i += kThreads) s_c[i] = centres[3 * (int64_t)c0 + i];
        __syncthreads();
        if (leaf) {
            for (int k = 0; k < nb; k++) {
                const float dx = x - s_c[3 * k], dy = y - s_c[3 * k + 1], dz = z - s_c[3 * k + 2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < best) {
                    best = d2;
                    owner = c0 + k;
                }
            }
        }
    }
    if (g < T) flag[g] = leaf && owner == chunk_of(first, C, g) ? 1u : 0u;
}

// Rule B's survival.  A leaf's flag is read by its own thread only; interior flags are touched by
// atomicOr only, and read by later launches.  kc[c]: the chunk's surviving leaves (integer atomics).
__global__ __launch_bounds__(kThreads) void hm_survive_kernel(int64_t T, int C, const int64_t *__restrict__ first,
                                                              const int *__restrict__ nodes, uint32_t *flag,
                                                              uint64_t *kc) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool alive = g < T && nodes[7 * g + 6] == 0 && flag[g] != 0u;
    const int c = alive ? chunk_of(first, C, g) : -1;
    // one add per wave where its surviving leaves share a chunk (all but the waves across a chunk's
    // end): millions of single adds to C addresses would serialise
    const unsigned long long m = __ballot(alive);
    if (m == 0ull) return;  // wave-uniform
    const int leader = __ffsll((long long)m) - 1;
    const int c0 = __shfl(c, leader, kWave);
    if (__all(!alive || c == c0)) {
        if ((int)(threadIdx.x & (kWave - 1)) == leader)
            atomicAdd(reinterpret_cast<unsigned long long *>(kc + c0), (unsigned long long)__popcll(m));
    } else if (alive) {
        atomicAdd(reinterpret_cast<unsigned long long *>(kc + c), 1ull);
    }
    if (!alive) return;
    const int64_t base = first[c];
    int64_t p = nodes[7 * g + 1];  // validated: -1, or in [0, n) with parent[p] < p
    while (p >= 0) {
        if (atomicOr(&flag[base + p], 1u) & 1u) break;
        p = nodes[7 * (base + p) + 1];
    }
}

// the retained node at or below surviving node x (chunk-local ids): down through the nodes with
// one surviving child.  Validated: a child's id is larger than its parent's and within the chunk.
__device__ __forceinline__ int64_t hm_down(const int *__restrict__ nodes, const uint32_t *__restrict__ flag, int64_t base,
                                           int64_t x) {
    for (;;) {
        const int *r = nodes + 7 * (base + x);
        if (r[6] == 0) return x;
        const int64_t a = r[5];
        const bool sa = flag[base + a] != 0u, sb = flag[base + a + 1] != 0u;
        if (sa && sb) return x;
        x = sa ? a : a + 1;
    }
}

// Rule B's splicing.  ret[g]: 0 not retained, 1 a retained leaf, 2 a retained interior node, whose
// two retained descendants (input node ids, lower old id first) go to ekids[g].  root[c]: r_c.
__global__ __launch_bounds__(kThreads) void hm_splice_kernel(int64_t T, int C, const int64_t *__restrict__ first,
                                                             const int *__restrict__ nodes,
                                                             const uint32_t *__restrict__ flag, uint8_t *__restrict__ ret,
                                                             int2 *__restrict__ ekids, int *__restrict__ root) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= T) return;
    uint8_t kind = 0;
    if (flag[g] != 0u) {
        const int c = chunk_of(first, C, g);
        const int64_t base = first[c], n = g - base;
        const int *r = nodes + 7 * g;
        if (r[6] == 0) {
            kind = 1;
        } else {
            const int64_t a = r[5];
            if (flag[base + a] != 0u && flag[base + a + 1] != 0u) {
                kind = 2;
                const int64_t x = hm_down(nodes, flag, base, a), y = hm_down(nodes, flag, base, a + 1);
                ekids[g] = make_int2((int)(base + (x < y ? x : y)), (int)(base + (x < y ? y : x)));  // lower old id first
            }
        }
        if (n == 0) root[c] = (int)(base + hm_down(nodes, flag, base, 0));
    }
    ret[g] = kind;
}

// ---- C. top tree -----------------------------------------------------------------------------

__global__ void hm_top_xyz_kernel(int Ca, const int *__restrict__ active, const int *__restrict__ root,
                                  const float *__restrict__ xyz, float *__restrict__ txyz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Ca) return;
    const int64_t g = root[active[i]];
#pragma unroll
    for (int k = 0; k < 3; k++) txyz[3 * i + k] = xyz[3 * g + k];
}

struct InRows {
    const float *xyz, *ls, *rot, *op, *shs, *boxes;
};

__device__ __forceinline__ void copy_row(const InRows &in, int64_t r, const HierRows &out, int64_t n) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        out.xyz[3 * n + k] = in.xyz[3 * r + k];
        out.ls[3 * n + k] = in.ls[3 * r + k];
    }
    reinterpret_cast<float4 *>(out.rot)[n] = reinterpret_cast<const float4 *>(in.rot)[r];
    out.op[n] = in.op[r];
    const float4 *b = reinterpret_cast<const float4 *>(in.boxes) + 2 * r;
    float4 *o = reinterpret_cast<float4 *>(out.boxes) + 2 * n;
    o[0] = b[0];
    o[1] = b[1];
}

// the top tree's leaves: bit copies of the chunk roots' rows, their stored boxes included
__global__ void hm_top_leaf_kernel(int64_t Nt, int M3, const int *__restrict__ tleaf, const int *__restrict__ active,
                                   const int *__restrict__ root, InRows in, HierRows top) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Nt || tleaf[t] < 0) return;
    const int64_t g = root[active[tleaf[t]]];
    copy_row(in, g, top, t);
    for (int j = 0; j < M3; j++) top.shs[t * M3 + j] = in.shs[g * M3 + j];
}

// ---- D. layout -------------------------------------------------------------------------------
// Ids of the joined topology: input node g -> g, top node t -> T + t (as unsigned: T + 2C' - 1 may
// pass 2^31).  A top leaf never appears: it is replaced by its chunk's r_c where its parent names it.

struct MergeTopo {
    uint32_t T;
    int C;
    const int64_t *first;
    const uint8_t *ret;
    const int2 *ekids;
    const int *tnodes, *tleaf, *active, *root;
    int *source, *top_node;
    __device__ __forceinline__ bool interior(int id) const {
        const uint32_t u = (uint32_t)id;
        return u >= T ? tnodes[7 * (int64_t)(u - T) + 6] == 2 : ret[u] == 2;
    }
    __device__ __forceinline__ int top_id(int64_t t) const {
        return tleaf[t] >= 0 ? root[active[tleaf[t]]] : (int)(T + (uint32_t)t);
    }
    __device__ __forceinline__ int2 children(int id) const {
        const uint32_t u = (uint32_t)id;
        if (u < T) return ekids[u];
        const int64_t a = tnodes[7 * (int64_t)(u - T) + 5];
        return make_int2(top_id(a), top_id(a + 1));
    }
    __device__ __forceinline__ void emit(int64_t n, int id, bool inner) const {
        const uint32_t u = (uint32_t)id;
        if (u >= T) {
            source[2 * n] = -1;
            source[2 * n + 1] = -1;
            top_node[u - T] = (int)n;
        } else {
            const int c = chunk_of(first, C, u);
            source[2 * n] = c;
            source[2 * n + 1] = (int)((int64_t)u - first[c]);
        }
    }
};

// ---- E. rows ---------------------------------------------------------------------------------

// A workgroup takes kThreads nodes: a thread per node for the small attributes and the box, then the
// lanes across the SH values.  New top nodes are left to hm_top_rows_kernel.
__global__ __launch_bounds__(kThreads) void hm_gather_kernel(int64_t N, int M3, int C, const int64_t *__restrict__ first,
                                                             const int *__restrict__ source, InRows in, HierRows out) {
    __shared__ int64_t s_row[kThreads];
    const int64_t n0 = (int64_t)blockIdx.x * kThreads, n = n0 + threadIdx.x;
    int64_t r = -1;
    if (n < N) {
        const int c = source[2 * n], old = source[2 * n + 1];
        if (c >= 0 && c < C && old >= 0 && first[c] + old < first[c + 1]) r = first[c] + old;
    }
    s_row[threadIdx.x] = r;
    if (r >= 0) copy_row(in, r, out, n);
    __syncthreads();
    for (int idx = threadIdx.x; idx < kThreads * M3; idx += kThreads) {
        const int t = idx / M3, j = idx - t * M3;
        const int64_t rr = s_row[t];
        if (rr >= 0) out.shs[(size_t)(n0 + t) * M3 + j] = in.shs[(size_t)rr * M3 + j];
    }
}

__global__ void hm_top_rows_kernel(int64_t Nt, int64_t N, int M3, const int *__restrict__ top_node, HierRows top,
                                   HierRows out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Nt) return;
    const int64_t n = top_node[t];
    if (n < 0 || n >= N) return;
    const InRows in{top.xyz, top.ls, top.rot, top.op, top.shs, top.boxes};
    copy_row(in, t, out, n);
    for (int j = 0; j < M3; j++) out.shs[n * M3 + j] = top.shs[t * M3 + j];
}

// ---- host ------------------------------------------------------------------------------------

struct MergeScratch {
    uint64_t *ctl;      // [8]: [0] a level's interior count, [1] the validation flag
    int64_t *first;     // [C + 1]
    uint64_t *kc;       // [C]
    int *root;          // [C] r_c as an input node id, -1 when K_c = 0
    int *active;        // [C] the chunks with K_c >= 1
    uint32_t *flag;     // [T] survival
    uint8_t *ret;       // [T]
    int2 *ekids;        // [T]
    int *kid;           // [T + C - 1]: the merged tree has at most that many nodes
    uint32_t *tile_sum;
    uint64_t *tile_off;
    int *tnodes;        // [(2C - 1) 7]
    int *tleaf;         // [2C - 1]
    float *txyz;        // [3C]
    void *build;        // the builder's scratch for C rows
    size_t build_bytes;
};

size_t merge_scratch(int64_t C, int64_t T, MergeScratch *sc, char *base) {
    Carve cv(base);
    const size_t c = (size_t)C, t = (size_t)T, nt = (size_t)hlevel::level_tiles((T + C) / 2 + 1);
    MergeScratch m{};
    m.build_bytes = gsr_hier_build_scratch_bytes(C);
    m.ctl = cv.take<uint64_t>(64);
    m.first = cv.take<int64_t>(8 * (c + 1));
    m.kc = cv.take<uint64_t>(8 * c);
    m.root = cv.take<int>(4 * c);
    m.active = cv.take<int>(4 * c);
    m.flag = cv.take<uint32_t>(4 * t);
    m.ret = cv.take<uint8_t>(t);
    m.ekids = cv.take<int2>(8 * t);
    m.kid = cv.take<int>(4 * (t + c));
    m.tile_sum = cv.take<uint32_t>(4 * nt);
    m.tile_off = cv.take<uint64_t>(8 * nt);
    m.tnodes = cv.take<int>(28 * (2 * c - 1));
    m.tleaf = cv.take<int>(4 * (2 * c - 1));
    m.txyz = cv.take<float>(12 * c);
    m.build = cv.take(m.build_bytes);
    if (sc) *sc = m;
    return cv.off;
}

HierRows top_rows_of(float *top, int64_t C, int M) {
    const size_t R = (size_t)(2 * C - 1);
    return HierRows{top + 12 * R, top + 15 * R, top + 8 * R, top + 18 * R, top + 19 * R, top};
}

int fail_merge(int code, const std::string &m) {
    set_last_error("gsr_hier_merge: " + m);
    return code;
}

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
dim3 blocks_of(int64_t n, int per) { return dim3((unsigned)std::max<int64_t>((n + per - 1) / per, 1)); }

thread_local float t_stage_ms[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_hier_merge_scratch_bytes(int64_t C, int64_t total_nodes) {
    if (C < 1 || total_nodes < C || total_nodes > kMaxNodes) return 0;
    return merge_scratch(C, total_nodes, nullptr, nullptr) + 256;
}

size_t gsr_hier_merge_top_floats(int64_t C, int M) {
    if (C < 1 || C > kMaxNodes || M < 1 || M > 16) return 0;
    return (size_t)(2 * C - 1) * (size_t)(19 + 3 * M);
}

int gsr_hier_merge_stage_ms(float *out, int n) {
    if (!out || n <= 0) return 0;
    const int m = n < 6 ? n : 6;
    for (int k = 0; k < m; k++) out[k] = t_stage_ms[k];
    return m;
}

int gsr_hier_merge_plan(int64_t C, const int64_t *chunk_first, int M, const float *centres, const float *xyz,
                        const float *log_scales, const float *rotations, const float *opacities, const float *shs,
                        const int *nodes, const float *boxes, int64_t *leaves, int64_t *out_nodes, int *levels,
                        int *nodes_out, int *source, float *top_rows, int *top_node, void *scratch,
                        size_t scratch_bytes, void *stream) {
    if (out_nodes) *out_nodes = 0;
    if (levels) *levels = 0;
    if (C < 1 || C > kMaxNodes) return fail_merge(GSR_ERR_INVALID_ARGUMENT, "C must be at least 1");
    if (M < 1 || M > 16) return fail_merge(GSR_ERR_INVALID_ARGUMENT, "M must be in 1 .. 16");
    if (!chunk_first || !centres || !xyz || !log_scales || !rotations || !opacities || !shs || !nodes || !boxes ||
        !leaves || !out_nodes || !levels || !nodes_out || !source || !top_rows || !top_node || !scratch)
        return fail_merge(GSR_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (chunk_first[0] != 0) return fail_merge(GSR_ERR_INVALID_ARGUMENT, "chunk_first must start at 0");
    for (int64_t c = 0; c < C; c++) {
        const int64_t nc = chunk_first[c + 1] - chunk_first[c];
        if (nc < 1 || nc % 2 == 0 || chunk_first[c + 1] > kMaxNodes)
            return fail_merge(GSR_ERR_INVALID_ARGUMENT,
                              "chunk " + std::to_string(c) + ": the node count must be odd, at least 1, and the chunks' sum "
                              "at most 2^31 - 1");
    }
    if (!aligned16(rotations) || !aligned16(boxes) || !aligned16(top_rows))
        return fail_merge(GSR_ERR_INVALID_ARGUMENT, "rotations, boxes and top_rows must be 16-byte aligned");
    const int64_t T = chunk_first[C];
    if (scratch_bytes < merge_scratch(C, T, nullptr, nullptr) + 256)
        return fail_merge(GSR_ERR_INVALID_ARGUMENT, "scratch too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MergeScratch sc;
    (void)merge_scratch(C, T, &sc, reinterpret_cast<char *>(align_up(reinterpret_cast<uintptr_t>(scratch), 256)));
    const int M3 = 3 * M, Ci = (int)C;
    const int64_t R = 2 * C - 1;

    hipEvent_t ev[6] = {};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 6 && e == hipSuccess; k++) e = hipEventCreate(&ev[k]);
    const auto done = [&](int code, const std::string &m) {
        for (int k = 0; k < 6; k++)
            if (ev[k]) (void)hipEventDestroy(ev[k]);
        return code == GSR_OK ? GSR_OK : fail_merge(code, m);
    };
    const auto dev_fail = [&](const char *what, hipError_t err) {
        return done(GSR_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(err));
    };
    if (e != hipSuccess) return dev_fail("events", e);

    // validation, and A. ownership (which follows no index)
    (void)hipEventRecord(ev[0], s);
    e = hipMemcpyAsync(sc.first, chunk_first, 8 * (size_t)(C + 1), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return dev_fail("chunk offsets", e);
    hipLaunchKernelGGL(hm_init_kernel, blocks_of(std::max<int64_t>(R, 8), kThreads), dim3(kThreads), 0, s, sc.ctl, sc.kc,
                       sc.root, C, top_node, R);
    hipLaunchKernelGGL(hm_validate_kernel, blocks_of(T, kThreads), dim3(kThreads), 0, s, T, Ci, sc.first, nodes, sc.ctl);
    hipLaunchKernelGGL(hm_own_kernel, blocks_of(T, kThreads), dim3(kThreads), 0, s, T, Ci, sc.first, centres, nodes, xyz,
                       sc.flag);
    e = hipGetLastError();
    uint64_t bad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, sc.ctl + 1, sizeof(bad), hipMemcpyDeviceToHost, s);
    (void)hipEventRecord(ev[1], s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return dev_fail("validation", e);
    if (bad != ~0ull) {
        const int64_t c = std::upper_bound(chunk_first, chunk_first + C + 1, (int64_t)bad) - chunk_first - 1;
        return done(GSR_ERR_INVALID_ARGUMENT, "chunk " + std::to_string(c) + ": node " +
                                                  std::to_string((int64_t)bad - chunk_first[c]) +
                                                  " breaks the hierarchy layout (one Gaussian per node, breadth-first ids, "
                                                  "parent < id, two adjacent children)");
    }

    // B. survival
    hipLaunchKernelGGL(hm_survive_kernel, blocks_of(T, kThreads), dim3(kThreads), 0, s, T, Ci, sc.first, nodes, sc.flag,
                       sc.kc);
    (void)hipEventRecord(ev[2], s);
    // B. splicing
    hipLaunchKernelGGL(hm_splice_kernel, blocks_of(T, kThreads), dim3(kThreads), 0, s, T, Ci, sc.first, nodes, sc.flag,
                       sc.ret, sc.ekids, sc.root);
    e = hipGetLastError();
    std::vector<uint64_t> kc((size_t)C);
    if (e == hipSuccess) e = hipMemcpyAsync(kc.data(), sc.kc, 8 * (size_t)C, hipMemcpyDeviceToHost, s);
    (void)hipEventRecord(ev[3], s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return dev_fail("survival", e);
    std::vector<int> active;
    int64_t K = 0;
    for (int64_t c = 0; c < C; c++) {
        leaves[c] = (int64_t)kc[(size_t)c];
        K += leaves[c];
        if (leaves[c] > 0) active.push_back((int)c);
    }
    if (K == 0) return done(GSR_ERR_INVALID_ARGUMENT, "no chunk has a surviving leaf");
    const int64_t Ca = (int64_t)active.size(), Nt = 2 * Ca - 1, N = 2 * K - 1;
    e = hipMemcpyAsync(sc.active, active.data(), 4 * (size_t)Ca, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return dev_fail("active chunks", e);

    // C. top tree: the builder's rules A, B, C and E over the C' root rows
    const HierRows top = top_rows_of(top_rows, C, M);
    const InRows in{xyz, log_scales, rotations, opacities, shs, boxes};
    if (Ca > 1) {
        hipLaunchKernelGGL(hm_top_xyz_kernel, blocks_of(Ca, kThreads), dim3(kThreads), 0, s, (int)Ca, sc.active, sc.root,
                           xyz, sc.txyz);
        std::vector<int64_t> tstart;
        const int rc = hier_build_tree(Ca, sc.txyz, sc.tnodes, sc.tleaf, &tstart, sc.build, sc.build_bytes, s,
                                       "gsr_hier_merge: top tree");
        if (rc != GSR_OK) {
            const std::string m = gsr_last_error();
            (void)done(GSR_OK, "");
            set_last_error(m);
            return rc;
        }
        hipLaunchKernelGGL(hm_top_leaf_kernel, blocks_of(Nt, kThreads), dim3(kThreads), 0, s, Nt, M3, sc.tleaf, sc.active,
                           sc.root, in, top);
        for (int d = (int)tstart.size() - 3; d >= 0; d--)
            hier_build_merge_level(Nt, tstart[d], tstart[d + 1], M3, sc.tnodes, top, true, s);
    }
    (void)hipEventRecord(ev[4], s);

    // D. layout
    const MergeTopo topo{(uint32_t)T, Ci, sc.first, sc.ret, sc.ekids, sc.tnodes, sc.tleaf, sc.active, sc.root, source, top_node};
    std::vector<int64_t> level_start;
    std::string why;
    int root_id = (int)(uint32_t)T;  // top node 0
    if (Ca == 1) {
        e = hipMemcpyAsync(&root_id, sc.root + active[0], sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return dev_fail("root", e);
    }
    e = hlevel::expand_levels(topo, K, root_id, sc.kid, nodes_out, sc.tile_sum, sc.tile_off, sc.ctl, s, &level_start, &why);
    if (e != hipSuccess) return dev_fail("numbering", e);
    if (!why.empty()) return done(GSR_ERR_DEVICE, why);
    (void)hipEventRecord(ev[5], s);
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return dev_fail("numbering", e);
    const int order[5][2] = {{0, 1}, {1, 2}, {2, 3}, {4, 5}, {3, 4}};  // ownership, survive, splice, numbering, top
    for (int k = 0; k < 5; k++) {
        float ms = 0.f;
        t_stage_ms[k] = hipEventElapsedTime(&ms, ev[order[k][0]], ev[order[k][1]]) == hipSuccess ? ms : 0.f;
    }
    t_stage_ms[5] = 0.f;
    *out_nodes = N;
    *levels = (int)level_start.size() - 1;
    return done(GSR_OK, "");
}

int gsr_hier_merge_gather(int64_t C, int M, int64_t N, const float *xyz, const float *log_scales,
                          const float *rotations, const float *opacities, const float *shs, const float *boxes,
                          const int *source, const float *top_rows, const int *top_node, float *out_xyz,
                          float *out_log_scales, float *out_rotations, float *out_opacities, float *out_shs,
                          float *out_boxes, const void *scratch, size_t scratch_bytes, void *stream) {
    if (C < 1 || C > kMaxNodes) return fail_merge(GSR_ERR_INVALID_ARGUMENT, "C must be at least 1");
    if (M < 1 || M > 16) return fail_merge(GSR_ERR_INVALID_ARGUMENT, "M must be in 1 .. 16");
    if (N < 1 || N > kMaxNodes || N % 2 == 0) return fail_merge(GSR_ERR_INVALID_ARGUMENT, "N must be odd, in 1 .. 2^31 - 1");
    if (!xyz || !log_scales || !rotations || !opacities || !shs || !boxes || !source || !top_rows || !top_node ||
        !out_xyz || !out_log_scales || !out_rotations || !out_opacities || !out_shs || !out_boxes || !scratch)
        return fail_merge(GSR_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (!aligned16(rotations) || !aligned16(boxes) || !aligned16(top_rows) || !aligned16(out_rotations) || !aligned16(out_boxes))
        return fail_merge(GSR_ERR_INVALID_ARGUMENT, "rotations, boxes, top_rows, out_rotations and out_boxes must be 16-byte aligned");
    if (scratch_bytes < merge_scratch(C, C, nullptr, nullptr) + 256)
        return fail_merge(GSR_ERR_INVALID_ARGUMENT, "scratch too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MergeScratch sc;  // only the head (the chunk offsets) is read: its place does not depend on T
    (void)merge_scratch(C, C, &sc,
                        reinterpret_cast<char *>(align_up(reinterpret_cast<uintptr_t>(const_cast<void *>(scratch)), 256)));
    hipEvent_t ev[2] = {};
    hipError_t e = hipEventCreate(&ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&ev[1]);
    const auto done = [&](int code, const std::string &m) {
        for (int k = 0; k < 2; k++)
            if (ev[k]) (void)hipEventDestroy(ev[k]);
        return code == GSR_OK ? GSR_OK : fail_merge(code, m);
    };
    if (e != hipSuccess) return done(GSR_ERR_DEVICE, std::string("events: ") + hipGetErrorString(e));
    const int M3 = 3 * M;
    const InRows in{xyz, log_scales, rotations, opacities, shs, boxes};
    const HierRows out{out_xyz, out_log_scales, out_rotations, out_opacities, out_shs, out_boxes};
    const HierRows top = top_rows_of(const_cast<float *>(top_rows), C, M);
    (void)hipEventRecord(ev[0], s);
    hipLaunchKernelGGL(hm_gather_kernel, blocks_of(N, kThreads), dim3(kThreads), 0, s, N, M3, (int)C, sc.first, source, in, out);
    hipLaunchKernelGGL(hm_top_rows_kernel, blocks_of(2 * C - 1, kThreads), dim3(kThreads), 0, s, 2 * C - 1, N, M3, top_node,
                       top, out);
    e = hipGetLastError();
    (void)hipEventRecord(ev[1], s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return done(GSR_ERR_DEVICE, std::string("gather: ") + hipGetErrorString(e));
    float ms = 0.f;
    t_stage_ms[5] = hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess ? ms : 0.f;
    return done(GSR_OK, "");
}

}  // extern "C"
