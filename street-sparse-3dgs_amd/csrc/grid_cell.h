// grid_cell.h -- the sparse cell grid under the two spatial indexes (gtcloud.hip's cloud index,
// lidar.hip's mesh index): a uniform grid whose occupied cells sit in a sorted table of 64-bit keys,
// each cell one contiguous run of items.  Here: the grid struct, the cell coordinate and key, the
// query walk, the host build of the cell table (cell_grid.hip), and the order-preserving
// float <-> uint map and wave reductions of the bounding-box reduction (launch_bbox, gsr_launch.h).
//
// Exactness of a query.  Let an item be able to satisfy the predicate for the query
// point p only if, per axis, some coordinate g of it has lo <= g <= hi as real numbers, where the
// caller computed [lo, hi] in fp32 around p (gtcloud.hip: p -+ reach stepped outward; lidar.hip: the
// triangle's grown box lists it, and the point's own cell or its widened range meets that box).
// cell_of is a composition of monotone non-decreasing fp32 operations and is evaluated by this one
// device function for the items at the build and for lo / hi at the query, so
// cell_of(lo) <= cell_of(g) <= cell_of(hi) whatever the rounding of each step did: a coordinate may
// be a cell off the real-number one at large coordinates, but it is off the same way on both sides.
// cell_walk visits every item of every cell of [c0, c1] on the three axes and tests each with the
// predicate itself, so "some item satisfies it" equals the all-pairs result bit for bit; an item
// listed in two cells changes nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstddef>
#include <vector>

namespace gsr {

// ---- ordered floats, wave reductions ---------------------------------------------------------

// f2ord is increasing in f as an unsigned integer (so atomicMin / atomicMax order floats); ord2f inverts it
__host__ __device__ __forceinline__ uint32_t f2ord(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float ord2f(uint32_t u) {
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// min / max over the 64 lanes, in every lane
__device__ __forceinline__ float wave_minf(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// The eight words launch_bbox reduces into: 0..2 the ordered minima, 3..5 the ordered maxima,
// 6 flags (kBBoxNonFinite; a caller may keep bits of its own above it), 7 the rows counted.
constexpr int kBBoxWords = 8, kBBoxFlags = 6, kBBoxKept = 7;
constexpr uint32_t kBBoxNonFinite = 1u;
// their initial values, by the first eight threads of the caller's own init kernel
__device__ __forceinline__ void bbox_words_init(uint32_t *w) {
    if (threadIdx.x < 3) {
        w[threadIdx.x] = 0xffffffffu;
        w[3 + threadIdx.x] = 0u;
    }
    if (threadIdx.x >= 6 && threadIdx.x < 8) w[threadIdx.x] = 0u;
}

// ---- the grid --------------------------------------------------------------------------------

struct CellGrid {
    const uint64_t *cell_key;    // ascending keys of the occupied cells
    const uint32_t *cell_start;  // n_cells + 1: first item of each cell, then the end of the last
    uint32_t n_cells;
    float lo[3], hi[3];  // the fp32 bounding box the grid spans
    float inv_h;
    int32_t n[3];  // cells per axis
};

// gtcloud.hip: what a query kernel needs of a gsr_gt_index (include/gsr_gtcloud.h)
struct GtGrid : CellGrid {
    const float4 *pts;  // the cloud in cell order (w unused); cell_start[n_cells] = G
};

// The cell coordinate along one axis: a composition of monotone non-decreasing fp32 operations, so
// v <= w gives cell_of(v) <= cell_of(w) whatever each rounding did.
__device__ __forceinline__ int cell_of(float v, float o, float inv_h, int n) {
    const float t = floorf(__fmul_rn(__fsub_rn(v, o), inv_h));
    return (int)fminf(fmaxf(t, 0.f), (float)(n - 1));
}

// (z, y, x) order: the cells x0..x1 of one (y, z) row have consecutive keys
__device__ __forceinline__ uint64_t cell_key_of(int cx, int cy, int cz, const CellGrid &g) {
    return ((uint64_t)cz * (uint64_t)g.n[1] + (uint64_t)cy) * (uint64_t)g.n[0] + (uint64_t)cx;
}

constexpr uint32_t kLaneRun = 16;  // longer runs are shared by the wave

// The query walk, a lane per query: does some item of the cells [c0, c1] satisfy hit(item, qx, qy, qz)?
// Per (y, z) row the items of cells x0..x1 are ONE run of the sorted array: one binary search of the
// cell table and a walk of at most x1 - x0 + 1 entries.  A run of up to kLaneRun items is scanned by
// its own lane (early exit at the first hit); longer runs -- a scanner's own position or a wall can
// put tens of thousands of points in one cell -- are taken one after the other by the whole wave:
// the owner's query and run are broadcast, the 64 lanes test consecutive items (coalesced) and the
// wave leaves the run at the first 64-item slice with a hit.  The row loop's trip count is
// wave-uniform (__any), so the broadcasts run with every lane active: every lane of the wave must
// call this, with search false for a lane that has nothing to look for.
template <class Hit>
__device__ __forceinline__ bool cell_walk(const CellGrid &g, const int c0[3], const int c1[3], bool search, float qx,
                                          float qy, float qz, Hit hit) {
    const int lane = threadIdx.x & 63;
    bool found = false;
    const int64_t ny = c1[1] - c0[1] + 1;
    const int64_t nrows = search ? ny * (int64_t)(c1[2] - c0[2] + 1) : 0;
    for (int64_t r = 0; __any(r < nrows && !found); r++) {
        uint32_t s = 0, e = 0;
        if (r < nrows && !found) {
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
            s = g.cell_start[a];
            e = g.cell_start[j];
        }
        if (e - s <= kLaneRun) {
            for (uint32_t j = s; j < e; j++) {
                if (hit(j, qx, qy, qz)) {
                    found = true;
                    break;
                }
            }
            s = e;
        }
        unsigned long long pending = __ballot(e > s);
        while (pending) {
            const int l = __ffsll((long long)pending) - 1;
            pending &= pending - 1;
            const float bx = __shfl(qx, l), by = __shfl(qy, l), bz = __shfl(qz, l);
            const uint32_t bs = (uint32_t)__shfl((int)s, l), be = (uint32_t)__shfl((int)e, l);
            bool any = false;
            for (uint32_t j = bs; j < be && !any; j += 64) {
                const uint32_t jj = j + lane;
                const bool h = jj < be && hit(jj, bx, by, bz);
                any = __any(h);
            }
            if (any && lane == l) found = true;
        }
    }
    return found;
}

// ---- the host build (cell_grid.hip) ----------------------------------------------------------

// The device allocations of a build: what is still held is freed when the owner goes out of scope.
class DeviceBufs {
public:
    DeviceBufs() = default;
    DeviceBufs(const DeviceBufs &) = delete;
    DeviceBufs &operator=(const DeviceBufs &) = delete;
    ~DeviceBufs();
    // n elements (at least a byte); NULL on failure, and from then on: error() keeps the first failure,
    // so a group of allocations is checked once
    template <class T>
    T *alloc(size_t n) {
        return static_cast<T *>(alloc_bytes(n * sizeof(T)));
    }
    hipError_t error() const { return err_; }
    void release(void *p);           // free now
    void disown() { held_.clear(); }  // the build succeeded: what is held belongs to the index

private:
    void *alloc_bytes(size_t bytes);
    std::vector<void *> held_;
    hipError_t err_ = hipSuccess;
};

// Why a build stopped: what != NULL; the message is "<who>: <what>: <HIP's text>", or "<who>: <what>"
// when e is hipSuccess (the data was refused).
struct BuildStop {
    const char *what = nullptr;
    hipError_t e = hipSuccess;
    explicit operator bool() const { return what != nullptr; }
};
std::nullptr_t build_stopped(const char *who, const BuildStop &stop);  // sets the thread's message; NULL

// lo / hi of the grid from the six ordered words of launch_bbox and the largest extent; false when a
// bound or an extent is not finite
bool cell_grid_box(CellGrid *g, const uint32_t *words, float *ext);
// inv_h and the cells per axis for the edge h: at most 2^21 - 1 per axis, so a 64-bit key holds the
// three coordinates.  *cells = their product; false when 1 / h is not a positive finite fp32.
bool cell_grid_dims(CellGrid *g, float h, uint64_t *cells);

struct CellTable {
    uint64_t *key;         // R sorted keys: between the two steps only
    uint32_t *values;      // R: the values in key order (stable: input order inside a cell); as key
    uint64_t *cell_key;    // n_cells: the distinct keys, ascending
    uint32_t *cell_start;  // n_cells + 1: each key's first position, then R
    uint32_t n_cells;
    uint64_t last_key;  // with want_last: the last run's key and first position
    uint32_t last_start;
};
// The cell table of R unsorted (key, value) pairs over key bits [0, end_bit), in two steps with the
// caller's gather of its items by t->values between them (queued behind the sort, it runs beside the
// run table's build).  sort_cell_pairs: key_in and val_in belong to bufs and are released after the
// sort.  finish_cell_table: the runs of equal keys, trimmed to their number, and the end sentinel;
// t->key and t->values are released.  On success bufs holds cell_key and cell_start.
BuildStop sort_cell_pairs(DeviceBufs &bufs, uint64_t *key_in, uint32_t *val_in, uint32_t R, int end_bit, hipStream_t s,
                          CellTable *t);
BuildStop finish_cell_table(DeviceBufs &bufs, uint32_t R, bool want_last, hipStream_t s, CellTable *t);

}  // namespace gsr
