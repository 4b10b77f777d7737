// cell_grid.hip -- the host side of the sparse cell grid (grid_cell.h) and the bounding-box reduction
// every stage that orders points by position starts with (launch_bbox, gsr_launch.h).
#include <cfloat>
#include <cmath>
#include <string>

#include "grid_cell.h"
#include "gsr_launch.h"

namespace gsr {
namespace {

// fminf / fmaxf drop a NaN, so the box is that of the other coordinates; the flag carries the rest
__global__ __launch_bounds__(256) void ord_bbox_kernel(int64_t N, const float *__restrict__ p,
                                                       const uint8_t *__restrict__ keep, uint32_t *w) {
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    uint32_t kept = 0;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        if (keep != nullptr && keep[i] == 0) continue;
        kept++;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float v = p[3 * i + k];
            bad |= !isfinite(v);
            mn[k] = fminf(mn[k], v);
            mx[k] = fmaxf(mx[k], v);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        mn[k] = wave_minf(mn[k]);
        mx[k] = wave_maxf(mx[k]);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&w[kBBoxFlags], kBBoxNonFinite);
    // without a mask the count is N: one store, not an atomic per wave on the line the box's atomics share
    if (keep == nullptr && blockIdx.x == 0 && threadIdx.x == 0) w[kBBoxKept] = (uint32_t)N;
    if ((threadIdx.x & 63) == 0 && kept) {
        if (keep != nullptr) atomicAdd(&w[kBBoxKept], kept);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            atomicMin(&w[k], f2ord(mn[k]));
            atomicMax(&w[3 + k], f2ord(mx[k]));
        }
    }
}

}  // namespace

void launch_bbox(int64_t N, const float *xyz, const uint8_t *keep, uint32_t *words, hipStream_t s, int max_blocks) {
    if (N <= 0) return;
    const int64_t want = (N + 255) / 256;
    const unsigned blocks = (unsigned)(want < max_blocks ? want : max_blocks);
    hipLaunchKernelGGL(ord_bbox_kernel, dim3(blocks), dim3(256), 0, s, N, xyz, keep, words);
}

DeviceBufs::~DeviceBufs() {
    for (void *p : held_) (void)hipFree(p);
}

void *DeviceBufs::alloc_bytes(size_t bytes) {
    if (err_ != hipSuccess) return nullptr;
    void *p = nullptr;
    err_ = hipMalloc(&p, bytes ? bytes : 1);
    if (err_ != hipSuccess) return nullptr;
    held_.push_back(p);
    return p;
}

void DeviceBufs::release(void *p) {
    for (auto &h : held_)
        if (h == p) {
            (void)hipFree(p);
            h = held_.back();
            held_.pop_back();
            return;
        }
}

std::nullptr_t build_stopped(const char *who, const BuildStop &stop) {
    std::string m = std::string(who) + ": " + stop.what;
    if (stop.e != hipSuccess) m += std::string(": ") + hipGetErrorString(stop.e);
    set_last_error(m);
    return nullptr;
}

bool cell_grid_box(CellGrid *g, const uint32_t *words, float *ext) {
    *ext = 0.f;
    for (int k = 0; k < 3; k++) {
        g->lo[k] = ord2f(words[k]);
        g->hi[k] = ord2f(words[3 + k]);
        if (!std::isfinite(g->lo[k]) || !std::isfinite(g->hi[k]) || !std::isfinite(g->hi[k] - g->lo[k])) return false;
        *ext = fmaxf(*ext, g->hi[k] - g->lo[k]);
    }
    return true;
}

bool cell_grid_dims(CellGrid *g, float h, uint64_t *cells) {
    g->inv_h = 1.f / h;
    if (!std::isfinite(g->inv_h) || !(g->inv_h > 0.f)) return false;
    *cells = 1;
    for (int k = 0; k < 3; k++) {
        // the device's cell_of(hi) without the clamp; cell_of clamps to n - 1, so the two agree
        const float t = floorf((g->hi[k] - g->lo[k]) * g->inv_h);
        g->n[k] = (int32_t)fminf(fmaxf(t, 0.f), 2097150.f) + 1;
        *cells *= (uint64_t)g->n[k];
    }
    return true;
}

BuildStop sort_cell_pairs(DeviceBufs &bufs, uint64_t *key_in, uint32_t *val_in, uint32_t R, int end_bit, hipStream_t s,
                          CellTable *t) {
    *t = CellTable{};
    t->key = bufs.alloc<uint64_t>(R);
    t->values = bufs.alloc<uint32_t>(R);
    const size_t tmp_bytes = sort_pairs64_temp_bytes(R, end_bit);
    void *tmp = bufs.alloc<char>(tmp_bytes);
    if (bufs.error() != hipSuccess) return {"allocation", bufs.error()};
    hipError_t e = sort_pairs64(tmp, tmp_bytes, key_in, t->key, val_in, t->values, R, end_bit, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return {"sort", e};
    bufs.release(tmp);
    bufs.release(key_in);
    bufs.release(val_in);
    return {};
}

BuildStop finish_cell_table(DeviceBufs &bufs, uint32_t R, bool want_last, hipStream_t s, CellTable *t) {
    uint64_t *run_key = bufs.alloc<uint64_t>(R);
    uint32_t *run_start = bufs.alloc<uint32_t>(R);
    uint32_t *n_runs = bufs.alloc<uint32_t>(1);
    const size_t tmp_bytes = key_runs_temp_bytes(R);
    void *tmp = bufs.alloc<char>(tmp_bytes);
    if (bufs.error() != hipSuccess) return {"allocation", bufs.error()};
    hipError_t e = key_runs(tmp, tmp_bytes, t->key, R, run_key, run_start, n_runs, s);
    uint32_t nc = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&nc, n_runs, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return {"cell table", e};
    if (nc < 1 || nc > R) return {"cell table: impossible cell count", hipSuccess};
    if (want_last) {
        e = hipMemcpyAsync(&t->last_key, run_key + (nc - 1), 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&t->last_start, run_start + (nc - 1), 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return {"cell table", e};
    }
    bufs.release(tmp);
    bufs.release(t->key);
    bufs.release(t->values);
    bufs.release(n_runs);
    t->key = nullptr;
    t->values = nullptr;
    t->cell_key = bufs.alloc<uint64_t>(nc);
    t->cell_start = bufs.alloc<uint32_t>((size_t)nc + 1);
    if (bufs.error() != hipSuccess) return {"allocation", bufs.error()};
    e = hipMemcpyAsync(t->cell_key, run_key, (size_t)nc * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(t->cell_start, run_start, (size_t)nc * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(t->cell_start + nc, &R, 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return {"cell table copy", e};
    bufs.release(run_key);
    bufs.release(run_start);
    t->n_cells = nc;
    return {};
}

}  // namespace gsr
