// sort.hip -- rocPRIM pair sorts, key runs and scans: knn.hip's Morton order, the cell table of the
// sparse cell grid (grid_cell.h, built in cell_grid.hip for gtcloud.hip and lidar.hip), the voxel
// mean, hier_build.hip and mesh_depth.hip.  The rasterizer's depth sort is dsort.hip.  Kept in its
// own translation unit: rocPRIM's templates dominate compile time.
#include <cstring>
#include <rocprim/rocprim.hpp>
#include "gsr_launch.h"

namespace gsr {

namespace {
// rocPRIM routes radix sorts of up to 2^20 items through block-sort + 10 merge passes; for the
// P ~ 1M depth keys that is ~150 us/frame on MI355X vs a few onesweep passes.  Cap the merge path.
using OnesweepCfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                               rocprim::default_config, 8192>;

}  // namespace

size_t sort_pairs_temp_bytes(size_t n, int end_bit) {
    size_t bytes = 0;
    rocprim::radix_sort_pairs<OnesweepCfg>(nullptr, bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                           (const uint32_t *)nullptr, (uint32_t *)nullptr, n > 0 ? n : 1, 0, end_bit);
    return bytes;
}

hipError_t sort_pairs(void *tmp, size_t tmp_bytes, const uint32_t *kin, uint32_t *kout, const uint32_t *vin,
                      uint32_t *vout, size_t n, int end_bit, hipStream_t s) {
    if (n == 0) return hipSuccess;
    return rocprim::radix_sort_pairs<OnesweepCfg>(tmp, tmp_bytes, kin, kout, vin, vout, n, 0, end_bit, s);
}

// 64-bit keys (the cell keys of grid_cell.h's grids): once per index, default config
size_t sort_pairs64_temp_bytes(size_t n, int end_bit) {
    size_t bytes = 0;
    rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                              (const uint32_t *)nullptr, (uint32_t *)nullptr, n > 0 ? n : 1, 0, end_bit);
    return bytes;
}

hipError_t sort_pairs64(void *tmp, size_t tmp_bytes, const uint64_t *kin, uint64_t *kout, const uint32_t *vin,
                        uint32_t *vout, size_t n, int end_bit, hipStream_t s) {
    if (n == 0) return hipSuccess;
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, kin, kout, vin, vout, n, 0, end_bit, s);
}

size_t key_runs_temp_bytes(size_t n) {
    size_t bytes = 0;
    rocprim::unique_by_key(nullptr, bytes, (const uint64_t *)nullptr, rocprim::counting_iterator<uint32_t>(0),
                           (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, n > 0 ? n : 1);
    return bytes;
}

hipError_t key_runs(void *tmp, size_t tmp_bytes, const uint64_t *keys, size_t n, uint64_t *run_key,
                    uint32_t *run_start, uint32_t *n_runs, hipStream_t s) {
    return rocprim::unique_by_key(tmp, tmp_bytes, keys, rocprim::counting_iterator<uint32_t>(0), run_key, run_start,
                                  n_runs, n, rocprim::equal_to<uint64_t>(), s);
}

// Exclusive prefix sum of n 32-bit counts (lidar.hip's mesh index: count, scan, fill).
size_t scan_u32_temp_bytes(size_t n) {
    size_t bytes = 0;
    rocprim::exclusive_scan(nullptr, bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, n > 0 ? n : 1,
                            rocprim::plus<uint32_t>());
    return bytes;
}

hipError_t scan_u32(void *tmp, size_t tmp_bytes, const uint32_t *in, uint32_t *out, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    return rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), s);
}

}  // namespace gsr
