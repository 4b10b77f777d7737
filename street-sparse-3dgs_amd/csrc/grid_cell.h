// grid_cell.h -- the cell coordinate of the uniform grids (gtcloud.hip's cloud index, lidar.hip's
// mesh index) and the order-preserving float <-> uint map their bounding-box reductions use.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>

namespace gsr {

// The cell coordinate along one axis: a composition of monotone non-decreasing fp32 operations, so
// v <= w gives cell_of(v) <= cell_of(w) whatever each rounding did (gtcloud.hip's exactness argument).
__device__ __forceinline__ int cell_of(float v, float o, float inv_h, int n) {
    const float t = floorf(__fmul_rn(__fsub_rn(v, o), inv_h));
    return (int)fminf(fmaxf(t, 0.f), (float)(n - 1));
}

__device__ __forceinline__ uint32_t f2ord(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float ord2f(uint32_t u) {
    const uint32_t b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

}  // namespace gsr
