// gsr_adam.h -- the Adam update of one element: the arithmetic of optim.hip's kernels (which form
// the same expressions over their own loads), for a kernel of another file that steps an optimizer
// in its own launch (loss.hip: the exposure optimizer's step in the exposure gradient's reduction).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gsr_train.h"

namespace gsr {

// Element e of group G with gradient g.  scene/OurAdam.py:297-324: exp_avg.mul_(b1).add_(g, alpha=1-b1);
// exp_avg_sq.mul_(b2).addcmul_(g, g, value=1-b2); denom = sqrt(v)/bc2_sqrt + eps;
// param.addcdiv_(exp_avg, denom, value=-step_size)
__device__ __forceinline__ void adam_at_g(const gsr_adam_group &G, int64_t e, float g, float b1, float b2, float omb1,
                                          float omb2, float eps) {
    const float m = G.exp_avg[e] * b1 + omb1 * g;
    const float v = G.exp_avg_sq[e] * b2 + omb2 * (g * g);
    const float denom = sqrtf(v) / G.bias_correction2_sqrt + eps;
    G.exp_avg[e] = m;
    G.exp_avg_sq[e] = v;
    G.param[e] = G.param[e] + (-G.step_size) * (m / denom);
}

// The dense step's flat runs (optim.hip dense_adam_flat_kernel) and the arithmetic of one element of
// a run; post_step.hip's row-state kernel applies the same function, so the two cannot drift apart.
constexpr int kMaxGroups = 8;
constexpr int kAdamThreads = 256;

struct FlatAdamRun {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t n;         // floats
    int row;           // floats per row (the column of element e is e % row)
    int split_col;     // columns < split_col take step0, the rest step1 (row: one step size)
    float step0, step1;
    float bc2s;
    int vec;           // all four arrays 16-B aligned and row % 4 == 0: float4 access
};
struct FlatAdamArgs {
    FlatAdamRun r[kMaxGroups];
    int64_t block_start[kMaxGroups + 1];
    int n;
};
constexpr int kFlatPerThread = 8;  // two float4 per lane
constexpr int64_t kFlatPerBlock = (int64_t)kAdamThreads * kFlatPerThread;

__device__ __forceinline__ void flat_adam_one(const FlatAdamRun &R, float &p, float &m, float &v, float g, float ss,
                                              float b1, float b2, float omb1, float omb2, float eps) {
    const float mm = m * b1 + omb1 * g;
    const float vv = v * b2 + omb2 * (g * g);
    const float denom = sqrtf(vv) / R.bc2s + eps;
    m = mm;
    v = vv;
    p = p + (-ss) * (mm / denom);
}

// optim.hip: the flat runs of a dense step over `groups` (a column-split pair of one buffer merged
// into one run); a group that is no whole-row run goes to rest[].  Returns the number of runs.
int flat_adam_runs(int n_groups, const gsr_adam_group *groups, int64_t P, FlatAdamArgs &fa, int *rest, int &n_rest);

}  // namespace gsr
