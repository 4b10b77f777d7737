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

}  // namespace gsr
