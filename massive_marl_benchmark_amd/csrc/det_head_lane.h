// det_head_lane.h -- the per-action math of ONE deterministic actor head with a gradient (agents/algorithms/rl/{ddpg,td3}/module.py
// MLPActor: Linear + tanh + act_limit; td3.py:361-367 target policy smoothing; autograd's backward of the head in compute_loss_pi,
// td3.py:383-388), written once for the HIP kernels (maddpg_kernels.hip forward, det_head_kernels.hip backward) and the CPU build
// (cpu/mms_cpu.cpp).  The forward's a = act_limit * tanh(pre) and its unclipped noise are maddpg_lane.h's det_action / det_explore.
// The backward's translation units are compiled with -ffp-contract=off and without fast-math: every product and difference of
// det_head_grad_one is rounded on its own, so dy has the same bits in both builds.
#pragma once
#include <math.h>

#include "mms_lane.h"

namespace mms {

// The rows of a tile of the backward (det_head_kernels.hip: what a workgroup holds in LDS at a time): a multiple of 4 with at most
// kDetGradTile elements, so a tile of a 16-byte aligned [N,A] array starts 16-byte aligned (sac_grad_lane.h's rule).
constexpr int kDetGradTile = 1024;
inline int det_grad_tile_rows(int A) {
    const int r = (kDetGradTile / A) & ~3;
    return r < 4 ? 4 : r;
}

// Target policy smoothing (td3.py:362-367): e = clamp(sigma z, -noise_clip, noise_clip), a2 = clamp(a + e, -act_limit, act_limit);
// z is the counter stream of det_explore, keyed by the action's column.  (noise_clip >= 0 and finite: the caller's choice of branch.)
MMS_HD float det_smooth(float a, float sigma, float noise_clip, uint64_t seed, uint64_t row_global, uint64_t counter, uint32_t col, float act_limit) {
    const float z = rand_normal(seed, row_global, counter, col);
    const float e = fminf(fmaxf(sigma * z, -noise_clip), noise_clip);
    return fminf(fmaxf(a + e, -act_limit), act_limit);
}

// One action of one row of the backward: t = tanh(pre) as the forward stored it, g = d loss / d action.
//   dy = (act_limit g) (1 - t^2)          d/dpre of act_limit tanh(pre)
MMS_HD float det_head_grad_one(float t, float g, float act_limit) { return (act_limit * g) * (1.0f - t * t); }

}  // namespace mms
