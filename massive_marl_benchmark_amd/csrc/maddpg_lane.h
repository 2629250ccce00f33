// maddpg_lane.h -- the per-action math of MADDPG's deterministic actor head (agents/algorithms/marl/maddpg/module.py:36-46
// MLPActLayer.forward, :165-175 MADDPG_policy.act), written once for the HIP kernel (maddpg_kernels.hip) and the CPU build of the
// engine (cpu/mms_cpu.cpp).  The grouped Q target's per-row math is q_lane.h's.
#pragma once
#include "mms_lane.h"

namespace mms {

// act_limit * tanh(pi's last Linear): `pre` is the finished dot product plus bias (module.py:46)
MMS_HD float det_action(float pre, float act_limit) { return act_limit * tanhf(pre); }

// clamp(a + sigma * z, -act_limit, act_limit) (module.py:172-173); z is the counter-based stream of the PPO sampling, keyed by the
// action's column in the JOINT action row so that the agents of one env draw different normals
MMS_HD float det_explore(float a, float sigma, uint64_t seed, uint64_t row_global, uint64_t counter, uint32_t joint_col, float act_limit) {
    const float z = rand_normal(seed, row_global, counter, joint_col);
    return fminf(fmaxf(a + sigma * z, -act_limit), act_limit);
}

}  // namespace mms
