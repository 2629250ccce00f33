// q_lane.h -- the per-row arithmetic behind the critics' last-layer dot product (agents/algorithms/rl/sac/sac.py:379-382,
// td3/td3.py:370-373, ddpg/ddpg.py:368-369), written once for the HIP kernel (q_kernels.hip) and the CPU build (cpu/mms_cpu.cpp).
#pragma once
#include "mms_lane.h"

namespace mms {

// the critic's output from its finished dot product: Linear(H, 1)'s bias
MMS_HD float q_value(float dot, float bias) { return dot + bias; }

// torch.min(q1_pi_targ, q2_pi_targ) for finite values.  The device code is built with finite-math-only, where a NaN test is folded
// away: a NaN in one critic (a diverged network) does not propagate here as it does through torch.min.
MMS_HD float q_min(float q0, float q1) { return fminf(q0, q1); }

// backup = r + gamma * (1 - d) * (q - alpha * logp); has_logp false: no alpha term (TD3, DDPG).  A done row (d != 0) returns r
// exactly for finite inputs: r + (gamma * 0) * x.
MMS_HD float q_backup(float r, uint8_t d, float q, bool has_logp, float logp, float gamma, float alpha) {
    const float keep = d ? 0.0f : 1.0f;
    const float x = has_logp ? q - alpha * logp : q;
    return r + (gamma * keep) * x;
}

}  // namespace mms
