// sac_lane.h -- the per-action math of SAC's squashed-Gaussian policy (agents/algorithms/rl/sac/module.py:31-61), written once for
// the HIP kernel (sac_kernels.hip) and the CPU build of the engine (cpu/mms_cpu.cpp).
#pragma once
#include "mms_lane.h"

namespace mms {

// One action of one row.  raw_log_std is log_std_layer's output before the clamp (module.py:35); the noise is the counter-based
// stream of the PPO sampling (rand_normal), none when deterministic (module.py:41-43).  Returns act_limit * tanh(u) (:58-59) and
// sets u (the pre-squash sample), log_std (clamped) and, when want_logp, this action's term of the log-probability (:50):
//   -z^2 / 2 - log_std - log(2 pi) / 2 - log(1 - tanh(u)^2 + epsilon),  z = (u - mu) / std = the drawn normal (0 when deterministic)
MMS_HD float sac_sample_one(float mu, float raw_log_std, int deterministic, uint64_t seed, uint64_t row_global, uint64_t counter, uint32_t j,
                            float act_limit, float epsilon, bool want_logp, float& u, float& log_std, float& logp_term) {
    log_std = fminf(fmaxf(raw_log_std, -20.0f), 2.0f);
    const float z = deterministic ? 0.0f : rand_normal(seed, row_global, counter, j);
    u = deterministic ? mu : fmaf(expf(log_std), z, mu);
    const float t = tanhf(u);
    logp_term = want_logp ? -0.5f * z * z - log_std - 0.9189385332046727f - logf(1.0f - t * t + epsilon) : 0.0f;
    return act_limit * t;
}

}  // namespace mms
