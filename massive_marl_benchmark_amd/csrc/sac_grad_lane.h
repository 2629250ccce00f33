// sac_grad_lane.h -- the per-action backward of SAC's squashed-Gaussian head (agents/algorithms/rl/sac/module.py:31-61; the forward is
// sac_lane.h), written once for the HIP kernel (sac_grad_kernels.hip) and the CPU build (cpu/mms_cpu.cpp).  Both are compiled with
// -ffp-contract=off and without fast-math: every product and sum below is rounded on its own, tanhf and the division are the
// libraries' accurate ones.
#pragma once
#include <math.h>

#include "mms_lane.h"

namespace mms {

// The rows of a tile (sac_grad_kernels.hip: what a workgroup holds in LDS at a time): a multiple of 4 with at most kSacGradTile
// elements, so a tile of a 16-byte aligned [N,A] array starts 16-byte aligned.
constexpr int kSacGradTile = 1024;
inline int sac_grad_tile_rows(int A) {
    const int r = (kSacGradTile / A) & ~3;
    return r < 4 ? 4 : r;
}

// One action of one row: u (the pre-squash sample), mu and log_std (clamped) as the forward stored them; g_a = d loss / d action,
// g_l = d loss / d logp of the row (0 where not given).  With t = tanh(u), s = 1 - t^2:
//   G    = act_limit s g_a + g_l 2 t s / (s + epsilon)        d/du of act_limit tanh(u) and of -log(1 - tanh(u)^2 + epsilon)
//   dmu  = G                                                  du/dmu = 1
//   dls  = G (u - mu) - g_l   inside the clamp, else 0        du/dlog_std = exp(log_std) z = u - mu; the -log_std term of logp
// (the -z^2 / 2 term of logp has no gradient: z is the drawn normal).  The clamp mask reads the stored value: the forward clamps
// exactly to the bound, so `inside` is -20 < log_std < 2.
MMS_HD void sac_grad_one(float u, float mu, float log_std, float g_a, float g_l, float act_limit, float epsilon, float& dmu, float& dls) {
    const float t = tanhf(u);
    const float s = 1.0f - t * t;
    const float r = (2.0f * t) * s / (s + epsilon);
    const float G = (act_limit * s) * g_a + g_l * r;
    dmu = G;
    dls = (log_std > -20.0f && log_std < 2.0f) ? G * (u - mu) - g_l : 0.0f;
}

}  // namespace mms
