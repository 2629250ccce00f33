// param_step_lane.h -- the per-element arithmetic of the parameter step (clip_grad_norm_ + torch.optim.Adam + the polyak statements:
// agents/algorithms/rl/sac/sac.py:325-349, marl/maddpg/module.py:280-292), written once for the HIP kernels (param_step_kernels.hip)
// and the CPU build (cpu/mms_cpu.cpp).  Both are compiled with -ffp-contract=off and without fast-math: every product and sum below
// is rounded on its own, division and square root are IEEE, NaN and inf propagate.
#pragma once
#include <math.h>

#include "mms_lane.h"

namespace mms {

// the call's scalars as the element rule reads them: formed in double from the caller's doubles and rounded once (torch does the
// same with its Python floats: `1 - beta1`, `lr / bias_correction1`, `bias_correction2 ** 0.5`, `(1 - polyak) * p`)
struct ParamCoef {
    float step_size;     // lr / (1 - beta1^step)
    float bc2_sqrt;      // sqrt(1 - beta2^step)
    float eps, beta2, omb1, omb2, weight_decay;
    float polyak, omp;   // (float)polyak, (float)(1.0 - polyak)
};

inline ParamCoef param_coef(double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, double polyak) {
    ParamCoef c;
    c.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    c.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    c.eps = (float)eps;
    c.beta2 = (float)beta2;
    c.omb1 = (float)(1.0 - beta1);
    c.omb2 = (float)(1.0 - beta2);
    c.weight_decay = (float)weight_decay;
    c.polyak = (float)polyak;
    c.omp = (float)(1.0 - polyak);
    return c;
}

// clip_grad_norm_'s coefficient from the total norm: clamp(max_norm / (total + 1e-6), max = 1); max_norm <= 0: no clipping.  A NaN
// total stays a NaN coefficient (torch.clamp keeps it), so the comparison is written to be false for NaN.
MMS_HD float param_clip_coef(float total, float max_norm) {
    if (!(max_norm > 0.f)) return 1.f;
    const float x = max_norm / (total + 1e-6f);
    return (x > 1.f) ? 1.f : x;
}

// torch.optim.Adam's default rule for one element (no amsgrad, no maximize); g is the gradient as stored, coef the clip coefficient
MMS_HD void param_adam(float& p, float g, float& m, float& v, float coef, const ParamCoef& c) {
    float gc = coef * g;
    if (c.weight_decay != 0.f) {
        const float wp = c.weight_decay * p;
        gc = gc + wp;
    }
    const float d = gc - m;
    const float dm = d * c.omb1;
    m = m + dm;
    const float vb = v * c.beta2;
    const float g2 = (c.omb2 * gc) * gc;
    v = vb + g2;
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    const float upd = c.step_size * (m / denom);
    p = p - upd;
}

// p_targ.mul_(polyak); p_targ.add_((1 - polyak) * p): two products, one sum, each rounded
MMS_HD float param_polyak(float t, float p, const ParamCoef& c) {
    const float a = t * c.polyak;
    const float b = c.omp * p;
    return a + b;
}

}  // namespace mms
