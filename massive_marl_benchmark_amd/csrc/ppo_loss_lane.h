// ppo_loss_lane.h -- the per-element and per-row arithmetic of the PPO update's loss head and its gradients
// (agents/algorithms/rl/ppo/ppo.py:270-302 behind ActorCritic.evaluate, module.py:93-109), written once for the HIP kernel
// (ppo_loss_kernels.hip) and the CPU build (cpu/mms_cpu.cpp).  The formulas are the comment block of mms_ppo_loss in include/mms.h.
//
// The gradients are torch autograd's for the same expression, including how torch.max and torch.clamp split ties: a ratio inside
// [1 - clip, 1 + clip] (bounds included) makes both surrogate terms equal and both carry half the gradient, which is the whole; a
// value inside tv +- clip (bounds included) likewise.  One measure-zero case differs: outside the clip range with EXACTLY equal
// squares (v - ret)^2 == (vc - ret)^2 torch's maximum gives the unclipped branch half the gradient; here it gets none.
#pragma once
#include <math.h>

#include "mms_lane.h"

namespace mms {

// expf to about 1 ulp.  The device code is built with approximate functions (KERNEL_FLAGS), where expf is v_exp_f32 of a rounded
// x log2(e): a relative error of |x| 2^-24, which the ratio and the KL terms would inherit.  Here the product is carried as a
// head and a tail and only the reduced argument, |a| <= 0.5 plus the tail, goes through the hardware exponential.
MMS_HD float ppo_exp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float c = 0x1.715476p+0f, cl = 0x1.4ae0bep-26f;              // log2(e) = c + cl
    const float ph = x * c;
    const float pl = fmaf(x, cl, fmaf(x, c, -ph));
    const float e = rintf(ph);
    return ldexpf(exp2f((ph - e) + pl), (int)e);
#else
    return expf(x);
#endif
}

// per column j, from l_j = log_std[j]: einv = exp(-2 l) (one over the reference's scale sigma^2) and den = 2 exp(l)^2 (the KL's divisor)
MMS_HD void ppo_col_consts(float l, float& einv, float& den) {
    einv = ppo_exp(-2.0f * l);
    const float s = ppo_exp(l);
    den = 2.0f * (s * s);
}

// one element of logp_i: -0.5 z^2 - 2 l - 0.5 log 2pi, with z = (a - mu) exp(-2 l) left in z
MMS_HD float ppo_logp_term(float a, float mu, float l, float einv, float& z) {
    z = (a - mu) * einv;
    return (-0.5f * z) * z - 2.0f * l - 0.918938533204672742f;
}

// one element of entropy: 0.5 + 0.5 log 2pi + 2 l
MMS_HD float ppo_entropy_term(float l) { return 1.418938533204672742f + 2.0f * l; }

// one element of kl_i: l - os + (exp(os)^2 + (om - mu)^2) / (2 exp(l)^2) - 0.5
MMS_HD float ppo_kl_term(float l, float os, float om, float mu, float den) {
    const float so = ppo_exp(os), d = om - mu;
    return l - os + (so * so + d * d) / den - 0.5f;
}

struct PpoRow {
    float g;            // d loss / d logp_i (0 where the clipped branch is taken)
    float dvalue;       // d loss / d value_i
    float surrogate;    // max(-adv r, -adv clamp(r)): this row's term of the mean
    float value_loss;   // this row's term of the mean
};

// what follows a row's finished logp (summed in double by both builds).  inv_m = 1 / M as fp32.
MMS_HD PpoRow ppo_row(double logp, float old_logp, float adv, float v, float ret, float tv, float clip, float value_coef, bool clipped_value,
                      float inv_m) {
    PpoRow o;
    const float r = ppo_exp((float)(logp - (double)old_logp));
    const float lo = 1.0f - clip, hi = 1.0f + clip;
    const float rc = r < lo ? lo : (r > hi ? hi : r);
    const float s1 = -adv * r, s2 = -adv * rc;
    o.surrogate = s1 > s2 ? s1 : s2;
    const bool take = (r >= lo && r <= hi) || s1 > s2;
    o.g = take ? (inv_m * -adv) * r : 0.0f;
    const float e1 = v - ret, l1 = e1 * e1;
    bool vtake = true;
    o.value_loss = l1;
    if (clipped_value) {
        const float d = v - tv;
        const float dc = d < -clip ? -clip : (d > clip ? clip : d);
        const float e2 = (tv + dc) - ret, l2 = e2 * e2;
        o.value_loss = l1 > l2 ? l1 : l2;
        vtake = (d >= -clip && d <= clip) || l1 > l2;
    }
    o.dvalue = vtake ? (value_coef * inv_m) * (2.0f * e1) : 0.0f;
    return o;
}

MMS_HD float ppo_dmu(float g, float z, float einv) { return (g * z) * einv; }

// one row's term of dlog_std_j: g_i (2 z^2 - 2)
MMS_HD float ppo_dlog_std_term(float g, float z) { return g * (2.0f * (z * z) - 2.0f); }

// the results from the finished sums (double, rounded once).  out = {loss, surrogate, value_loss, entropy, kl}
MMS_HD void ppo_finish_scalars(double sum_surrogate, double sum_value_loss, double sum_kl, double entropy, int64_t M, float value_coef,
                               float entropy_coef, float* out) {
    const double m = (double)M;
    const double su = sum_surrogate / m, vl = sum_value_loss / m;
    out[0] = (float)(su + (double)value_coef * vl - (double)entropy_coef * entropy);
    out[1] = (float)su;
    out[2] = (float)vl;
    out[3] = (float)entropy;
    out[4] = (float)(sum_kl / m);
}

MMS_HD float ppo_finish_dlog_std(double column_sum, float entropy_coef) { return (float)(column_sum - 2.0 * (double)entropy_coef); }

}  // namespace mms
