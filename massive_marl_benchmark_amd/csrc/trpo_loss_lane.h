// trpo_loss_lane.h -- the per-element and per-row arithmetic of the TRPO policy step's head (agents/algorithms/rl/trpo/trpo.py:287-298,
// 417-435, 464-478 behind ActorCritic.evaluate), written once for the HIP kernel (trpo_loss_kernels.hip) and the CPU build
// (cpu/mms_cpu.cpp).  The formulas are the comment block of mms_trpo_heads in include/mms.h.
//
// logp, the ratio and the KL term are ppo_loss_lane.h's statements (ppo_col_consts, ppo_logp_term, ppo_kl_term, ppo_exp), so on one build
// a_loss, kl and gsur have the bits mms_ppo_loss gives for its unclipped surrogate, its kl and its dmu.  ppo_exp is expf on the host and
// the hardware exponential behind a two-word argument reduction on the device: logp, a_loss, kl and gsur of the two builds agree to
// rounding, NOT bit for bit.
// gkl and gn use none of it: a subtraction, one IEEE division, and a divisor exp(2 l) M from trpo_exp below, which is written in
// operations both builds round alike (fma, rint, ldexp in double; no contraction in either build).  gkl and gn have the SAME BITS in
// the HIP and the CPU build.
#pragma once
#include <math.h>

#include "mms_lane.h"
#include "ppo_loss_lane.h"

namespace mms {

// exp(x) in double to about 1e-16 relative, from operations that are correctly rounded everywhere: x = k ln2 + r with |r| <= 0.35,
// the Taylor polynomial of degree 13 in Horner form (the next term is below 4e-18), ldexp.
MMS_HD double trpo_exp(double x) {
    const double k = rint(x * 1.4426950408889634);
    double r = fma(-k, 6.93147180369123816490e-01, x);
    r = fma(-k, 1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)k);
}

// per column j: the divisor of gkl and gn, exp(l_j)^2 M, rounded to fp32 once
MMS_HD float trpo_col_den(float l, int64_t M) { return (float)(trpo_exp(2.0 * (double)l) * (double)M); }

struct TrpoRow {
    float term;         // -adv r: this row's term of a_loss
    float g;            // d a_loss / d logp_i = -adv r / M
};

// what follows a row's finished logp (summed in double by both builds): ppo_row's unclipped branch.  inv_m = 1 / M as fp32.
MMS_HD TrpoRow trpo_row(double logp, float old_logp, float adv, float inv_m) {
    TrpoRow o;
    const float r = ppo_exp((float)(logp - (double)old_logp));
    o.term = -adv * r;
    o.g = (inv_m * -adv) * r;
    return o;
}

// gsur_ij = g_i z_ij exp(-2 l_j): ppo_dmu
MMS_HD float trpo_gsur(float g, float z, float einv) { return ppo_dmu(g, z, einv); }

// gkl_ij = (mu_ij - om_ij) / (exp(l_j)^2 M)
MMS_HD float trpo_gkl(float mu, float om, float cden) { return (mu - om) / cden; }

// gn_ij = rmu_ij / (exp(l_j)^2 M)
MMS_HD float trpo_gn(float rmu, float cden) { return rmu / cden; }

// a scalar from its finished sum (double, rounded once)
MMS_HD float trpo_finish_mean(double sum, int64_t M) { return (float)(sum / (double)M); }

}  // namespace mms
