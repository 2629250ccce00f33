// marl_eval_lane.h -- the per-row arithmetic of mms_marl_heads_eval (include/mms.h): the last LayerNorm, the action head's mean and
// the diagonal Gaussian's log-density of GIVEN actions with the HAPPO factor product, written once for the HIP kernel
// (marl_eval_kernels.hip) and the CPU build (cpu/mms_cpu.cpp).  Both are compiled with -ffp-contract=off and without fast-math: every
// product and sum below is rounded on its own.
// Everything between the fp32 inputs and the two fp32 outputs is double: the LayerNorm's statistics and its normalised row, the dot
// product with a head row, the mean, the log-density -- logp is one rounding of it --, the sum of the differences over the action
// dimensions and its exp, rounded once at the product.  The differences are those of the fp32 value logp[r, j] that is (or would be)
// stored and old_logp[r, j]: where the parameters have not moved since old_logp was written by this entry, every difference is 0 and
// the factor is factor_in bit for bit (a HAPPO update that changes nothing leaves the factor at exactly 1); the factor does not depend
// on whether logp is stored.  A row-wise pass has the time: (A + 3) H double operations per row against 4 H bytes read.
// The builds differ only in the order in which a row's sums over H are added (the kernel: a lane's columns lane, lane + 64, .. in
// ascending order, then an xor butterfly over the wave's 64 lanes; the CPU build: ascending columns).  The sum over the action
// dimensions is ascending j in both.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mms_lane.h"

namespace mms {

constexpr int kEvalMaxH = 1024, kEvalMaxA = 16;

// the LayerNorm's statistics from a row's two sums (two-pass, biased, eps inside the root, as nn.LayerNorm)
MMS_HD double eval_mean(double sum, int H) { return sum / (double)H; }
MMS_HD double eval_dev2(float h, double mean) {
    const double d = (double)h - mean;
    return d * d;
}
MMS_HD double eval_rstd(double sum_sq, int H, float eps) { return 1.0 / sqrt(sum_sq / (double)H + (double)eps); }
MMS_HD double eval_norm(float h, double mean, double rstd, float gamma, float beta) { return ((double)h - mean) * rstd * (double)gamma + (double)beta; }

// one term of the head's dot product, and the mean from the finished sum
MMS_HD double eval_term(double xn, float w) { return xn * (double)w; }
MMS_HD double eval_mu(double dot, float bias) { return dot + (double)bias; }

// log N(act | mu, sd) of one dimension (FixedNormal.log_probs): -(act - mu)^2 / (2 sd^2) - log(sd) - log(sqrt(2 pi))
MMS_HD float eval_logp(float act, double mu, float sd) {
    const double d = (double)act - mu, s = (double)sd;
    return (float)(-(d * d) / (2.0 * s * s) - log(s) - 0.9189385332046727);
}

// one term of the factor's exponent, and the product with its one rounding
MMS_HD double eval_diff(float logp, float old_logp) { return (double)logp - (double)old_logp; }
MMS_HD float eval_factor(float factor_in, double sum) { return (float)((double)factor_in * exp(sum)); }

}  // namespace mms
