// marl_loss_lane.h -- the per-element and per-row arithmetic of the MAPPO / HAPPO update's loss head and its gradients
// (agents/algorithms/marl/mappo_trainer.py:63-179, happo_trainer.py:48-170 behind ACTLayer.evaluate_actions, utils/act.py:154-165,
// FixedNormal.log_probs, agents/utils/util.py:23-29), written once for the HIP kernels (marl_loss_kernels.hip) and the CPU build
// (cpu/mms_cpu.cpp).  The formulas are the comment block of mms_marl_ppo_loss in include/mms.h.
//
// The gradients are torch autograd's for the same expression, including how torch.min, torch.max and torch.clamp split ties: a ratio
// inside [1 - clip, 1 + clip] (bounds included) makes both surrogate terms equal and both carry half the gradient, which is the whole;
// a value inside vp +- clip (bounds included) likewise.  One measure-zero case differs: outside the clip range with EXACTLY equal
// non-zero losses h(e_o) == h(e_c) torch's maximum gives the unclipped branch half the gradient; here it gets none.
#pragma once
#include <math.h>

#include "mms_lane.h"
#include "ppo_loss_lane.h"

namespace mms {

// per column j, from std_j, in double: the device code is built with approximate logf and division, and a constant rounded to fp32 is
// an error shared by every row of its column, which the sums over rows (dstd_j, a parameter's gradient behind dmu) do not average out
struct MarlCol {
    double lstd;    // log std
    double ivar;    // 1 / std^2
    double istd3;   // 1 / std^3
    double istd;    // 1 / std
};

MMS_HD MarlCol marl_col_consts(float std) {
    const double s = (double)std, i = 1.0 / s;
    MarlCol c;
    c.lstd = log(s);
    c.ivar = i * i;
    c.istd3 = i * i * i;
    c.istd = i;
    return c;
}

// logp_ij = -(a - mu)^2 / (2 std^2) - log std - 0.5 log 2pi from the fp32 difference d = a - mu (left in d), in double
MMS_HD double marl_logp_term(float a, float mu, const MarlCol& c, float& d) {
    d = a - mu;
    return -((double)d * (double)d) * (0.5 * c.ivar) - c.lstd - 0.918938533204672742;
}

// one column of the entropy, in double: 0.5 + 0.5 log 2pi + log std
MMS_HD double marl_entropy_term(float std) { return 1.418938533204672742 + log((double)std); }

// the reference's huber_loss (util.py:23-26: b = (e > d), so e < -d gives 0) or mse_loss, and its derivative
MMS_HD float marl_h(float e, float delta, bool huber) {
    if (!huber) return (e * e) * 0.5f;
    const float ae = fabsf(e);
    if (ae <= delta) return (e * e) * 0.5f;
    return e > delta ? delta * (ae - 0.5f * delta) : 0.0f;
}
MMS_HD float marl_dh(float e, float delta, bool huber) {
    if (!huber || fabsf(e) <= delta) return e;
    return e > delta ? delta : 0.0f;
}

struct MarlScalars {
    float clip, value_coef, delta;
    bool huber, clipped_value, use_norm;
    double norm_mean, norm_inv_sd;      // the target's normalisation (use_norm): mean and 1 / sqrt(var) in double
};

struct MarlRow {
    float ratio;        // r_i
    float surrogate;    // f_i min(r adv, clamp(r) adv)
    float value_loss;   // vl_i
    float g;            // d objective / d (sum_j logp_ij)
    float dvalue;       // d objective / d value_i
};

// what follows a row's finished sum_j (logp_ij - old_logp_ij) (summed in double by both builds).  wp, wv: the row's weight in the
// policy and the value mean (m_i / sum m or 1 / M), in double: g and dvalue are products rounded once.
MMS_HD MarlRow marl_row(double dlogp, float adv, float f, float v, float vp, float ret, const MarlScalars& k, double wp, double wv) {
    MarlRow o;
    const float r = ppo_exp((float)dlogp);
    const float lo = 1.0f - k.clip, hi = 1.0f + k.clip;
    const float rc = r < lo ? lo : (r > hi ? hi : r);
    const float s1 = r * adv, s2 = rc * adv;
    o.ratio = r;
    o.surrogate = f * (s1 < s2 ? s1 : s2);
    const bool take = (r >= lo && r <= hi) || s1 < s2;
    o.g = take ? (float)(((wp * -(double)adv) * (double)f) * (double)r) : 0.0f;
    const float t = k.use_norm ? (float)(((double)ret - k.norm_mean) * k.norm_inv_sd) : ret;
    const float eo = t - v, ho = marl_h(eo, k.delta, k.huber);
    float dh = marl_dh(eo, k.delta, k.huber);
    o.value_loss = ho;
    if (k.clipped_value) {
        const float d = v - vp;
        const bool inside = d >= -k.clip && d <= k.clip;
        const float dc = d < -k.clip ? -k.clip : (d > k.clip ? k.clip : d);
        const float ec = t - (vp + dc), hc = marl_h(ec, k.delta, k.huber);
        o.value_loss = ho > hc ? ho : hc;
        // inside the range vc is v and both branches pass their gradient to v; outside only the unclipped one can
        if (!(inside || ho > hc)) dh = 0.0f;
    }
    o.dvalue = (float)(-((double)k.value_coef * wv) * (double)dh);
    return o;
}

MMS_HD float marl_dmu(float g, float d, const MarlCol& c) { return (float)(((double)g * (double)d) * c.ivar); }

// one row's term of dstd_j: g_i ((a - mu)^2 / std^3 - 1 / std)
MMS_HD double marl_dstd_term(float g, float d, const MarlCol& c) { return (double)g * (((double)d * (double)d) * c.istd3 - c.istd); }

// the results from the finished sums (double, rounded once).  den_p, den_v: sum m or M.  ent_scale: 1 with policy masks, else 1 / A.
// out = {objective, policy_loss, value_loss, dist_entropy, ratio_mean}
MMS_HD void marl_finish_scalars(double sum_surrogate, double sum_value_loss, double sum_ratio, double entropy, double den_p, double den_v,
                                double ent_scale, int64_t M, float value_coef, float entropy_coef, float* out) {
    const double pl = -sum_surrogate / den_p, vl = sum_value_loss / den_v, ent = entropy * ent_scale;
    out[0] = (float)(pl - (double)entropy_coef * ent + (double)value_coef * vl);
    out[1] = (float)pl;
    out[2] = (float)vl;
    out[3] = (float)ent;
    out[4] = (float)(sum_ratio / (double)M);
}

MMS_HD float marl_finish_dstd(double column_sum, float std, float entropy_coef, double ent_scale) {
    return (float)(column_sum - (double)entropy_coef * ent_scale / (double)std);
}

}  // namespace mms
