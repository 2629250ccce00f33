// q_loss_lane.h -- the per-row arithmetic and the partition of the critics' loss heads with a gradient (mms_q_heads_loss, include/mms.h:
// compute_loss_q, sac.py:367-389, and the critic half of compute_loss_pi, sac.py:392-403), written once for the HIP kernel
// (q_loss_kernels.hip) and the CPU build (cpu/mms_cpu.cpp).  q itself is q_lane.h's q_value on each build's own dot product.
#pragma once
#include <stdint.h>

#include "mms_lane.h"
#include "q_lane.h"

namespace mms {

constexpr int kQLossRows = 16;          // rows of a row group: the HIP kernel's 256 threads, a quarter wave per row
constexpr int kQLossSegments = 16;      // the finish pass adds the workgroups' partials in this many ascending segments

// The partition, a function of (M, H) alone: workgroup b walks `iters` consecutive row groups of kQLossRows rows each.  About 512
// workgroups where M allows (two per CU: a workgroup holds a whole row per quarter wave in registers, and every workgroup adds
// G (H + 1) + 1 doubles to the finish pass's traffic).
struct QLossPartition { int64_t groups, iters, blocks, per_segment; };
MMS_HD QLossPartition q_loss_partition(int64_t M, int /*H*/) {
    QLossPartition p;
    p.groups = (M + kQLossRows - 1) / kQLossRows;
    p.iters = (p.groups + 511) / 512;
    if (p.iters < 1) p.iters = 1;
    p.blocks = (p.groups + p.iters - 1) / p.iters;
    p.per_segment = (p.blocks + kQLossSegments - 1) / kQLossSegments;
    return p;
}
// columns of a workgroup's partial: [g][H] dw, [g][1] db at g (H + 1) + H, then the loss term's sum
MMS_HD int q_loss_columns(int G, int H) { return G * (H + 1) + 1; }

// d loss / d q_g of one row, times `scale`, IN DOUBLE, and the row's term of the loss sum (the caller divides the sum by M once).
//   mode 0: e_g = q_g - target, term = sum_g e_g^2, dq_g = scale 2 e_g / M
//   mode 1: m = min_g q_g, term = alpha logp - m (no logp: -m), dq_g = -scale / M on the strict minimum, half of it on a tie
//           (torch.min(a, b)'s backward), 0 otherwise
// dq stays in double for the sums over rows: dw and db then carry their own final rounding and nothing else -- rounded to fp32 first,
// every term would carry a rounding of its own (mode 0), or 1 / M its fp32 representation error into all of them with one sign (mode 1).
template <int G>
MMS_HD double q_loss_row(int mode, const float* q, float target, bool has_logp, float logp, float alpha, float scale, double m_rows, double* dq) {
    if (mode == 0) {
        double term = 0.0;
        for (int g = 0; g < G; g++) {
            const double e = (double)q[g] - (double)target;
            term += e * e;
            dq[g] = ((double)scale * 2.0 * e) / m_rows;
        }
        return term;
    }
    const double full = -(double)scale / m_rows;
    float m = q[0];
    if (G == 2) {
        const float a = q[0], b = q[G - 1];
        dq[0] = a < b ? full : b < a ? 0.0 : 0.5 * full;
        dq[G - 1] = b < a ? full : a < b ? 0.0 : 0.5 * full;
        m = b < a ? b : a;
    } else {
        dq[0] = full;
    }
    return (has_logp ? (double)alpha * (double)logp : 0.0) - (double)m;
}
// dh = dq w.  Mode 0: dq rounded to fp32 (one rounding), then the fp32 product (one more); mode 1, where dq is a constant of the
// call: the double product rounded once.
MMS_HD float q_loss_dh(int mode, double dq, float w) { return mode == 0 ? (float)dq * w : (float)(dq * (double)w); }

// a workgroup's sum over its 16 row slots (slot r: the rows (group) * 16 + r of its row groups, added in ascending order): the slots of
// a wave pairwise -- what two xor shuffles (16, 32) leave in the wave's first quarter -- then the four waves in ascending order
MMS_HD double q_loss_slot_sum(const double* a) {
    double w[4];
    for (int i = 0; i < 4; i++) w[i] = (a[4 * i] + a[4 * i + 1]) + (a[4 * i + 2] + a[4 * i + 3]);
    return ((w[0] + w[1]) + w[2]) + w[3];
}

// the finish pass's sum of one column over the workgroups' partials: kQLossSegments ascending segments, each ascending, then the
// segments in ascending order
MMS_HD double q_loss_segment_sum(const double* part, int64_t stride, int64_t first, int64_t last) {
    double s = 0.0;
    for (int64_t b = first; b < last; b++) s += part[b * stride];
    return s;
}

}  // namespace mms
