// gru_lane.h -- the gate arithmetic of one GRU cell step (torch.nn.GRU's cell, gate order r, z, n; the reference's RNNLayer,
// agents/algorithms/utils/rnn.py:25-29, runs it on hxs * masks), written once for the HIP kernels (gru_kernels.hip,
// gru_gates_kernels.hip) and the CPU build (cpu/mms_cpu.cpp).  Both are compiled with -ffp-contract=off and without fast-math: every product and sum below is rounded on its
// own, expf, tanhf and the division are the libraries' accurate ones.  The two builds differ only in the order of the dot products
// that feed it.
#pragma once
#include <math.h>

#include "mms_lane.h"

namespace mms {

constexpr int kGruMaxH = 1024;

// hm = mask * h as the reference multiplies (a NaN in a masked row stays NaN); + 0 turns the -0 of 0 * negative into +0, so a masked
// row is bit for bit the row of a zero state
MMS_HD float gru_masked(float m, float h) { return m * h + 0.0f; }

MMS_HD float gru_sigmoid(float a) { return 1.0f / (1.0f + expf(-a)); }

// s_r, s_z: the r and z rows' dot products over x AND hm (one sum); s_ni, s_nh: the n row's over x and over hm, kept apart because r
// multiplies the second with its bias
MMS_HD float gru_cell(float s_r, float s_z, float s_ni, float s_nh, float bi_r, float bi_z, float bi_n, float bh_r, float bh_z, float bh_n, float hm) {
    const float r = gru_sigmoid((s_r + bi_r) + bh_r);
    const float z = gru_sigmoid((s_z + bi_z) + bh_z);
    const float n = tanhf((s_ni + bi_n) + r * (s_nh + bh_n));
    return (1.0f - z) * n + z * hm;
}

// The same cell from the two [3H] pre-activation blocks of a step whose products ran elsewhere (mms_gru_gates_group): gi_* = x W_ih^T +
// b_ih with the bias in, gh_* = h W_hh^T of the UNMASKED state without its bias.  A per-row 0 / 1 mask commutes with the product,
// (m h) W^T = m (h W^T), so it multiplies gh here as gru_masked multiplies h above: a row with mask 0 is bit for bit the row of a zero
// state with zero gh.  masked = false: m is not read (hm = h, a = gh + b).
MMS_HD float gru_gates(bool masked, float m, float gi_r, float gi_z, float gi_n, float gh_r, float gh_z, float gh_n, float bh_r, float bh_z, float bh_n, float h) {
    const float hm = masked ? gru_masked(m, h) : h;
    const float a_r = (masked ? gru_masked(m, gh_r) : gh_r) + bh_r;
    const float a_z = (masked ? gru_masked(m, gh_z) : gh_z) + bh_z;
    const float a_n = (masked ? gru_masked(m, gh_n) : gh_n) + bh_n;
    const float r = gru_sigmoid(gi_r + a_r);
    const float z = gru_sigmoid(gi_z + a_z);
    const float n = tanhf(gi_n + r * a_n);
    return (1.0f - z) * n + z * hm;
}

}  // namespace mms
