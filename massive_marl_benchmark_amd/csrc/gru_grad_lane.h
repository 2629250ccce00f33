// gru_grad_lane.h -- the per-element backward of the GRU gate step of gru_lane.h (gru_gates; mms_gru_gates_grad_group, include/mms.h),
// written once for the HIP kernel (gru_grad_kernels.hip) and the CPU build (cpu/mms_cpu.cpp).  Both are compiled with
// -ffp-contract=off and without fast-math: every product and sum below is rounded on its own, and the forward's r, z, n are recomputed
// by the statements of gru_gates in their order, so they are bit for bit the forward's.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gru_lane.h"

namespace mms {

// The rows of the dbias partition: a workgroup (the CPU build: one loop iteration) owns `chunk` consecutive rows and leaves one
// partial per column, in double.  H / 4 <= 256 threads hold a row's items, so P = 256 / (H / 4) rows are in flight per workgroup; a
// chunk is at least 8 P rows and there are at most kGruGradMaxChunks of them.  A function of (M, H) alone.
constexpr int kGruGradBlock = 256, kGruGradMaxChunks = 256, kGruGradMinRows = 8;
inline int64_t gru_grad_chunk_rows(int64_t M, int H) {
    const int64_t least = (int64_t)kGruGradMinRows * (kGruGradBlock / (H >> 2));
    const int64_t spread = (M + kGruGradMaxChunks - 1) / kGruGradMaxChunks;
    return spread > least ? spread : least;
}
inline int64_t gru_grad_chunks(int64_t M, int H) {
    const int64_t c = gru_grad_chunk_rows(M, H);
    return (M + c - 1) / c;
}

struct GruGateGrad {
    float dpr, dpz, dpn, rdpn;      // d loss / d (pre-activation of r, z, n), and r dpn = d loss / d a_n: dgi and the dbias terms
    float dgh_r, dgh_z, dgh_n;      // m [dpr | dpz | r dpn] + 0
    float dh;                       // m (G z) + 0: the direct path to the incoming state
};

// One hidden unit of one row.  G = d loss / d h' (the caller added dh_out and dy).  h' = (1 - z) n + z hm:
//   dn = G (1 - z), dz = G (hm - n), d hm (direct) = G z;  n = tanh(gi_n + r a_n): dpn = dn (1 - n^2), dr = dpn a_n, d a_n = r dpn;
//   z = sigmoid(..): dpz = dz z (1 - z);  r = sigmoid(..): dpr = dr r (1 - r);  a_* = m gh_* + b: d gh_* = m d a_*;  hm = m h: dh = m G z.
// masked = false: m is not read.  Every product with the mask is followed by + 0 (and the unmasked values too, so that mask NULL is a
// mask of ones bit for bit): a masked row's dgh and dh are +0, never -0.
MMS_HD GruGateGrad gru_gates_grad(bool masked, float m, float gi_r, float gi_z, float gi_n, float gh_r, float gh_z, float gh_n, float bh_r, float bh_z,
                                  float bh_n, float h, float G) {
    const float hm = masked ? gru_masked(m, h) : h;
    const float a_r = (masked ? gru_masked(m, gh_r) : gh_r) + bh_r;
    const float a_z = (masked ? gru_masked(m, gh_z) : gh_z) + bh_z;
    const float a_n = (masked ? gru_masked(m, gh_n) : gh_n) + bh_n;
    const float r = gru_sigmoid(gi_r + a_r);
    const float z = gru_sigmoid(gi_z + a_z);
    const float n = tanhf(gi_n + r * a_n);
    GruGateGrad o;
    o.dpn = (G * (1.0f - z)) * (1.0f - n * n);
    o.dpz = (G * (hm - n)) * (z * (1.0f - z));
    o.dpr = (o.dpn * a_n) * (r * (1.0f - r));
    o.rdpn = r * o.dpn;
    const float gz = G * z;
    o.dgh_r = (masked ? m * o.dpr : o.dpr) + 0.0f;
    o.dgh_z = (masked ? m * o.dpz : o.dpz) + 0.0f;
    o.dgh_n = (masked ? m * o.rdpn : o.rdpn) + 0.0f;
    o.dh = (masked ? m * gz : gz) + 0.0f;
    return o;
}

}  // namespace mms
