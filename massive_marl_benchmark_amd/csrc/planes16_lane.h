// planes16_lane.h -- the two-plane fp16 operand format "H32" (f16x2), defined ONCE for the HIP kernels and the CPU build.
//
// A row x of K floats is stored as x s = hi + lo 2^-11 with s a power of two per row: [rows][KC][2][32] f16, KC = ceil(K / 32) -- the hi
// and the lo plane of 32 consecutive k are one 128-byte chunk, columns past K are zero, MMS_H32_BYTES(rows, K) bytes (include/mms.h).
// s puts a BOUND of the row's magnitudes at 2^14 (fp16 ends just below 2^16): a row's own largest magnitude for an input or a weight
// row, an a-priori bound for a hidden activation (the chain below, or the folded layers' row bound).  Why this loses nothing that
// matters and how the layer kernel multiplies such operands: split16_kernels.hip.
//
// Scalar rules only, no HIP builtins: the kernels cast to _Float16 around them, the host converts with f2h / h2f (cpu/lane_step.h).
#pragma once
#include "mms_lane.h"

namespace mms {

constexpr int kChunk16 = 128;                    // one row's two planes of 32 k, in bytes: hi at [0, 64), lo at [64, 128)
constexpr float kLoScale = 2048.f;               // the lo plane holds the residual times 2^11
constexpr int kTopExp = 14;                      // a row's bound sits at 2^14
constexpr float kBoundSlack = 1.001f;            // on every a-priori bound: the rounding of the bound itself (2^14 leaves a factor 4 besides)

// scale = 2^(14 - e) with bound <= 2^e; an all-zero row keeps scale 1
MMS_HD void pow2_scale(float bound, float& scale, float& inv) {
    int e = kTopExp;
    if (bound > 0.f) (void)frexpf(bound, &e);    // bound = f 2^e, 0.5 <= f < 1
    int sh = kTopExp - e;
    sh = sh > 100 ? 100 : (sh < -100 ? -100 : sh);
    scale = ldexpf(1.f, sh);
    inv = ldexpf(1.f, -sh);
}

// element t = x s:  hi = f16(t),  lo = f16(planes16_lo(t, hi));  back:  t ~ planes16_join(hi, lo)
MMS_HD float planes16_lo(float t, float hi) { return (t - hi) * kLoScale; }
MMS_HD float planes16_join(float hi, float lo) { return hi + lo * (1.f / kLoScale); }

// where 8-element piece p of a row starts in its hi plane (the kernels' 16-byte store; its lo half is 64 bytes on) ...
MMS_HD uint8_t* planes16_piece(uint8_t* planes, int64_t row, int KC, int p) { return planes + (row * KC + (p >> 2)) * (int64_t)kChunk16 + (p & 3) * 16; }
// ... and element k, in f16 units (its lo value is 32 on)
template <class T>
MMS_HD T* planes16_elem(T* planes, int64_t row, int KC, int k) { return planes + (row * KC + k / 32) * (int64_t)(kChunk16 / 2) + k % 32; }

// The bound chain |act(W x + b)| <= (max row 1-norm of W) max|x| + max|b| (ELU, ReLU, tanh and the identity satisfy |act(y)| <= |y|):
// one layer, and chain c's L layers (ch = its (mult, add) pairs) from the input bound of row `row` of `rows`, stored as the scales the
// layer kernel reads: chain_scale / chain_inv [nchains][L][rows].
MMS_HD float chain_bound(float mult, float bound, float add) { return (mult * bound + add) * kBoundSlack; }
MMS_HD void chain_scales(const float* ch, int c, int L, float bound, float* chain_scale, float* chain_inv, int64_t rows, int64_t row) {
    for (int l = 0; l < L; l++) {
        bound = chain_bound(ch[2 * l], bound, ch[2 * l + 1]);
        float sc, iv;
        pow2_scale(bound, sc, iv);
        chain_scale[((size_t)c * L + l) * rows + row] = sc;
        chain_inv[((size_t)c * L + l) * rows + row] = iv;
    }
}

// The folded-LayerNorm layers (fold16_kernels.hip): |W~ xhat + c| <= |W~ row|_2 sqrt(K) + |c| per output row (l2 = the row's sum of
// squares), and the network's output bound from the largest of them
MMS_HD float fold_row_bound(float l2, int K, float c) { return sqrtf(l2) * sqrtf((float)K) + fabsf(c); }
MMS_HD float fold_net_bound(float row_bound_max) {
    float bound = row_bound_max * kBoundSlack;
    if (!(bound > 1e-30f)) bound = 1e-30f;
    return bound;
}

}  // namespace mms
