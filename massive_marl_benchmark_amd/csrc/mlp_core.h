// mlp_core.h -- the operand splits, the GEMM and the fixed-order reductions of trpo_kernels.hip, as the LayerNorm MLP's entries
// (ln_mlp_kernels.hip) launch them.  The kernels and these launchers are defined once, in trpo_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "trpo_plan.h"

namespace mms {

constexpr int kChunk = 192;                      // one row's three planes of 32 k

// The fp32 operand of a split, evaluated at (m, k):  op 0: x;  op 1: x . f'(h);  op 2: x . f'(h) + e . f''(h) . r;
// op 3: LayerNorm's output (x - mean_m) rstd_m ga[k] + be[k] with (mean_m, rstd_m) = st[2 m], st[2 m + 1]
struct OperandArgs {
    const float* x;
    const float* h;
    const float* e;
    const float* r;
    int ldx, ldh, lde, ldr, op;
    const float* st;
    const float* ga;
    const float* be;
};

static inline OperandArgs operand(const float* x, int ldx, int op = 0, const float* h = nullptr, int ldh = 0, const float* e = nullptr, int lde = 0,
                                  const float* r = nullptr, int ldr = 0) {
    OperandArgs o = {x, h, e, r, ldx, ldh, lde, ldr, op, nullptr, nullptr, nullptr};
    return o;
}
static inline OperandArgs operand_ln(const float* x, int ldx, const float* st, const float* ga, const float* be) {
    OperandArgs o = {x, nullptr, nullptr, nullptr, ldx, 0, 0, 0, 3, st, ga, be};
    return o;
}

// A [rows, K] -> planes of A, rows padded to rows_pad, into chunks [coff, coff + KC) of rows of `pitch` chunks
hipError_t psplit(const OperandArgs& o, int64_t rows, int K, int64_t rows_pad, int pitch, int coff, uint8_t* dst, hipStream_t s);
// A [rows, cols] -> planes of A^T; MC = chunks over A's rows (all parts), MCs per part
hipError_t tsplit(const OperandArgs& o, int64_t rows, int cols, int MC, int MCs, int rows_pad, int pitch, int coff, uint8_t* dst, float* out, int ldo,
                  float* colp, int ldc, hipStream_t s);
// y_g = x_g w_g^T (+ b), g < groups, operands in planes (groups consecutive in memory at the given strides)
hipError_t gemm(int groups, int64_t M, int N, int KC, const uint8_t* x, size_t xs, const uint8_t* w, size_t ws, const float* b, float* y, size_t ys,
                hipStream_t s);
hipError_t copy2d(const float* src, int64_t rs, int cs, int lds, float* dst, int64_t rd, int cd, int ldd, hipStream_t s);
// out[n, k] = sum over g (in order) of part[g * stride + n * ldp + k], accumulated in Acc (float or double)
template <typename Acc>
hipError_t reduce(const float* part, int groups, size_t stride, int ldp, int N, int K, float* out, hipStream_t s);
// dW_l (and db_l) of one layer from the transposed planes already in ta / tb
hipError_t weight_grad(const MlpPlan& P, int l, int prods, uint8_t* ws, float* dw, float* db, hipStream_t s);
// tsplit into product q's S parts of ta / tb for layer l (contraction over the M rows)
hipError_t tsplit_rows(const MlpPlan& P, int l_rows, int S, int q, const OperandArgs& o, bool into_a, uint8_t* ws, float* out, int ldo, bool colsum,
                       hipStream_t s);

}  // namespace mms
