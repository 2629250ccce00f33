// elu_ln_lane.h -- the per-element arithmetic of one `Linear + ELU + LayerNorm` block behind its matrix product (the reference's
// MLPLayer, agents/algorithms/utils/mlp.py:19-27) and of its backward (mms_elu_ln_group, mms_elu_ln_grad_group, include/mms.h), written
// once for the HIP kernels (elu_ln_kernels.hip) and the CPU build (cpu/mms_cpu.cpp).  Both are compiled with -ffp-contract=off and
// without fast-math: every product and sum below is rounded on its own.
// Which values are fp32: what torch holds in fp32 too -- u = z + bias, a = ELU(u) (expm1f) -- and everything that is stored: mean, rstd,
// y, dz.  What lies between two stored values is formed in double from those fp32 values and rounded once when it is stored: a row's
// sums, xhat, q, c1, c2, da.  A streaming pass has the time (a dozen double operations per element against 12 bytes of traffic), and
// the outputs then carry the rounding of u, a, mean and rstd and their own, not that of a chain of fp32 intermediates: LayerNorm's
// backward is a difference of three terms that cancel, in a narrow row to a small fraction of their size.
// The backward recomputes u, a and xhat by the forward's statements from z, bias and the stored (mean, rstd): bit for bit the forward's.
// The builds differ only in the order in which a row's sums over H are added (the kernel: four columns per thread, then over the row's
// threads in an order that is a function of H; the CPU build: ascending columns), both in double.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mms_lane.h"

namespace mms {

constexpr int kEluLnMaxH = 1024;

// The rows of the column-sum partition (gru_grad_lane.h's, with twice its cap on the chunks: at 32768 rows of width 512 two networks then
// fill the device's 256 CUs with the four workgroups each that the row pass's registers admit): H / 4 <= 256 threads hold a row's items, so
// P = 256 / (H / 4) rows are in flight per workgroup; a workgroup (the CPU build: one loop iteration) owns `chunk` consecutive rows
// and leaves one partial per column, in double; a chunk is at least 8 P rows and there are at most kEluLnMaxChunks of them.  A
// function of (M, H) alone.
constexpr int kEluLnBlock = 256, kEluLnMaxChunks = 512, kEluLnMinRows = 8;
inline int64_t elu_ln_chunk_rows(int64_t M, int H) {
    const int64_t least = (int64_t)kEluLnMinRows * (kEluLnBlock / (H >> 2));
    const int64_t spread = (M + kEluLnMaxChunks - 1) / kEluLnMaxChunks;
    return spread > least ? spread : least;
}
inline int64_t elu_ln_chunks(int64_t M, int H) {
    const int64_t c = elu_ln_chunk_rows(M, H);
    return (M + c - 1) / c;
}

// u = z + bias (z: the bias-free product x W^T), a = ELU(u) with alpha = 1
MMS_HD float elu_ln_u(float z, float bias) { return z + bias; }
MMS_HD float elu_ln_act(float u) { return u > 0.0f ? u : expm1f(u); }

// a row's statistics from its two sums (the second over (a - mean)^2 with the stored mean: two-pass, biased, as nn.LayerNorm)
MMS_HD float elu_ln_mean(double sum, int H) { return (float)(sum / (double)H); }
MMS_HD double elu_ln_dev2(float a, float mean) {
    const double d = (double)a - (double)mean;
    return d * d;
}
MMS_HD float elu_ln_rstd(double sum_sq, int H, float eps) { return (float)(1.0 / sqrt(sum_sq / (double)H + (double)eps)); }

MMS_HD double elu_ln_xhat(float a, float mean, float rstd) { return ((double)a - (double)mean) * (double)rstd; }
MMS_HD float elu_ln_out(double xhat, float gamma, float beta) { return (float)(xhat * (double)gamma + (double)beta); }

// backward: q = dy gamma (exact in double); c1 = mean_row(q), c2 = mean_row(q xhat);
//   da = rstd (q - c1 - xhat c2);  dz = da ELU'(u),  ELU'(u) = 1 for u > 0 and a + 1 (= e^u) otherwise
MMS_HD double elu_ln_q(float dy, float gamma) { return (double)dy * (double)gamma; }
MMS_HD double elu_ln_row_mean(double sum, int H) { return sum / (double)H; }
MMS_HD float elu_ln_dz(float u, float a, double xhat, float rstd, double q, double c1, double c2) {
    const double da = (double)rstd * ((q - c1) - xhat * c2);
    return (float)(da * (u > 0.0f ? 1.0 : (double)a + 1.0));
}

}  // namespace mms
