// marl_heads_grad_lane.h -- the per-element arithmetic of the MAPPO / HAPPO update's output heads and of their backward
// (mms_marl_heads_fwd_group, mms_marl_heads_grad_group, include/mms.h): DiagGaussian.fc_mean = Linear(H, A) with
// std = sigmoid(log_std / x_coef) y_coef, and Critic.v_out = Linear(H, 1).  Written once for the HIP kernels
// (marl_heads_grad_kernels.hip) and the CPU build (cpu/mms_cpu.cpp); both are compiled with -ffp-contract=off and without fast-math.
// Which arithmetic was built: every product of two fp32 values is formed in double (exact: 48 bits of significand) and every sum --
// over the H columns of a row (out), over the A actions (df), over the M rows (dw, db) -- is accumulated in double and rounded to fp32
// once, behind the bias where there is one.  The heads are skinny (A <= 16): the passes stream [M, H] once or twice and the double
// operations per element (A of them) sit behind 4 or 8 bytes of traffic.  An output is then the correctly rounded sum up to the
// accumulation's own 1e-16, whatever H and M are.
// The builds differ only in the order of the sums over H and over M (the kernel: four columns per thread, then over the row's threads
// in an order that is a function of H; rows in chunks; the CPU build: ascending), both in double.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mms_lane.h"

namespace mms {

constexpr int kHeadsMaxA = 16, kHeadsMaxH = 1024;

// The rows of the column-sum partition (elu_ln_lane.h's, with a quarter of its cap on the chunks: a chunk leaves A (H + 1) doubles, A
// times elu_ln's 3 H / 3, so at 128 chunks an A = 8, H = 512 head writes 4.2 MB of partials against the 64 MB of a 32768-row f): H / 4
// threads hold a row's items, P = 256 / (H / 4) rows are in flight per workgroup; a workgroup (the CPU build: one loop iteration) owns
// `chunk` consecutive rows; a chunk is at least 8 P rows and there are at most kHeadsMaxChunks of them.  A function of (M, H) alone.
constexpr int kHeadsBlock = 256, kHeadsMaxChunks = 128, kHeadsMinTrips = 8;
inline int64_t heads_chunk_rows(int64_t M, int H) {
    const int64_t least = (int64_t)kHeadsMinTrips * (kHeadsBlock / (H >> 2));
    const int64_t spread = (M + kHeadsMaxChunks - 1) / kHeadsMaxChunks;
    return spread > least ? spread : least;
}
inline int64_t heads_chunks(int64_t M, int H) {
    const int64_t c = heads_chunk_rows(M, H);
    return (M + c - 1) / c;
}
// doubles that one chunk of a network with A outputs leaves: dw [A, H], then db [A]
MMS_HD int64_t heads_part_doubles(int A, int H) { return (int64_t)A * (H + 1); }

MMS_HD double heads_prod(float a, float b) { return (double)a * (double)b; }
MMS_HD float heads_out(double sum, float bias) { return (float)(sum + (double)bias); }

// std = sigmoid(log_std / x_coef) y_coef and d std / d log_std, in double from the fp32 values, rounded once
MMS_HD double heads_sigmoid(float log_std, float x_coef) { return 1.0 / (1.0 + exp(-((double)log_std / (double)x_coef))); }
MMS_HD float heads_std(float log_std, float x_coef, float y_coef) { return (float)(heads_sigmoid(log_std, x_coef) * (double)y_coef); }
MMS_HD float heads_dlog_std(float dstd, float log_std, float x_coef, float y_coef) {
    const double s = heads_sigmoid(log_std, x_coef);
    return (float)((double)dstd * (double)y_coef * (s * (1.0 - s)) / (double)x_coef);
}

}  // namespace mms
