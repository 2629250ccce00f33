// marl_eval_kernels.hip -- the log-density of GIVEN actions under each agent's Gaussian head and the HAPPO factor product for gfx950
// (mms_marl_heads_eval, include/mms.h): the tail of Actor.evaluate_actions behind the grouped hidden layers, for up to MMS_MAX_GROUPS
// networks per launch (blockIdx.y).
// The front is marl_heads_kernel's (policy_kernels.hip): the head's weights ([A, H] fp32, at most 64 KB) are staged in LDS once per
// workgroup and reused by its 4 x ROWS rows; a wave owns a row, lane t holds columns t, t + 64, .. of it.  In place of the sample a lane
// j < A reads act[row, j] and stores logp[row, j]; lane 0 forms the factor from the A differences in ascending j.
// Arithmetic: marl_eval_lane.h, shared with the CPU build: double between the fp32 inputs and the fp32 outputs.  A row's sums over H
// are a lane's columns in ascending order, then the xor butterfly 32 .. 1, after which every lane holds the same bits.  The order is a
// function of H alone: a row's results do not depend on M, on the group count, on ROWS or on where the row sits.  No atomics.
// Cost: per row and head output H conversions of a weight, H products and H sums in double (no contraction), and a six-step butterfly
// of 64-bit values.  That arithmetic, not the 4 H bytes read per row, bounds the kernel: measured 1.33 ms for 10 networks x 32768 rows
// at H = 512, A = 8 (0.50 TB/s of h), a third of one agent's pass through the layers and this tail.  Running four head rows'
// butterflies side by side was tried and was slower (176 registers against the chains it shortened: 1.80 ms).
// Built like param_step_kernels.hip (csrc/Makefile: PARAM_FLAGS): no fast-math, -ffp-contract=off, IEEE division and square root.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marl_eval_args.h"
#include "marl_eval_lane.h"

namespace mms {

constexpr int kEvalPerLane = kEvalMaxH / 64;
constexpr int kEvalRows = 8;

__device__ __forceinline__ double eval_wave_sum(double s) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    return s;
}

template <int ROWS>
__global__ void __launch_bounds__(256) marl_heads_eval_kernel(HeadsEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];          // [A][H]
    const int g = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = a.H, A = a.A[g];
    for (int k = threadIdx.x; k < A * H; k += 256) s_w[k] = a.w[g][k];
    __syncthreads();
    const bool ln = a.eps >= 0.f;                       // (eps < 0: no LayerNorm; gamma / beta are not read and may be NULL)
    float gm[kEvalPerLane], bt[kEvalPerLane];
#pragma unroll
    for (int i = 0; i < kEvalPerLane; i++) {
        const int k = lane + 64 * i;
        gm[i] = (ln && k < H) ? a.gamma[g][k] : 0.f;
        bt[i] = (ln && k < H) ? a.beta[g][k] : 0.f;
    }
    const bool mine_dim = lane < A;
    const float bias = mine_dim ? a.b[g][lane] : 0.f;
    const float sd = mine_dim ? a.std[g][lane] : 1.f;
    const float* __restrict__ act = a.act[g];
    const float* __restrict__ old = a.old_logp[g];
    float* logp = a.logp[g];
    float* fout = a.factor_out[g];
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * ROWS;
    for (int r = 0; r < ROWS; r++) {
        const int64_t row = row0 + r;
        if (row >= a.M) return;                         // (wave-uniform; no barrier follows)
        const float* __restrict__ h = a.h[g] + row * H;
        double x[kEvalPerLane];                         // the (normalised) row, this lane's columns
#pragma unroll
        for (int i = 0; i < kEvalPerLane; i++) x[i] = (lane + 64 * i < H) ? (double)h[lane + 64 * i] : 0.0;
        if (ln) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < kEvalPerLane; i++) if (lane + 64 * i < H) s += x[i];
            const double mean = eval_mean(eval_wave_sum(s), H);
            double q = 0.0;
#pragma unroll
            for (int i = 0; i < kEvalPerLane; i++) if (lane + 64 * i < H) q += eval_dev2((float)x[i], mean);
            const double rstd = eval_rstd(eval_wave_sum(q), H, a.eps);
#pragma unroll
            for (int i = 0; i < kEvalPerLane; i++) x[i] = eval_norm((float)x[i], mean, rstd, gm[i], bt[i]);       // (slots past H are not read below)
        }
        double dot = 0.0;                               // lane j keeps output j
        for (int j = 0; j < A; j++) {
            const float* wj = s_w + j * H;
            double p = 0.0;
#pragma unroll
            for (int i = 0; i < kEvalPerLane; i++) if (lane + 64 * i < H) p += eval_term(x[i], wj[lane + 64 * i]);
            p = eval_wave_sum(p);
            if (lane == j) dot = p;
        }
        float lp = 0.f;
        if (mine_dim) {
            lp = eval_logp(act[row * a.act_pitch[g] + lane], eval_mu(dot, bias), sd);
            if (logp) logp[row * a.logp_pitch[g] + lane] = lp;
        }
        if (fout == nullptr) continue;                  // (uniform over the workgroup)
        const double diff = mine_dim ? eval_diff(lp, old[row * a.old_pitch[g] + lane]) : 0.0;
        double sum = 0.0;
        for (int j = 0; j < A; j++) sum += __shfl(diff, j, 64);          // ascending j, as the CPU build
        if (lane == 0) fout[row] = eval_factor(a.factor_in[g] ? a.factor_in[g][row] : 1.f, sum);
    }
}

// the launch of a checked call (mms_host.h: check_marl_heads_eval)
hipError_t launch_marl_heads_eval(const HeadsEvalArgs& a, int groups, hipStream_t s) {
    if (a.M == 0 || groups == 0) return hipSuccess;
    if (groups < 0 || groups > MMS_MAX_GROUPS || a.M < 0 || a.M > 0x7fffffff || a.H < 1 || a.H > kEvalMaxH) return hipErrorInvalidValue;
    int amax = 1;
    for (int g = 0; g < groups; g++) {
        if (a.A[g] < 1 || a.A[g] > kEvalMaxA) return hipErrorInvalidValue;       // (the entry's check refuses it with a message)
        amax = a.A[g] > amax ? a.A[g] : amax;
    }
    const size_t lds = (size_t)amax * a.H * sizeof(float);                       // <= 16 x 1024 x 4 = 64 KB
    // fewer than two workgroups per CU at 8 rows per wave: 2 rows per wave (which rows a wave owns changes no row's arithmetic)
    const bool small = (a.M + 4 * kEvalRows - 1) / (4 * kEvalRows) * groups < 512;
    const int64_t per_block = 4 * (small ? 2 : kEvalRows);
    const dim3 grid((unsigned)((a.M + per_block - 1) / per_block), groups);
    if (small) hipLaunchKernelGGL(marl_heads_eval_kernel<2>, grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL(marl_heads_eval_kernel<kEvalRows>, grid, dim3(256), lds, s, a);
    return hipGetLastError();
}

}  // namespace mms
