// trpo_loss_kernels.hip -- the head of TRPO's policy step for gfx950 (mms_trpo_heads, include/mms.h).
//
//   trpo_heads_rows_kernel    per row: logp, the ratio's term of a_loss, the KL term; gsur, gkl and gn; per block: two partial sums
//   trpo_heads_finish_kernel  the partials added in a fixed order: out = {a_loss, kl}   (launched only when `out` is asked for)
//
// A streaming pass on ppo_loss_kernels.hip's plan, bound by the [M, A] reads: every array a requested output does not need is not
// touched (the line search's evaluation reads mu and actions, 8 A + 16 bytes per row; gn alone reads rmu and writes gn).  Stored rows
// are read once through the minibatch's index vector.
// Lane roles: column j of a row belongs to lane j / 4 of a group of S lanes, S = the power of two that holds ceil(A / 4) (S <= 32),
// so a wave holds 64 / S rows and a group reads its row as float4 (when A is a multiple of 4 and every base in use is 16-byte
// aligned; the same columns as four scalar accesses otherwise: the lane roles, and with them every sum's order, depend on A alone,
// so both paths give the same bits).
// Order of the sums.  Within a row: logp and the KL term in double, a lane over its (up to) four columns in ascending order, then an xor
// butterfly over the group (1, 2, .. S / 2) -- mms_ppo_loss's order.  Over rows: the group's first lane adds its rows in the order
// the block walks them (`iters` steps of 256 / S rows), in double; a full butterfly over the wave, the four waves in LDS as
// (w0 + w1) + (w2 + w3); block b stores its two partials at part[q * blocks + b].  The finish pass gives each of the two a wave: lane t
// adds part[q][t], part[q][t + 64], .. in ascending order, then the full butterfly; one division by M and one rounding to fp32.
// No atomics, no memset: every word of the workspace that the finish pass reads was written by the row pass of the same call.
// Built WITHOUT fast-math and without contraction (csrc/Makefile: PARAM_FLAGS): IEEE division, every product and sum rounded on its
// own, so gkl and gn have the bits of the CPU build's evaluation of trpo_loss_lane.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mms_lane.h"
#include "trpo_loss_lane.h"

namespace mms {

constexpr int kThThreads = 256;                 // 4 waves
constexpr int kThMaxBlocks = 1024;              // row blocks (partials per quantity): 4 per CU
constexpr int kThSums = 2;                      // a_loss, kl

struct TrpoHeadsArgs {
    const float *mu, *log_std, *rmu;
    const int64_t* indices;
    const float *actions, *adv, *old_mu, *old_sigma, *old_logp;
    float *out, *logp, *gsur, *gkl, *gn;
    double* part;
    int64_t M;
    float inv_m;
    int A, log2s, iters, blocks, dense_old_logp;
};

struct TrpoHeadsPlan { int log2s, iters, blocks; int64_t bytes; };

static TrpoHeadsPlan trpo_heads_plan(int64_t M, int A) {
    TrpoHeadsPlan p;
    p.log2s = 0;
    while ((4 << p.log2s) < A) p.log2s++;
    const int64_t rows = kThThreads >> p.log2s;                  // rows per step of a block
    const int64_t groups = (M + rows - 1) / rows;
    const int64_t iters = (groups + kThMaxBlocks - 1) / kThMaxBlocks;
    p.iters = (int)iters;
    p.blocks = (int)((groups + iters - 1) / iters);
    p.bytes = (((int64_t)kThSums * p.blocks * (int64_t)sizeof(double)) + 255) & ~(int64_t)255;
    return p;
}

int64_t trpo_heads_ws_bytes(int64_t M, int A) { return trpo_heads_plan(M, A).bytes; }

__device__ __forceinline__ double th_shfl_xor(double x, int m) { return __shfl_xor(x, m, 64); }

// the four columns col .. col + 3 of a row (columns past A: 0)
template <bool VEC>
__device__ __forceinline__ void th_load4(const float* row, int col, int A, float (&x)[4]) {
    if (VEC) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < A) v = *reinterpret_cast<const float4*>(row + col);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = (col + k < A) ? row[col + k] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void th_store4(float* row, int col, int A, const float (&d)[4]) {
    if (VEC) {
        if (col < A) *reinterpret_cast<float4*>(row + col) = make_float4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (col + k < A) row[col + k] = d[k];
    }
}

template <bool VEC>
__global__ void __launch_bounds__(kThThreads) trpo_heads_rows_kernel(TrpoHeadsArgs a) {
    __shared__ double s_sum[4][kThSums];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = 1 << a.log2s, sub = lane & (S - 1), col = 4 * sub, A = a.A;
    const int rows_per_wave = 64 >> a.log2s, rows_per_step = kThThreads >> a.log2s;
    // what the requested outputs need (uniform over the grid)
    const bool sums = a.out != nullptr;
    const bool want_lp = sums || a.logp != nullptr || a.gsur != nullptr;       // logp: mu, actions
    const bool want_r = sums || a.gsur != nullptr;                              // the ratio: old_logp, adv
    const bool want_kl = sums;                                                  // the KL term: mu, old_mu, old_sigma
    const bool want_om = sums || a.gkl != nullptr;
    const bool want_mu = want_lp || want_om;

    float l[4], einv[4], den[4], cden[4];
    th_load4<false>(a.log_std, col, A, l);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        ppo_col_consts(l[k], einv[k], den[k]);
        cden[k] = trpo_col_den(l[k], a.M);
    }

    double rsum[kThSums] = {0.0, 0.0};                  // this lane's rows (the group's first lane only): a_loss, kl

    for (int it = 0; it < a.iters; it++) {
        const int64_t row = ((int64_t)blockIdx.x * a.iters + it) * rows_per_step + wave * rows_per_wave + (lane >> a.log2s);
        const bool live = row < a.M;                                        // rows past M are neither read nor written
        float mu[4] = {0.f, 0.f, 0.f, 0.f}, act[4] = {0.f, 0.f, 0.f, 0.f}, om[4] = {0.f, 0.f, 0.f, 0.f}, os[4] = {0.f, 0.f, 0.f, 0.f};
        float rm[4] = {0.f, 0.f, 0.f, 0.f};
        int64_t src = 0;
        if (live) {
            src = a.indices ? a.indices[row] : row;
            if (want_mu) th_load4<VEC>(a.mu + row * (int64_t)A, col, A, mu);
            if (want_lp) th_load4<VEC>(a.actions + src * (int64_t)A, col, A, act);
            if (want_om) th_load4<VEC>(a.old_mu + src * (int64_t)A, col, A, om);
            if (want_kl) th_load4<VEC>(a.old_sigma + src * (int64_t)A, col, A, os);
            if (a.gn) th_load4<VEC>(a.rmu + row * (int64_t)A, col, A, rm);
        }
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        double logp = 0.0, kl = 0.0;
        if (want_lp) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float t = ppo_logp_term(act[k], mu[k], l[k], einv[k], z[k]);
                logp += (live && col + k < A) ? (double)t : 0.0;
            }
            for (int m = 1; m < S; m <<= 1) logp += th_shfl_xor(logp, m);
        }
        if (want_kl) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float u = ppo_kl_term(l[k], os[k], om[k], mu[k], den[k]);
                kl += (live && col + k < A) ? (double)u : 0.0;
            }
            for (int m = 1; m < S; m <<= 1) kl += th_shfl_xor(kl, m);
        }
        if (live) {
            float g = 0.f;
            if (want_r) {
                const TrpoRow r = trpo_row(logp, a.old_logp[a.dense_old_logp ? row : src], a.adv[src], a.inv_m);
                g = r.g;
                if (sums && sub == 0) rsum[0] += (double)r.term;
            }
            if (sums && sub == 0) rsum[1] += kl;
            if (a.logp && sub == 0) a.logp[row] = (float)logp;
            float d[4];
            if (a.gsur) {
#pragma unroll
                for (int k = 0; k < 4; k++) d[k] = trpo_gsur(g, z[k], einv[k]);
                th_store4<VEC>(a.gsur + row * (int64_t)A, col, A, d);
            }
            if (a.gkl) {
#pragma unroll
                for (int k = 0; k < 4; k++) d[k] = trpo_gkl(mu[k], om[k], cden[k]);
                th_store4<VEC>(a.gkl + row * (int64_t)A, col, A, d);
            }
            if (a.gn) {
#pragma unroll
                for (int k = 0; k < 4; k++) d[k] = trpo_gn(rm[k], cden[k]);
                th_store4<VEC>(a.gn + row * (int64_t)A, col, A, d);
            }
        }
    }

    if (!sums) return;                                                      // (uniform: no barrier is skipped by part of a block)
#pragma unroll
    for (int q = 0; q < kThSums; q++)
        for (int m = 1; m < 64; m <<= 1) rsum[q] += th_shfl_xor(rsum[q], m);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < kThSums; q++) s_sum[wave][q] = rsum[q];
    }
    __syncthreads();
    if (tid < kThSums) a.part[(int64_t)tid * a.blocks + blockIdx.x] = (s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid]);
}

// one workgroup of two waves: wave q adds quantity q's partials -- lane t adds p[t], p[t + 64], .. in ascending order (eight loads in
// flight; a slot past n adds 0.0, which changes nothing), then the full butterfly -- and its first lane stores the mean
__global__ void __launch_bounds__(64 * kThSums) trpo_heads_finish_kernel(TrpoHeadsArgs a) {
    const int lane = (int)threadIdx.x & 63, q = (int)threadIdx.x >> 6, n = a.blocks;
    const double* p = a.part + (int64_t)q * n;
    double s = 0.0;
    for (int base = 0; base < n; base += 64 * 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int i = base + 64 * u + lane;
            v[u] = i < n ? p[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) s += v[u];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += th_shfl_xor(s, m);
    if (lane == 0) a.out[q] = trpo_finish_mean(s, a.M);
}

// the launches of a checked call (mms_host.h: check_trpo_heads)
hipError_t launch_trpo_heads(int64_t M, int A, const float* mu, const float* log_std, const float* rmu, const int64_t* indices, const float* actions,
                             const float* adv, const float* old_mu, const float* old_sigma, const float* old_logp, int dense_old_logp, float* out,
                             float* logp, float* gsur, float* gkl, float* gn, void* workspace, hipStream_t s) {
    if (M < 1 || M > 0x7fffffff || A < 1 || A > MMS_PPO_LOSS_MAX_A) return hipErrorInvalidValue;     // (the entry's check refuses it with a message)
    const TrpoHeadsPlan p = trpo_heads_plan(M, A);
    TrpoHeadsArgs a = {};
    a.mu = mu; a.log_std = log_std; a.rmu = rmu; a.indices = indices;
    a.actions = actions; a.adv = adv; a.old_mu = old_mu; a.old_sigma = old_sigma; a.old_logp = old_logp;
    a.out = out; a.logp = logp; a.gsur = gsur; a.gkl = gkl; a.gn = gn;
    a.part = static_cast<double*>(workspace);
    a.M = M; a.inv_m = 1.0f / (float)M;
    a.A = A; a.log2s = p.log2s; a.iters = p.iters; a.blocks = p.blocks; a.dense_old_logp = dense_old_logp;
    // rows as float4: A a multiple of 4 makes every row of a 16-byte aligned base 16-byte aligned.  Every [*, A] base the call was
    // given counts, also one this subset of outputs does not read: the choice then does not depend on the subset.
    const uintptr_t bases = reinterpret_cast<uintptr_t>(mu) | reinterpret_cast<uintptr_t>(rmu) | reinterpret_cast<uintptr_t>(actions) |
                            reinterpret_cast<uintptr_t>(old_mu) | reinterpret_cast<uintptr_t>(old_sigma) | reinterpret_cast<uintptr_t>(gsur) |
                            reinterpret_cast<uintptr_t>(gkl) | reinterpret_cast<uintptr_t>(gn);
    const bool vec = (A % 4) == 0 && (bases & 15) == 0;
    const dim3 grid((unsigned)p.blocks), block(kThThreads);
    if (vec) hipLaunchKernelGGL((trpo_heads_rows_kernel<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((trpo_heads_rows_kernel<false>), grid, block, 0, s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || !out) return err;
    hipLaunchKernelGGL(trpo_heads_finish_kernel, dim3(1), dim3(64 * kThSums), 0, s, a);
    return hipGetLastError();
}

}  // namespace mms
