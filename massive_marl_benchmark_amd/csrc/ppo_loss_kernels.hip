// ppo_loss_kernels.hip -- the PPO update's loss head and its gradients for gfx950 (mms_ppo_loss, include/mms.h).
//
//   ppo_loss_rows_kernel    per row: logp, the KL term, the ratio, both clipped terms and dmu / dvalue; per block: partial sums
//   ppo_loss_finish_kernel  the partials added in a fixed order: the five scalars and dlog_std
//
// A streaming pass, 16 A + 32 bytes in and 4 A + 4 bytes out per row (mu, actions, old_mu, old_sigma; the index, the value and five
// stored scalars; dmu and dvalue), every stored row read once through the minibatch's index vector.
// Lane roles: column j of a row belongs to lane j / 4 of a group of S lanes, S = the power of two that holds ceil(A / 4) (S <= 32),
// so a wave holds 64 / S rows and a group reads its row as float4 (when A is a multiple of 4 and the bases are 16-byte aligned;
// the same columns as four scalar loads otherwise: the lane roles, and with them every sum's order, depend on A alone).
// Order of the sums.  Within a row: logp and the KL term in double, a lane over its (up to) four columns in ascending order, then an xor
// butterfly over the group (1, 2, .. S / 2).  Over rows: a lane adds what its group's rows give in the order the block walks them
// (`iters` steps of 256 / S rows), in double; the lanes of a wave that hold the same column meet in an xor butterfly (S .. 32), the four
// waves in LDS as (w0 + w1) + (w2 + w3); block b stores its 3 + A partials at part[q * blocks + b].  The finish pass gives quantity q
// a wave (the three scalar sums and the entropy share its last block): lane t adds part[q][t], part[q][t + 64], .. in ascending order,
// then the full butterfly; one rounding to fp32 at the end.
// No atomics, no memset: every word of the workspace that the finish pass reads was written by the row pass of the same call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mms_lane.h"
#include "ppo_loss_lane.h"

namespace mms {

constexpr int kPlThreads = 256;                 // 4 waves
constexpr int kPlMaxBlocks = 1024;              // row blocks (partials per quantity): 4 per CU
constexpr int kPlSums = 3;                      // surrogate, value loss, KL; then the A columns of dlog_std

struct PpoLossArgs {
    const float *mu, *log_std, *value;
    const int64_t* indices;
    const float *actions, *old_logp, *adv, *returns, *target_values, *old_mu, *old_sigma;
    float clip, value_coef, entropy_coef, inv_m;
    int clipped_value;
    float *out, *dmu, *dlog_std, *dvalue;
    double* part;
    int64_t M;
    int A, log2s, iters, blocks;
};

struct PpoLossPlan { int log2s, iters, blocks; int64_t bytes; };

static PpoLossPlan ppo_loss_plan(int64_t M, int A) {
    PpoLossPlan p;
    p.log2s = 0;
    while ((4 << p.log2s) < A) p.log2s++;
    const int64_t rows = kPlThreads >> p.log2s;                  // rows per step of a block
    const int64_t groups = (M + rows - 1) / rows;
    const int64_t iters = (groups + kPlMaxBlocks - 1) / kPlMaxBlocks;
    p.iters = (int)iters;
    p.blocks = (int)((groups + iters - 1) / iters);
    p.bytes = (((int64_t)(kPlSums + A) * p.blocks * (int64_t)sizeof(double)) + 255) & ~(int64_t)255;
    return p;
}

int64_t ppo_loss_ws_bytes(int64_t M, int A) { return ppo_loss_plan(M, A).bytes; }

__device__ __forceinline__ double pl_shfl_xor(double x, int m) { return __shfl_xor(x, m, 64); }

// the four columns 4 sub .. 4 sub + 3 of a row (columns past A: 0)
template <bool VEC>
__device__ __forceinline__ void pl_load4(const float* row, int col, int A, float (&x)[4]) {
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
__global__ void __launch_bounds__(kPlThreads) ppo_loss_rows_kernel(PpoLossArgs a) {
    __shared__ double s_col[4][MMS_PPO_LOSS_MAX_A];
    __shared__ double s_sum[4][kPlSums];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = 1 << a.log2s, sub = lane & (S - 1), col = 4 * sub, A = a.A;
    const int rows_per_wave = 64 >> a.log2s, rows_per_step = kPlThreads >> a.log2s;
    const bool grads = a.dmu != nullptr;

    float l[4], einv[4], den[4];
    pl_load4<false>(a.log_std, col, A, l);
#pragma unroll
    for (int k = 0; k < 4; k++) ppo_col_consts(l[k], einv[k], den[k]);

    double csum[4] = {0.0, 0.0, 0.0, 0.0};              // this lane's four columns of sum_i g_i (2 z_ij^2 - 2)
    double rsum[kPlSums] = {0.0, 0.0, 0.0};             // this lane's rows (the group's first lane only): surrogate, value loss, KL

    for (int it = 0; it < a.iters; it++) {
        const int64_t row = ((int64_t)blockIdx.x * a.iters + it) * rows_per_step + wave * rows_per_wave + (lane >> a.log2s);
        const bool live = row < a.M;                                        // rows past M are neither read nor written
        float mu[4] = {0.f, 0.f, 0.f, 0.f}, act[4] = {0.f, 0.f, 0.f, 0.f}, om[4] = {0.f, 0.f, 0.f, 0.f}, os[4] = {0.f, 0.f, 0.f, 0.f};
        int64_t src = 0;
        if (live) {
            src = a.indices ? a.indices[row] : row;
            pl_load4<VEC>(a.mu + row * (int64_t)A, col, A, mu);
            pl_load4<VEC>(a.actions + src * (int64_t)A, col, A, act);
            pl_load4<VEC>(a.old_mu + src * (int64_t)A, col, A, om);
            pl_load4<VEC>(a.old_sigma + src * (int64_t)A, col, A, os);
        }
        float z[4];
        double logp = 0.0, kl = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool on = live && col + k < A;
            const float t = ppo_logp_term(act[k], mu[k], l[k], einv[k], z[k]);
            const float u = ppo_kl_term(l[k], os[k], om[k], mu[k], den[k]);
            logp += on ? (double)t : 0.0;
            kl += on ? (double)u : 0.0;
        }
        for (int m = 1; m < S; m <<= 1) {
            logp += pl_shfl_xor(logp, m);
            kl += pl_shfl_xor(kl, m);
        }
        if (live) {
            const PpoRow r = ppo_row(logp, a.old_logp[src], a.adv[src], a.value[row], a.returns[src], a.target_values[src], a.clip, a.value_coef,
                                     a.clipped_value != 0, a.inv_m);
            if (sub == 0) {
                rsum[0] += (double)r.surrogate;
                rsum[1] += (double)r.value_loss;
                rsum[2] += kl;
                if (grads) a.dvalue[row] = r.dvalue;
            }
            if (grads) {
                float d[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    d[k] = ppo_dmu(r.g, z[k], einv[k]);
                    if (col + k < A) csum[k] += (double)ppo_dlog_std_term(r.g, z[k]);
                }
                float* dst = a.dmu + row * (int64_t)A + col;
                if (VEC) {
                    if (col < A) *reinterpret_cast<float4*>(dst) = make_float4(d[0], d[1], d[2], d[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (col + k < A) dst[k] = d[k];
                }
            }
        }
    }

    // the block's partials: the lanes of a wave that hold the same columns, then the four waves
    for (int m = S; m < 64; m <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) csum[k] += pl_shfl_xor(csum[k], m);
    }
#pragma unroll
    for (int q = 0; q < kPlSums; q++)
        for (int m = 1; m < 64; m <<= 1) rsum[q] += pl_shfl_xor(rsum[q], m);
    if (lane < S) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (col + k < A) s_col[wave][col + k] = csum[k];
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < kPlSums; q++) s_sum[wave][q] = rsum[q];
    }
    __syncthreads();
    const int64_t nb = a.blocks;
    if (tid < kPlSums) a.part[tid * nb + blockIdx.x] = (s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid]);
    if (grads && tid < A) a.part[(kPlSums + tid) * nb + blockIdx.x] = (s_col[0][tid] + s_col[1][tid]) + (s_col[2][tid] + s_col[3][tid]);
}

// one quantity's partials: lane t adds p[t], p[t + 64], .. in ascending order (eight loads in flight; a slot past n adds 0.0, which
// changes nothing), then the full butterfly
__device__ __forceinline__ double pl_part_sum(const double* p, int n, int lane) {
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
    for (int m = 32; m >= 1; m >>= 1) s += pl_shfl_xor(s, m);
    return s;
}

// the last block: its four waves take the surrogate, value loss and KL sums and the entropy, thread 0 forms the five scalars; with
// gradients, the blocks before it: wave w of the grid takes column w of dlog_std
__global__ void __launch_bounds__(kPlThreads) ppo_loss_finish_kernel(PpoLossArgs a) {
    __shared__ double s_tot[4];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int A = a.A, nb = a.blocks;
    if (blockIdx.x + 1 < gridDim.x) {
        const int w = (int)blockIdx.x * (kPlThreads / 64) + wave;
        if (w >= A) return;
        const double s = pl_part_sum(a.part + (int64_t)(kPlSums + w) * nb, nb, lane);
        if (lane == 0) a.dlog_std[w] = ppo_finish_dlog_std(s, a.entropy_coef);
        return;
    }
    double t;
    if (wave < kPlSums) {
        t = pl_part_sum(a.part + (int64_t)wave * nb, nb, lane);
    } else {
        t = 0.0;
        for (int j = lane; j < A; j += 64) t += (double)ppo_entropy_term(a.log_std[j]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) t += pl_shfl_xor(t, m);
    }
    if (lane == 0) s_tot[wave] = t;
    __syncthreads();
    if (threadIdx.x == 0) ppo_finish_scalars(s_tot[0], s_tot[1], s_tot[2], s_tot[3], a.M, a.value_coef, a.entropy_coef, a.out);
}

hipError_t launch_ppo_loss(int64_t M, int A, const float* mu, const float* log_std, const float* value, const int64_t* indices, const float* actions,
                           const float* old_logp, const float* adv, const float* returns, const float* target_values, const float* old_mu,
                           const float* old_sigma, float clip, float value_coef, float entropy_coef, int clipped_value, float* out, float* dmu,
                           float* dlog_std, float* dvalue, void* workspace, hipStream_t s) {
    if (M < 1 || M > 0x7fffffff || A < 1 || A > MMS_PPO_LOSS_MAX_A) return hipErrorInvalidValue;     // (the entry's check refuses it with a message)
    const PpoLossPlan p = ppo_loss_plan(M, A);
    PpoLossArgs a = {};
    a.mu = mu; a.log_std = log_std; a.value = value; a.indices = indices;
    a.actions = actions; a.old_logp = old_logp; a.adv = adv; a.returns = returns; a.target_values = target_values; a.old_mu = old_mu; a.old_sigma = old_sigma;
    a.clip = clip; a.value_coef = value_coef; a.entropy_coef = entropy_coef; a.inv_m = 1.0f / (float)M;
    a.clipped_value = clipped_value;
    a.out = out; a.dmu = dmu; a.dlog_std = dlog_std; a.dvalue = dvalue;
    a.part = static_cast<double*>(workspace);
    a.M = M; a.A = A; a.log2s = p.log2s; a.iters = p.iters; a.blocks = p.blocks;
    // rows as float4: A a multiple of 4 makes every row of a 16-byte aligned base 16-byte aligned
    const uintptr_t bases = reinterpret_cast<uintptr_t>(mu) | reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(old_mu) |
                            reinterpret_cast<uintptr_t>(old_sigma) | reinterpret_cast<uintptr_t>(dmu);
    const bool vec = (A % 4) == 0 && (bases & 15) == 0;
    const dim3 grid((unsigned)p.blocks), block(kPlThreads);
    if (vec) hipLaunchKernelGGL((ppo_loss_rows_kernel<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ppo_loss_rows_kernel<false>), grid, block, 0, s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const unsigned column_blocks = dmu ? (unsigned)((A + 3) / 4) : 0u;
    hipLaunchKernelGGL(ppo_loss_finish_kernel, dim3(column_blocks + 1), block, 0, s, a);
    return hipGetLastError();
}

}  // namespace mms
