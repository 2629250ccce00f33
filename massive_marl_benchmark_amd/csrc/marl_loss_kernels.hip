// marl_loss_kernels.hip -- the MAPPO / HAPPO update's loss head and its gradients for gfx950 (mms_marl_ppo_loss, include/mms.h).
//
//   marl_mask_sum_kernel     only with a mask flag: sum_i m_i over the minibatch, one double per block (at most 64 blocks)
//   marl_loss_rows_kernel    per row: the per-dimension logp, the ratio, both surrogate terms, the value loss and dmu / dvalue /
//                            row_logp; per block: partial sums
//   marl_loss_finish_kernel  the partials added in a fixed order: the five scalars and dstd
//
// A streaming pass, 12 A + 28 bytes in and 4 A + 4 bytes out per row with both mask flags off and no factor (mu, actions, old_logp;
// the index, the value and three stored scalars; dmu and dvalue), every stored row read once through the minibatch's index vector
// and each field's own row pitch (a SeparatedReplayBuffer's tensors, or one agent's strided view of the shared ones).
// Lane roles, as ppo_loss_kernels.hip: column j of a row belongs to lane j / 4 of a group of S lanes, S = the power of two that holds
// ceil(A / 4) (S <= 32), so a wave holds 64 / S rows and a group reads its row as float4 (when A and both wide pitches are multiples
// of 4 and the bases are 16-byte aligned; the same columns as four scalar loads otherwise: the lane roles, and with them every sum's
// order, depend on A alone).
// Order of the sums.  Within a row: sum_j (logp_ij - old_logp_ij) and sum_j logp_ij in double, a lane over its (up to) four columns in
// ascending order, then an xor butterfly over the group (1, 2, .. S / 2).  Over rows: a lane adds what its group's rows give in the
// order the block walks them (`iters` steps of 256 / S rows), in double; the lanes of a wave that hold the same column meet in an xor
// butterfly (S .. 32), the four waves in LDS as (w0 + w1) + (w2 + w3); block b stores its 3 + A partials at part[q * blocks + b].
// The finish pass gives quantity q a wave (the three scalar sums and the entropy share its last block): lane t adds part[q][t],
// part[q][t + 64], .. in ascending order, then the full butterfly; one rounding to fp32 at the end.
// The mask sum: thread t of block b adds rows 256 b + t, + 256 nb, .. in ascending order in double, the full butterfly, the four waves
// as above; every later block adds the nb <= 64 partials as one lane each and the full butterfly, so all see the same total.
// No atomics, no memset: every word of the workspace that a pass reads was written by an earlier pass of the same call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marl_loss_lane.h"
#include "mms_lane.h"

namespace mms {

constexpr int kMlThreads = 256;                 // 4 waves
constexpr int kMlMaxBlocks = 1024;              // row blocks (partials per quantity): 4 per CU
constexpr int kMlSums = 3;                      // surrogate, value loss, ratio; then the A columns of dstd
constexpr int kMlMaskBlocks = 64;               // partials of the mask sum: one per lane of a wave

struct MarlLossArgs {
    const float *mu, *std, *value;
    const int64_t* indices;
    mms_marl_loss_fields f;
    float clip, value_coef, entropy_coef, delta;
    int huber, clipped_value, policy_masks, value_masks, use_norm;
    const float *norm_mean, *norm_var;
    float *out, *dmu, *dstd, *dvalue, *row_logp;
    double *part, *msum;
    int64_t M;
    int A, log2s, iters, blocks, mask_blocks;
};

struct MarlLossPlan { int log2s, iters, blocks, mask_blocks; int64_t bytes; };

static MarlLossPlan marl_loss_plan(int64_t M, int A) {
    MarlLossPlan p;
    p.log2s = 0;
    while ((4 << p.log2s) < A) p.log2s++;
    const int64_t rows = kMlThreads >> p.log2s;                  // rows per step of a block
    const int64_t groups = (M + rows - 1) / rows;
    const int64_t iters = (groups + kMlMaxBlocks - 1) / kMlMaxBlocks;
    p.iters = (int)iters;
    p.blocks = (int)((groups + iters - 1) / iters);
    const int64_t mb = (M + kMlThreads - 1) / kMlThreads;
    p.mask_blocks = (int)(mb < kMlMaskBlocks ? mb : kMlMaskBlocks);
    p.bytes = ((((int64_t)(kMlSums + A) * p.blocks + kMlMaskBlocks) * (int64_t)sizeof(double)) + 255) & ~(int64_t)255;
    return p;
}

int64_t marl_loss_ws_bytes(int64_t M, int A) { return marl_loss_plan(M, A).bytes; }

__device__ __forceinline__ double ml_shfl_xor(double x, int m) { return __shfl_xor(x, m, 64); }

__device__ __forceinline__ double ml_wave_sum(double s) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += ml_shfl_xor(s, m);
    return s;
}

// the four columns col .. col + 3 of a row (columns past A: 0)
template <bool VEC>
__device__ __forceinline__ void ml_load4(const float* row, int col, int A, float (&x)[4]) {
    if (VEC) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < A) v = *reinterpret_cast<const float4*>(row + col);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = (col + k < A) ? row[col + k] : 0.f;
    }
}

// sum_i m_i as the later passes form it from the mask pass's partials: the same value in every lane of every block
__device__ __forceinline__ double ml_mask_total(const MarlLossArgs& a, int lane) {
    return ml_wave_sum(lane < a.mask_blocks ? a.msum[lane] : 0.0);
}

__global__ void __launch_bounds__(kMlThreads) marl_mask_sum_kernel(MarlLossArgs a) {
    __shared__ double s_w[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s = 0.0;
    for (int64_t row = (int64_t)blockIdx.x * kMlThreads + tid; row < a.M; row += (int64_t)gridDim.x * kMlThreads) {
        const int64_t src = a.indices ? a.indices[row] : row;
        s += (double)a.f.active_masks.base[src * a.f.active_masks.pitch];
    }
    s = ml_wave_sum(s);
    if (lane == 0) s_w[wave] = s;
    __syncthreads();
    if (tid == 0) a.msum[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

template <bool VEC>
__global__ void __launch_bounds__(kMlThreads) marl_loss_rows_kernel(MarlLossArgs a) {
    __shared__ double s_col[4][MMS_MARL_LOSS_MAX_A];
    __shared__ double s_sum[4][kMlSums];
    __shared__ MarlCol s_c[MMS_MARL_LOSS_MAX_A];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = 1 << a.log2s, sub = lane & (S - 1), col = 4 * sub, A = a.A;
    const int rows_per_wave = 64 >> a.log2s, rows_per_step = kMlThreads >> a.log2s;
    const bool grads = a.dmu != nullptr, pm = a.policy_masks != 0, vm = a.value_masks != 0;

    // the per-column constants, formed in double once per block
    if (tid < A) s_c[tid] = marl_col_consts(a.std[tid]);
    __syncthreads();
    MarlCol c[4];
#pragma unroll
    for (int k = 0; k < 4; k++) c[k] = s_c[col + k < A ? col + k : 0];

    MarlScalars sc;
    sc.clip = a.clip; sc.value_coef = a.value_coef; sc.delta = a.delta;
    sc.huber = a.huber != 0; sc.clipped_value = a.clipped_value != 0; sc.use_norm = a.use_norm != 0;
    sc.norm_mean = 0.0; sc.norm_inv_sd = 1.0;
    if (sc.use_norm) {
        sc.norm_mean = (double)a.norm_mean[0];
        sc.norm_inv_sd = 1.0 / sqrt((double)a.norm_var[0]);
    }
    const double inv_m = 1.0 / (double)a.M;
    double inv_msum = 0.0;
    if (pm || vm) inv_msum = 1.0 / ml_mask_total(a, lane);

    double csum[4] = {0.0, 0.0, 0.0, 0.0};              // this lane's four columns of sum_i g_i ((a - mu)^2 / std^3 - 1 / std)
    double rsum[kMlSums] = {0.0, 0.0, 0.0};             // this lane's rows (the group's first lane only): surrogate, value loss, ratio

    for (int it = 0; it < a.iters; it++) {
        const int64_t row = ((int64_t)blockIdx.x * a.iters + it) * rows_per_step + wave * rows_per_wave + (lane >> a.log2s);
        const bool live = row < a.M;                                        // rows past M are neither read nor written
        float mu[4] = {0.f, 0.f, 0.f, 0.f}, act[4] = {0.f, 0.f, 0.f, 0.f}, olp[4] = {0.f, 0.f, 0.f, 0.f};
        int64_t src = 0;
        if (live) {
            src = a.indices ? a.indices[row] : row;
            ml_load4<VEC>(a.mu + row * (int64_t)A, col, A, mu);
            ml_load4<VEC>(a.f.actions.base + src * a.f.actions.pitch, col, A, act);
            ml_load4<VEC>(a.f.old_logp.base + src * a.f.old_logp.pitch, col, A, olp);
        }
        float d[4];
        double dlogp = 0.0, logp = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool on = live && col + k < A;
            const double t = marl_logp_term(act[k], mu[k], c[k], d[k]);
            dlogp += on ? t - (double)olp[k] : 0.0;
            logp += on ? t : 0.0;
        }
        for (int m = 1; m < S; m <<= 1) {
            dlogp += ml_shfl_xor(dlogp, m);
            logp += ml_shfl_xor(logp, m);
        }
        if (live) {
            const float mask = (pm || vm) ? a.f.active_masks.base[src * a.f.active_masks.pitch] : 1.0f;
            const float fac = a.f.factor.base ? a.f.factor.base[src * a.f.factor.pitch] : 1.0f;
            const MarlRow r = marl_row(dlogp, a.f.adv.base[src * a.f.adv.pitch], fac, a.value[row], a.f.value_preds.base[src * a.f.value_preds.pitch],
                                       a.f.returns.base[src * a.f.returns.pitch], sc, pm ? (double)mask * inv_msum : inv_m, vm ? (double)mask * inv_msum : inv_m);
            if (sub == 0) {
                rsum[0] += pm ? (double)mask * (double)r.surrogate : (double)r.surrogate;
                rsum[1] += vm ? (double)mask * (double)r.value_loss : (double)r.value_loss;
                rsum[2] += (double)r.ratio;
                if (grads) a.dvalue[row] = r.dvalue;
                if (a.row_logp) a.row_logp[row] = (float)logp;
            }
            if (grads) {
                float g[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    g[k] = marl_dmu(r.g, d[k], c[k]);
                    if (col + k < A) csum[k] += marl_dstd_term(r.g, d[k], c[k]);
                }
                float* dst = a.dmu + row * (int64_t)A + col;
                if (VEC) {
                    if (col < A) *reinterpret_cast<float4*>(dst) = make_float4(g[0], g[1], g[2], g[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (col + k < A) dst[k] = g[k];
                }
            }
        }
    }

    // the block's partials: the lanes of a wave that hold the same columns, then the four waves
    for (int m = S; m < 64; m <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) csum[k] += ml_shfl_xor(csum[k], m);
    }
#pragma unroll
    for (int q = 0; q < kMlSums; q++) rsum[q] = ml_wave_sum(rsum[q]);
    if (lane < S) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (col + k < A) s_col[wave][col + k] = csum[k];
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < kMlSums; q++) s_sum[wave][q] = rsum[q];
    }
    __syncthreads();
    const int64_t nb = a.blocks;
    if (tid < kMlSums) a.part[tid * nb + blockIdx.x] = (s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid]);
    if (grads && tid < A) a.part[(kMlSums + tid) * nb + blockIdx.x] = (s_col[0][tid] + s_col[1][tid]) + (s_col[2][tid] + s_col[3][tid]);
}

// one quantity's partials: lane t adds p[t], p[t + 64], .. in ascending order (eight loads in flight; a slot past n adds 0.0, which
// changes nothing), then the full butterfly
__device__ __forceinline__ double ml_part_sum(const double* p, int n, int lane) {
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
    return ml_wave_sum(s);
}

// the last block: its four waves take the surrogate, value loss and ratio sums and the entropy, thread 0 forms the five scalars; with
// gradients, the blocks before it: wave w of the grid takes column w of dstd
__global__ void __launch_bounds__(kMlThreads) marl_loss_finish_kernel(MarlLossArgs a) {
    __shared__ double s_tot[4];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int A = a.A, nb = a.blocks;
    const double ent_scale = a.policy_masks ? 1.0 : 1.0 / (double)A;
    if (blockIdx.x + 1 < gridDim.x) {
        const int w = (int)blockIdx.x * (kMlThreads / 64) + wave;
        if (w >= A) return;
        const double s = ml_part_sum(a.part + (int64_t)(kMlSums + w) * nb, nb, lane);
        if (lane == 0) a.dstd[w] = marl_finish_dstd(s, a.std[w], a.entropy_coef, ent_scale);
        return;
    }
    double t;
    if (wave < kMlSums) {
        t = ml_part_sum(a.part + (int64_t)wave * nb, nb, lane);
    } else {
        t = 0.0;
        for (int j = lane; j < A; j += 64) t += marl_entropy_term(a.std[j]);
        t = ml_wave_sum(t);
    }
    const double msum = (a.policy_masks || a.value_masks) ? ml_mask_total(a, lane) : 0.0;
    if (lane == 0) s_tot[wave] = t;
    __syncthreads();
    if (threadIdx.x == 0)
        marl_finish_scalars(s_tot[0], s_tot[1], s_tot[2], s_tot[3], a.policy_masks ? msum : (double)a.M, a.value_masks ? msum : (double)a.M, ent_scale, a.M,
                            a.value_coef, a.entropy_coef, a.out);
}

hipError_t launch_marl_ppo_loss(int64_t M, int A, const float* mu, const float* std, const float* value, const int64_t* indices,
                                const mms_marl_loss_fields& f, float clip, float value_coef, float entropy_coef, float delta, int huber, int clipped_value,
                                int policy_masks, int value_masks, int use_norm, const float* norm_mean, const float* norm_var, float* out, float* dmu,
                                float* dstd, float* dvalue, float* row_logp, void* workspace, hipStream_t s) {
    if (M < 1 || M > 0x7fffffff || A < 1 || A > MMS_MARL_LOSS_MAX_A) return hipErrorInvalidValue;    // (the entry's check refuses it with a message)
    const MarlLossPlan p = marl_loss_plan(M, A);
    MarlLossArgs a = {};
    a.mu = mu; a.std = std; a.value = value; a.indices = indices; a.f = f;
    a.clip = clip; a.value_coef = value_coef; a.entropy_coef = entropy_coef; a.delta = delta;
    a.huber = huber; a.clipped_value = clipped_value; a.policy_masks = policy_masks; a.value_masks = value_masks; a.use_norm = use_norm;
    a.norm_mean = norm_mean; a.norm_var = norm_var;
    a.out = out; a.dmu = dmu; a.dstd = dstd; a.dvalue = dvalue; a.row_logp = row_logp;
    a.part = static_cast<double*>(workspace);
    a.msum = a.part + (int64_t)(kMlSums + A) * p.blocks;
    a.M = M; a.A = A; a.log2s = p.log2s; a.iters = p.iters; a.blocks = p.blocks; a.mask_blocks = p.mask_blocks;
    const dim3 block(kMlThreads);
    if (policy_masks || value_masks) {
        hipLaunchKernelGGL(marl_mask_sum_kernel, dim3((unsigned)p.mask_blocks), block, 0, s, a);
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    // rows as float4: A and the wide pitches multiples of 4 make every row of a 16-byte aligned base 16-byte aligned
    const uintptr_t bases = reinterpret_cast<uintptr_t>(mu) | reinterpret_cast<uintptr_t>(f.actions.base) | reinterpret_cast<uintptr_t>(f.old_logp.base) |
                            reinterpret_cast<uintptr_t>(dmu);
    const bool vec = (A % 4) == 0 && ((f.actions.pitch | f.old_logp.pitch) % 4) == 0 && (bases & 15) == 0;
    const dim3 grid((unsigned)p.blocks);
    if (vec) hipLaunchKernelGGL((marl_loss_rows_kernel<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((marl_loss_rows_kernel<false>), grid, block, 0, s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const unsigned column_blocks = dmu ? (unsigned)((A + 3) / 4) : 0u;
    hipLaunchKernelGGL(marl_loss_finish_kernel, dim3(column_blocks + 1), block, 0, s, a);
    return hipGetLastError();
}

}  // namespace mms
