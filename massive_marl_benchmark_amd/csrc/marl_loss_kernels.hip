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
// mms_marl_ppo_loss_group (the end of this file) runs the same passes for up to MMS_MAX_GROUPS agents with the group on blockIdx.y.
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

// The three passes as device functions of (the call's arguments, this block's index bx of gx): the kernels of the single entry call
// them with their own grid, the grouped entry's (below) with group blockIdx.y's arguments -- one copy of every sum's order.
__device__ __forceinline__ void ml_mask_sum(const MarlLossArgs& a, int bx, int gx, double (&s_w)[4]) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s = 0.0;
    for (int64_t row = (int64_t)bx * kMlThreads + tid; row < a.M; row += (int64_t)gx * kMlThreads) {
        const int64_t src = a.indices ? a.indices[row] : row;
        s += (double)a.f.active_masks.base[src * a.f.active_masks.pitch];
    }
    s = ml_wave_sum(s);
    if (lane == 0) s_w[wave] = s;
    __syncthreads();
    if (tid == 0) a.msum[bx] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

__global__ void __launch_bounds__(kMlThreads) marl_mask_sum_kernel(MarlLossArgs a) {
    __shared__ double s_w[4];
    ml_mask_sum(a, (int)blockIdx.x, (int)gridDim.x, s_w);
}

struct MlRowsLds {
    double col[4][MMS_MARL_LOSS_MAX_A];
    double sum[4][kMlSums];
    MarlCol c[MMS_MARL_LOSS_MAX_A];
};

template <bool VEC>
__device__ __forceinline__ void ml_rows(const MarlLossArgs& a, int bx, MlRowsLds& lds) {
    double (&s_col)[4][MMS_MARL_LOSS_MAX_A] = lds.col;
    double (&s_sum)[4][kMlSums] = lds.sum;
    MarlCol (&s_c)[MMS_MARL_LOSS_MAX_A] = lds.c;
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
        const int64_t row = ((int64_t)bx * a.iters + it) * rows_per_step + wave * rows_per_wave + (lane >> a.log2s);
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
    if (tid < kMlSums) a.part[tid * nb + bx] = (s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid]);
    if (grads && tid < A) a.part[(kMlSums + tid) * nb + bx] = (s_col[0][tid] + s_col[1][tid]) + (s_col[2][tid] + s_col[3][tid]);
}

template <bool VEC>
__global__ void __launch_bounds__(kMlThreads) marl_loss_rows_kernel(MarlLossArgs a) {
    __shared__ MlRowsLds lds;
    ml_rows<VEC>(a, (int)blockIdx.x, lds);
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
__device__ __forceinline__ void ml_finish(const MarlLossArgs& a, int bx, int gx, double (&s_tot)[4]) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int A = a.A, nb = a.blocks;
    const double ent_scale = a.policy_masks ? 1.0 : 1.0 / (double)A;
    if (bx + 1 < gx) {
        const int w = bx * (kMlThreads / 64) + wave;
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

__global__ void __launch_bounds__(kMlThreads) marl_loss_finish_kernel(MarlLossArgs a) {
    __shared__ double s_tot[4];
    ml_finish(a, (int)blockIdx.x, (int)gridDim.x, s_tot);
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

// ---- mms_marl_ppo_loss_group: the same three passes with the group on blockIdx.y --------------------------------------------------
// A pass builds group g's MarlLossArgs from per-member arrays and runs the single entry's device function on it, so group g's results
// are the single entry's bits.  The arrays a pass needs travel in its kernel arguments where they fit beside each other (4 KB); the
// twelve words per group that do not fit beside the rows pass's eleven (MlgTable) ride in the FIRST launch's arguments, whose block
// (0, 0) stores them at the head of the workspace, and the rows pass reads them from there behind the kernel boundary.  With a mask flag
// the first launch is also the mask-sum pass (it holds what that needs itself); without one it is a single block.
// Workspace: MlgTable, then per group the single entry's region (marl_loss_plan(M, A).bytes: the partials, then the mask partials).

struct MlgTable {
    const float* std[MMS_MAX_GROUPS];
    const float* norm_mean[MMS_MAX_GROUPS];
    const float* norm_var[MMS_MAX_GROUPS];
    const float* mask_base[MMS_MAX_GROUPS];
    const float* factor_base[MMS_MAX_GROUPS];
    int64_t pitch[7][MMS_MAX_GROUPS];           // in the order of mms_marl_loss_fields
};
static_assert(sizeof(MlgTable) % 256 == 0, "the groups' regions behind the table stay 256-byte aligned");

struct MlgShared {
    char* ws;
    int64_t M, group_bytes;
    float clip, value_coef, entropy_coef, delta;
    int huber, clipped_value, policy_masks, value_masks, use_norm;
    int A, log2s, iters, blocks, mask_blocks;
};

struct MlgFirstArgs {
    MlgTable t;
    const int64_t* indices[MMS_MAX_GROUPS];
    MlgShared s;
};

struct MlgRowsArgs {
    const float* mu[MMS_MAX_GROUPS];
    const float* value[MMS_MAX_GROUPS];
    const int64_t* indices[MMS_MAX_GROUPS];
    const float* actions[MMS_MAX_GROUPS];
    const float* old_logp[MMS_MAX_GROUPS];
    const float* adv[MMS_MAX_GROUPS];
    const float* value_preds[MMS_MAX_GROUPS];
    const float* returns[MMS_MAX_GROUPS];
    float* dmu[MMS_MAX_GROUPS];
    float* dvalue[MMS_MAX_GROUPS];
    float* row_logp[MMS_MAX_GROUPS];
    uint32_t vec;                               // bit g: group g's rows as float4 (the single entry's rule)
    MlgShared s;
};

struct MlgFinishArgs {
    const float* std[MMS_MAX_GROUPS];
    float* out[MMS_MAX_GROUPS];
    float* dstd[MMS_MAX_GROUPS];
    MlgShared s;
};
static_assert(sizeof(MlgFirstArgs) <= 3584 && sizeof(MlgRowsArgs) <= 3584 && sizeof(MlgFinishArgs) <= 3584, "kernel arguments: 4 KB limit");

// what every pass takes from the shared part, and group g's region of the workspace
__device__ __forceinline__ MarlLossArgs mlg_common(const MlgShared& s, int g) {
    MarlLossArgs a = {};
    a.clip = s.clip; a.value_coef = s.value_coef; a.entropy_coef = s.entropy_coef; a.delta = s.delta;
    a.huber = s.huber; a.clipped_value = s.clipped_value; a.policy_masks = s.policy_masks; a.value_masks = s.value_masks; a.use_norm = s.use_norm;
    a.M = s.M; a.A = s.A; a.log2s = s.log2s; a.iters = s.iters; a.blocks = s.blocks; a.mask_blocks = s.mask_blocks;
    a.part = reinterpret_cast<double*>(s.ws + (int64_t)sizeof(MlgTable) + (int64_t)g * s.group_bytes);
    a.msum = a.part + (int64_t)(kMlSums + s.A) * s.blocks;
    return a;
}

__global__ void __launch_bounds__(kMlThreads) marl_loss_group_first_kernel(MlgFirstArgs k) {
    __shared__ double s_w[4];
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        const uint64_t* src = reinterpret_cast<const uint64_t*>(&k.t);
        uint64_t* dst = reinterpret_cast<uint64_t*>(k.s.ws);
        for (int i = (int)threadIdx.x; i < (int)(sizeof(MlgTable) / 8); i += kMlThreads) dst[i] = src[i];
    }
    if (!(k.s.policy_masks || k.s.value_masks)) return;
    const int g = (int)blockIdx.y;
    MarlLossArgs a = mlg_common(k.s, g);
    a.indices = k.indices[g];
    a.f.active_masks.base = k.t.mask_base[g];
    a.f.active_masks.pitch = k.t.pitch[5][g];
    ml_mask_sum(a, (int)blockIdx.x, (int)gridDim.x, s_w);
}

__global__ void __launch_bounds__(kMlThreads) marl_loss_group_rows_kernel(MlgRowsArgs k) {
    __shared__ MlRowsLds lds;
    const int g = (int)blockIdx.y;
    const MlgTable* t = reinterpret_cast<const MlgTable*>(k.s.ws);
    MarlLossArgs a = mlg_common(k.s, g);
    a.mu = k.mu[g]; a.std = t->std[g]; a.value = k.value[g]; a.indices = k.indices[g];
    a.f.actions = {k.actions[g], t->pitch[0][g]};
    a.f.old_logp = {k.old_logp[g], t->pitch[1][g]};
    a.f.adv = {k.adv[g], t->pitch[2][g]};
    a.f.value_preds = {k.value_preds[g], t->pitch[3][g]};
    a.f.returns = {k.returns[g], t->pitch[4][g]};
    a.f.active_masks = {t->mask_base[g], t->pitch[5][g]};
    a.f.factor = {t->factor_base[g], t->pitch[6][g]};
    a.norm_mean = t->norm_mean[g]; a.norm_var = t->norm_var[g];
    a.dmu = k.dmu[g]; a.dvalue = k.dvalue[g]; a.row_logp = k.row_logp[g];
    if ((k.vec >> g) & 1u) ml_rows<true>(a, (int)blockIdx.x, lds);
    else ml_rows<false>(a, (int)blockIdx.x, lds);
}

__global__ void __launch_bounds__(kMlThreads) marl_loss_group_finish_kernel(MlgFinishArgs k) {
    __shared__ double s_tot[4];
    const int g = (int)blockIdx.y;
    MarlLossArgs a = mlg_common(k.s, g);
    a.std = k.std[g]; a.out = k.out[g]; a.dstd = k.dstd[g];
    if (blockIdx.x + 1 < gridDim.x && !a.dstd) return;              // the column blocks of a group that asked for no gradients
    ml_finish(a, (int)blockIdx.x, (int)gridDim.x, s_tot);
}

int64_t marl_loss_group_ws_bytes(int groups, int64_t M, int A) { return (int64_t)sizeof(MlgTable) + (int64_t)groups * marl_loss_plan(M, A).bytes; }

hipError_t launch_marl_ppo_loss_group(int groups, int64_t M, int A, const mms_marl_loss_group* table, float clip, float value_coef, float entropy_coef,
                                      float delta, int huber, int clipped_value, int policy_masks, int value_masks, int use_norm, void* workspace,
                                      hipStream_t s) {
    if (groups < 1 || groups > MMS_MAX_GROUPS || M < 1 || M > 0x7fffffff || A < 1 || A > MMS_MARL_LOSS_MAX_A || !table) return hipErrorInvalidValue;
    const MarlLossPlan p = marl_loss_plan(M, A);
    MlgShared sh = {};
    sh.ws = static_cast<char*>(workspace); sh.M = M; sh.group_bytes = p.bytes;
    sh.clip = clip; sh.value_coef = value_coef; sh.entropy_coef = entropy_coef; sh.delta = delta;
    sh.huber = huber; sh.clipped_value = clipped_value; sh.policy_masks = policy_masks; sh.value_masks = value_masks; sh.use_norm = use_norm;
    sh.A = A; sh.log2s = p.log2s; sh.iters = p.iters; sh.blocks = p.blocks; sh.mask_blocks = p.mask_blocks;
    MlgFirstArgs first = {};
    MlgRowsArgs rows = {};
    MlgFinishArgs fin = {};
    first.s = rows.s = fin.s = sh;
    bool any_grads = false;
    for (int g = 0; g < groups; g++) {
        const mms_marl_loss_group& t = table[g];
        const mms_rows* f = &t.fields.actions;
        first.t.std[g] = t.std; first.t.norm_mean[g] = t.norm_mean; first.t.norm_var[g] = t.norm_var;
        first.t.mask_base[g] = t.fields.active_masks.base; first.t.factor_base[g] = t.fields.factor.base;
        for (int q = 0; q < 7; q++) first.t.pitch[q][g] = f[q].pitch;
        first.indices[g] = t.indices;
        rows.mu[g] = t.mu; rows.value[g] = t.value; rows.indices[g] = t.indices;
        rows.actions[g] = t.fields.actions.base; rows.old_logp[g] = t.fields.old_logp.base; rows.adv[g] = t.fields.adv.base;
        rows.value_preds[g] = t.fields.value_preds.base; rows.returns[g] = t.fields.returns.base;
        rows.dmu[g] = t.dmu; rows.dvalue[g] = t.dvalue; rows.row_logp[g] = t.row_logp;
        const uintptr_t bases = reinterpret_cast<uintptr_t>(t.mu) | reinterpret_cast<uintptr_t>(t.fields.actions.base) |
                                reinterpret_cast<uintptr_t>(t.fields.old_logp.base) | reinterpret_cast<uintptr_t>(t.dmu);
        if ((A % 4) == 0 && ((t.fields.actions.pitch | t.fields.old_logp.pitch) % 4) == 0 && (bases & 15) == 0) rows.vec |= 1u << g;
        fin.std[g] = t.std; fin.out[g] = t.out; fin.dstd[g] = t.dstd;
        any_grads = any_grads || t.dmu != nullptr;
    }
    const dim3 block(kMlThreads);
    const bool masked = policy_masks || value_masks;
    hipLaunchKernelGGL(marl_loss_group_first_kernel, masked ? dim3((unsigned)p.mask_blocks, (unsigned)groups) : dim3(1), block, 0, s, first);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(marl_loss_group_rows_kernel, dim3((unsigned)p.blocks, (unsigned)groups), block, 0, s, rows);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    const unsigned column_blocks = any_grads ? (unsigned)((A + 3) / 4) : 0u;
    hipLaunchKernelGGL(marl_loss_group_finish_kernel, dim3(column_blocks + 1, (unsigned)groups), block, 0, s, fin);
    return hipGetLastError();
}

}  // namespace mms
