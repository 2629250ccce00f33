// maddpg_kernels.hip -- MADDPG's no-gradient tails for gfx950, every agent's network per launch.
//
//   det_heads_act_kernel         the last layer of up to MMS_MAX_GROUPS deterministic actors (MLPActLayer.forward after the last hidden
//                                activation, agents/algorithms/marl/maddpg/module.py:36-46), the exploration noise of
//                                MADDPG_policy.act (:165-175) and the stores: each agent's action to its own destination (a replay
//                                ring row) AND to its columns of the joint action row -- torch's Linear, tanh, scale, randn, add,
//                                clamp per agent, the cat of N tensors and N copies into N buffers in one launch.  With one group it
//                                is also mms_det_heads_act, the head of DDPG's / TD3's actor (rl/ddpg/module.py MLPActor): the same
//                                block body, so the same bits, plus two things only that entry asks for -- tanh(pre) stored for the
//                                backward (det_head_kernels.hip) and TD3's clipped smoothing noise (td3.py:361-367; det_head_lane.h)
//   q_heads_backup_group_kernel  q_kernels.hip's q_heads_backup_kernel<1> with one critic per group (cal_value_loss, :218-219)
//
// The head's matrix phase is sac_kernels.hip's as separate code: the group on blockIdx.y, a block owns 16 rows, its WAVES waves split
// K = H and each accumulates the NCT = ceil(A / 16) column tiles with v_mfma_f32_16x16x4_f32 (exact fp32 products and sums).  Operand
// lane map: lane l supplies A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15]; a lane loads 4 consecutive k of its row as one float4
// and feeds four MFMAs from it.  The weights are read where torch keeps them ([A, H] row-major): the optimizer and the polyak update
// rewrite them between calls.  The activations are read once: 16-byte non-temporal loads.  The partial sums meet in LDS in wave
// order, so the order of the sum is a function of H and A alone (WAVES is chosen from them): a row's sigma = 0 result depends on that
// row and its network's parameters, not on M, groups, agent0, the pitches or where the row sits.  No atomics.
//
// The draw counter is per ROW and shared by the groups, which are different blocks: no block may write counters[i] while another
// still reads it.  The head kernel therefore only reads the counters, and det_counters_bump_kernel, enqueued behind it on the same
// stream by the same entry, adds the 1.  Both are plain launches: a captured graph replays them in order and draws fresh noise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "det_head_lane.h"
#include "maddpg_args.h"
#include "maddpg_lane.h"
#include "mms_lane.h"
#include "q_lane.h"

namespace mms {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 ldx_nt(const float* p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

// Rows past M and columns past A are computed from clamped (valid) addresses and never stored.  s_part: LDS, WAVES x 16 rows x
// NCT * 16 floats.
template <int NCT, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) det_heads_act_kernel(DetHeadsArgs a) {
    constexpr int RW = NCT * 16;                                  // LDS row width
    constexpr int UB = NCT <= 4 ? 4 : 2;                          // float4 operand groups loaded ahead of their MFMAs
    extern __shared__ __attribute__((aligned(16))) float s_part[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int grp = (int)blockIdx.y;
    const int H = a.H, A = a.A;
    const int64_t M = a.M, r0 = (int64_t)blockIdx.x * 16;
    {
        const float* hrow = a.h[grp] + (r0 + i < M ? r0 + i : M - 1) * (int64_t)H + 4 * q;
        const float* wg = a.w[grp];
        const float* wrow[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) {
            const int j = ct * 16 + i;
            wrow[ct] = wg + (int64_t)(j < A ? j : A - 1) * H + 4 * q;
        }
        f32x4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kq = H / WAVES;                                 // a multiple of 64 (the launcher's choice of WAVES)
        const int kbeg = wave * kq;
        for (int kc = kbeg; kc < kbeg + kq; kc += 64) {
#pragma unroll
            for (int u0 = 0; u0 < 4; u0 += UB) {
                float4 x[UB], b[UB][NCT];
#pragma unroll
                for (int u = 0; u < UB; u++) {
                    x[u] = ldx_nt(hrow + kc + 16 * (u0 + u));
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) b[u][ct] = *reinterpret_cast<const float4*>(wrow[ct] + kc + 16 * (u0 + u));
                }
#pragma unroll
                for (int u = 0; u < UB; u++) {
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[u].x, b[u][ct].x, acc[ct], 0, 0, 0);
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[u].y, b[u][ct].y, acc[ct], 0, 0, 0);
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[u].z, b[u][ct].z, acc[ct], 0, 0, 0);
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[u].w, b[u][ct].w, acc[ct], 0, 0, 0);
                }
            }
        }
        // C/D map: col = lane & 15, row = 4 (lane >> 4) + reg
        float* mine = s_part + (size_t)wave * 16 * RW;
#pragma unroll
        for (int ct = 0; ct < NCT; ct++)
#pragma unroll
            for (int r = 0; r < 4; r++) mine[(4 * q + r) * RW + ct * 16 + i] = acc[ct][r];
    }
    __syncthreads();
    // one element per thread and pass: the partials in wave order, bias, tanh, noise, clamp, stores
    const float* bg = a.b[grp];
    const float limit = a.act_limit[grp];
    float* out = a.act_out[grp];
    const int64_t jcol0 = (int64_t)(a.agent0 + grp) * A;
    for (int e = tid; e < 16 * RW; e += 64 * WAVES) {
        const int r = e / RW, k = e % RW;
        const int64_t row = r0 + r;
        if (row >= M || k >= A) continue;
        float sum = s_part[e];
#pragma unroll
        for (int w = 1; w < WAVES; w++) sum += s_part[w * 16 * RW + e];
        const float pre = sum + bg[k];
        float act = det_action(pre, limit);
        if (a.tanh_out) a.tanh_out[row * A + k] = tanhf(pre);      // (one network: mms_det_heads_act) the backward's t, before any noise
        if (a.sigma > 0.f) {
            const uint64_t rg = (uint64_t)(a.row_offset + row), cnt = (uint64_t)a.counters[row];
            act = a.noise_clip >= 0.f ? det_smooth(act, a.sigma, a.noise_clip, a.seed, rg, cnt, (uint32_t)(jcol0 + k), limit)
                                      : det_explore(act, a.sigma, a.seed, rg, cnt, (uint32_t)(jcol0 + k), limit);
        }
        if (out) out[row * a.act_pitch + k] = act;
        if (a.joint_out) a.joint_out[row * a.joint_pitch + jcol0 + k] = act;
    }
}

__global__ void __launch_bounds__(256) det_counters_bump_kernel(int64_t* __restrict__ counters, int64_t M) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < M) counters[i] += 1;
}

hipError_t launch_det_heads_act(const DetHeadsArgs& a, int groups, hipStream_t s) {
    if (a.M == 0) return hipSuccess;
    const int nct = (a.A + 15) / 16;
    int waves = (a.H % 512 == 0) ? 8 : (a.H % 256 == 0) ? 4 : (a.H % 128 == 0) ? 2 : 1;            // H / waves is a multiple of 64
    while (waves > 1 && (size_t)waves * 16 * nct * 16 * sizeof(float) > 64 * 1024) waves /= 2;     // the partials stay within 64 KB of LDS
    const size_t lds = (size_t)waves * 16 * nct * 16 * sizeof(float);
    const int64_t blocks = (a.M + 15) / 16;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)groups);
#define MMS_DET_W(NCT, W) hipLaunchKernelGGL((det_heads_act_kernel<NCT, W>), grid, dim3(64 * W), lds, s, a)
#define MMS_DET(NCT)                                \
    case NCT:                                       \
        if (waves == 8) MMS_DET_W(NCT, 8);          \
        else if (waves == 4) MMS_DET_W(NCT, 4);     \
        else if (waves == 2) MMS_DET_W(NCT, 2);     \
        else MMS_DET_W(NCT, 1);                     \
        break;
    switch (nct) {
        MMS_DET(1) MMS_DET(2) MMS_DET(3) MMS_DET(4) MMS_DET(5) MMS_DET(6) MMS_DET(7) MMS_DET(8)
        default: return hipErrorInvalidValue;
    }
#undef MMS_DET
#undef MMS_DET_W
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || !(a.sigma > 0.f)) return err;
    const int64_t bump = (a.M + 255) / 256;
    if (bump > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(det_counters_bump_kernel, dim3((unsigned)bump), dim3(256), 0, s, a.counters, a.M);
    return hipGetLastError();
}

// ---- the grouped Q tail: q_heads_backup_kernel<1> (q_kernels.hip) with the group on blockIdx.y -------------------------------------
// Same lane roles and the same order of the sum: a row belongs to the 16 lanes of a quarter wave, lane s reads the float4 at
// k = 64 j + 4 s and keeps one fmaf chain, the 16 partials meet in an xor butterfly (8, 4, 2, 1).  Per group the results are the
// ungrouped kernel's bits for that network alone.
constexpr int kQgThreads = 256;
constexpr int kQgRows = kQgThreads / 16;
constexpr int kQgUnroll = 4;

__global__ void __launch_bounds__(kQgThreads) q_heads_backup_group_kernel(QGroupArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];            // [H]
    const int tid = (int)threadIdx.x, sub = tid & 15;
    const int grp = (int)blockIdx.y;
    const int H = a.H, nj = H / 64;
    {
        const float4* src = reinterpret_cast<const float4*>(a.w[grp]);
        float4* dst = reinterpret_cast<float4*>(s_w);
        for (int i = tid; i < H / 4; i += kQgThreads) dst[i] = src[i];
    }
    const float* wsrc = s_w + 4 * sub;
    __syncthreads();
    const float bias = a.b[grp][0];
    const float* hg = a.h[grp];
    float* q_out = a.q_out[grp];
    float* backup = a.backup[grp];

    for (int it = 0; it < a.iters; it++) {
        const int64_t row = ((int64_t)blockIdx.x * a.iters + it) * kQgRows + (tid >> 4);
        const bool live = row < a.M;                                        // rows past M are neither read nor written
        float acc = 0.f;
        if (live) {
            const float* hrow = hg + row * (int64_t)H + 4 * sub;
            int j = 0;
            for (; j + kQgUnroll <= nj; j += kQgUnroll) {
                float4 x[kQgUnroll];
#pragma unroll
                for (int u = 0; u < kQgUnroll; u++) x[u] = ldx_nt(hrow + 64 * (j + u));
#pragma unroll
                for (int u = 0; u < kQgUnroll; u++) {
                    const float4 w = *reinterpret_cast<const float4*>(wsrc + 64 * (j + u));
                    acc = fmaf(x[u].x, w.x, acc);
                    acc = fmaf(x[u].y, w.y, acc);
                    acc = fmaf(x[u].z, w.z, acc);
                    acc = fmaf(x[u].w, w.w, acc);
                }
            }
            for (; j < nj; j++) {
                const float4 x = ldx_nt(hrow + 64 * j);
                const float4 w = *reinterpret_cast<const float4*>(wsrc + 64 * j);
                acc = fmaf(x.x, w.x, acc);
                acc = fmaf(x.y, w.y, acc);
                acc = fmaf(x.z, w.z, acc);
                acc = fmaf(x.w, w.w, acc);
            }
        }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
        if (live && sub == 0) {
            const float q = q_value(acc, bias);
            if (q_out) q_out[row] = q;
            if (backup) backup[row] = q_backup(a.reward[grp][row], a.done[grp][row], q, false, 0.f, a.gamma, 0.f);
        }
    }
}

hipError_t launch_q_heads_backup_group(const QGroupArgs& args, int groups, hipStream_t s) {
    if (args.M == 0) return hipSuccess;
    if (args.H > MMS_Q_MAX_H) return hipErrorInvalidValue;     // (the entry's check refuses it with a message)
    QGroupArgs a = args;
    // about 1024 blocks over all groups where M allows (the ungrouped launcher's rule); the result does not depend on this choice
    const int64_t rgroups = (a.M + kQgRows - 1) / kQgRows;
    int64_t iters = (rgroups * groups + 1023) / 1024;
    iters = iters < 1 ? 1 : iters > 8 ? 8 : iters;
    a.iters = (int)iters;
    const int64_t blocks = (rgroups + iters - 1) / iters;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)groups), block(kQgThreads);
    hipLaunchKernelGGL(q_heads_backup_group_kernel, grid, block, (size_t)a.H * sizeof(float), s, a);
    return hipGetLastError();
}

}  // namespace mms
