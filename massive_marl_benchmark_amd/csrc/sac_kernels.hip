// sac_kernels.hip -- SAC's squashed-Gaussian policy head for gfx950.
//
//   sac_head_act_kernel  SquashedGaussianMLPActor.forward after `net` (agents/algorithms/rl/sac/module.py:31-61): mu_layer and
//                        log_std_layer on the matrix cores, the clamp of log_std, the rsample from the counter-based stream, the
//                        tanh-corrected log-probability and the scaled action -- torch's chain of about a dozen launches in one
//
// The matrix phase follows the PPO head (head_block.h: ppo_head_block) as separate code: a block owns 16 rows, its WAVES waves split
// K = H, and each accumulates all NCT column tiles -- the ceil(A / 16) tiles of mu_layer, then as many of log_std_layer -- with
// v_mfma_f32_16x16x4_f32 (exact fp32 products and sums).  Operand lane map: lane l supplies A[l & 15][k = l >> 4] and
// B[k = l >> 4][l & 15]; a lane loads 4 consecutive k of its row as one float4 and feeds four MFMAs from it.  Both weight matrices
// are read where torch keeps them ([A, H] row-major): SAC writes them on every env step (optimizer step, polyak .data write), so a
// derived copy would need a refresh.  The partial sums meet in LDS in wave order (deterministic), then one wave per row samples.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mms_lane.h"
#include "sac_lane.h"

namespace mms {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct SacOut {
    float* actions_out; float* act_slot; float* logp_slot; float* u_slot; float* mu_slot; float* log_std_slot;
};

// NCT = 2 ceil(A / 16) column tiles (compile time: the accumulators must be plain registers).  Rows past N and columns past A are
// computed from clamped (valid) addresses and never read back.  s_part: LDS, WAVES x 16 rows x NCT * 16 floats; wave 0's slice
// receives the sums (every element is read and written by the same thread).
template <int NCT, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) sac_head_act_kernel(const float* __restrict__ hidden, int H, const float* __restrict__ mu_w,
                                                                  const float* __restrict__ mu_b, const float* __restrict__ ls_w,
                                                                  const float* __restrict__ ls_b, float act_limit, float epsilon,
                                                                  int deterministic, uint64_t seed, int64_t* __restrict__ counters,
                                                                  int64_t row_offset, SacOut o, int64_t N, int A) {
    constexpr int HT = NCT / 2, AP = HT * 16, RW = NCT * 16;     // tiles per head, padded head width, LDS row width (mu | log_std)
    constexpr int UB = NCT <= 8 ? 4 : 2;                          // float4 operand groups loaded ahead of their MFMAs (<= 32 float4 live)
    constexpr int RPW = 16 / WAVES;                               // rows sampled per wave
    extern __shared__ __attribute__((aligned(16))) float s_part[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * 16;
    {
        const float* hrow = hidden + (r0 + i < N ? r0 + i : N - 1) * (int64_t)H + 4 * g;
        const float* wrow[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) {
            const int j = (ct % HT) * 16 + i;
            wrow[ct] = (ct < HT ? mu_w : ls_w) + (int64_t)(j < A ? j : A - 1) * H + 4 * g;
        }
        f32x4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kq = H / WAVES;                                 // a multiple of 64 (the launcher's choice of WAVES)
        const int kbeg = wave * kq;
        for (int kc = kbeg; kc < kbeg + kq; kc += 64) {
#pragma unroll
            for (int u0 = 0; u0 < 4; u0 += UB) {
                float4 a[UB], b[UB][NCT];
#pragma unroll
                for (int u = 0; u < UB; u++) {
                    a[u] = *reinterpret_cast<const float4*>(hrow + kc + 16 * (u0 + u));
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) b[u][ct] = *reinterpret_cast<const float4*>(wrow[ct] + kc + 16 * (u0 + u));
                }
#pragma unroll
                for (int u = 0; u < UB; u++) {
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, b[u][ct].x, acc[ct], 0, 0, 0);
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, b[u][ct].y, acc[ct], 0, 0, 0);
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, b[u][ct].z, acc[ct], 0, 0, 0);
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, b[u][ct].w, acc[ct], 0, 0, 0);
                }
            }
        }
        // C/D map: col = lane & 15, row = 4 (lane >> 4) + reg
        float* mine = s_part + (size_t)wave * 16 * RW;
#pragma unroll
        for (int ct = 0; ct < NCT; ct++)
#pragma unroll
            for (int r = 0; r < 4; r++) mine[(4 * g + r) * RW + ct * 16 + i] = acc[ct][r];
    }
    __syncthreads();
    for (int e = tid; e < 16 * RW; e += 64 * WAVES) {
        const int col = e % RW;
        const int j = col % AP;
        float sum = s_part[e];
#pragma unroll
        for (int w = 1; w < WAVES; w++) sum += s_part[w * 16 * RW + e];    // wave order
        s_part[e] = sum + (col < AP ? mu_b : ls_b)[j < A ? j : 0];
    }
    __syncthreads();
    // sampling: one wave per row, lane j handles actions j and j + 64; the row's log-probability is a wave reduction.  The draw
    // counter lives in device memory so that a replayed hipGraph draws fresh noise; the store of c + 1 depends on the load of c.
    const bool want_logp = o.logp_slot != nullptr;
#pragma unroll
    for (int q = 0; q < RPW; q++) {
        const int r = wave * RPW + q;
        const int64_t row = r0 + r;
        if (row >= N) continue;
        const float* srow = s_part + r * RW;
        const int64_t c = deterministic ? 0 : counters[row];
        float lp = 0.f;
        for (int j = lane; j < A; j += 64) {
            float u, ls, term;
            const float act = sac_sample_one(srow[j], srow[AP + j], deterministic, seed, (uint64_t)(row_offset + row), (uint64_t)c, (uint32_t)j,
                                             act_limit, epsilon, want_logp, u, ls, term);
            lp += term;
            const int64_t at = row * A + j;
            if (o.actions_out) o.actions_out[at] = act;
            if (o.act_slot) o.act_slot[at] = act;
            if (o.u_slot) o.u_slot[at] = u;
            if (o.mu_slot) o.mu_slot[at] = srow[j];
            if (o.log_std_slot) o.log_std_slot[at] = ls;
        }
        if (want_logp) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) lp += __shfl_xor(lp, m, 64);
        }
        if (lane == 0) {
            if (want_logp) o.logp_slot[row] = lp;
            if (!deterministic) counters[row] = c + 1;
        }
    }
}

hipError_t launch_sac_head_act(const float* hidden, int H, const float* mu_w, const float* mu_b, const float* ls_w, const float* ls_b,
                               float act_limit, float epsilon, int deterministic, uint64_t seed, int64_t* counters, int64_t row_offset,
                               float* actions_out, float* act_slot, float* logp_slot, float* u_slot, float* mu_slot, float* log_std_slot,
                               int64_t N, int A, hipStream_t s) {
    if (N == 0) return hipSuccess;
    const SacOut o{actions_out, act_slot, logp_slot, u_slot, mu_slot, log_std_slot};
    const int nct = 2 * ((A + 15) / 16);
    int waves = (H % 512 == 0) ? 8 : (H % 256 == 0) ? 4 : (H % 128 == 0) ? 2 : 1;            // H / waves is a multiple of 64
    while (waves > 1 && (size_t)waves * 16 * nct * 16 * sizeof(float) > 64 * 1024) waves /= 2;  // the partials stay within 64 KB of LDS
    const size_t lds = (size_t)waves * 16 * nct * 16 * sizeof(float);
    const dim3 grid((unsigned)((N + 15) / 16));
#define MMS_SAC_W(NCT, W)                                                                                                                  \
    hipLaunchKernelGGL((sac_head_act_kernel<NCT, W>), grid, dim3(64 * W), lds, s, hidden, H, mu_w, mu_b, ls_w, ls_b, act_limit, epsilon, \
                       deterministic, seed, counters, row_offset, o, N, A)
#define MMS_SAC(NCT)                                \
    case NCT:                                       \
        if (waves == 8) MMS_SAC_W(NCT, 8);          \
        else if (waves == 4) MMS_SAC_W(NCT, 4);     \
        else if (waves == 2) MMS_SAC_W(NCT, 2);     \
        else MMS_SAC_W(NCT, 1);                     \
        break;
    switch (nct) {
        MMS_SAC(2) MMS_SAC(4) MMS_SAC(6) MMS_SAC(8) MMS_SAC(10) MMS_SAC(12) MMS_SAC(14) MMS_SAC(16)
        default: return hipErrorInvalidValue;
    }
#undef MMS_SAC
#undef MMS_SAC_W
    return hipGetLastError();
}

}  // namespace mms
