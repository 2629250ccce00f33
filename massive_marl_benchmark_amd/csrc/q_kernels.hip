// q_kernels.hip -- the off-policy Q target's tail for gfx950.
//
//   q_heads_backup_kernel  the last layer of one or two critics (MLPQFunction's Linear(H, 1), rl/{ddpg,td3,sac}/module.py), the min
//                          of the two and the Bellman backup r + gamma (1 - d) (min q - alpha logp) (sac.py:379-382,
//                          td3.py:370-373, ddpg.py:368-369): two [M,H] x [H,1] products and five element-wise launches in one
//
// A streaming reduction: 4 G M H bytes in, a few bytes per row out, so HBM bandwidth is the bound.  Lane roles: a row belongs to
// the 16 lanes of a quarter wave.  Lane s of the quarter reads the float4 at k = 64 j + 4 s for j = 0 .. H / 64 - 1 (the quarter
// reads 256 contiguous bytes of its row per load, the wave four such rows) and keeps ONE fmaf chain per network over its elements in
// that order; the 16 partial sums meet in an xor butterfly (8, 4, 2, 1), which leaves the same bits in every lane of the quarter.
// The order of the sum is therefore a function of H alone: q[i] depends on row i and the weights, not on M, the grid or where the row
// sits in the call.  No atomics anywhere.  The weights (read where torch keeps them) are staged into LDS once per block, which then
// walks `iters` groups of 16 rows (H <= MMS_Q_MAX_H = 4096, checked by the entry: at most 32 KB of LDS per block).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mms_lane.h"
#include "q_lane.h"

namespace mms {

constexpr int kQThreads = 256;                  // 4 waves: 16 rows per pass
constexpr int kQRows = kQThreads / 16;
constexpr int kQUnroll = 4;                     // float4 loads per network in flight per lane

struct QArgs {
    const float* h[2]; const float* w[2]; const float* b[2]; float* q_out[2];
    const float* reward; const uint8_t* done; const float* logp; float* backup;
    float gamma, alpha;
    int64_t M;
    int H, iters;
};

// The activations are read once: a non-temporal 16-byte load (G = 2, M = 65536, H = 1024: 78 - 84 us against 88 - 97 us with plain
// loads, profiles/q_heads_tail_ab.jsonl).
__device__ __forceinline__ float4 ldx(const float* p) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

template <int G>
__global__ void __launch_bounds__(kQThreads) q_heads_backup_kernel(QArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];            // [G][H]
    const int tid = (int)threadIdx.x, sub = tid & 15;
    const int H = a.H, nj = H / 64;
    const float* wsrc[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        const float4* src = reinterpret_cast<const float4*>(a.w[g]);
        float4* dst = reinterpret_cast<float4*>(s_w + (size_t)g * H);
        for (int i = tid; i < H / 4; i += kQThreads) dst[i] = src[i];
        wsrc[g] = s_w + (size_t)g * H + 4 * sub;
    }
    __syncthreads();
    float bias[G];
#pragma unroll
    for (int g = 0; g < G; g++) bias[g] = a.b[g][0];

    for (int it = 0; it < a.iters; it++) {
        const int64_t row = ((int64_t)blockIdx.x * a.iters + it) * kQRows + (tid >> 4);
        const bool live = row < a.M;                                        // rows past M are neither read nor written
        float acc[G];
#pragma unroll
        for (int g = 0; g < G; g++) acc[g] = 0.f;
        if (live) {
            const float* hrow[G];
#pragma unroll
            for (int g = 0; g < G; g++) hrow[g] = a.h[g] + row * (int64_t)H + 4 * sub;
            int j = 0;
            for (; j + kQUnroll <= nj; j += kQUnroll) {
                float4 x[G][kQUnroll];
#pragma unroll
                for (int u = 0; u < kQUnroll; u++)
#pragma unroll
                    for (int g = 0; g < G; g++) x[g][u] = ldx(hrow[g] + 64 * (j + u));
#pragma unroll
                for (int u = 0; u < kQUnroll; u++)
#pragma unroll
                    for (int g = 0; g < G; g++) {
                        const float4 w = *reinterpret_cast<const float4*>(wsrc[g] + 64 * (j + u));
                        acc[g] = fmaf(x[g][u].x, w.x, acc[g]);
                        acc[g] = fmaf(x[g][u].y, w.y, acc[g]);
                        acc[g] = fmaf(x[g][u].z, w.z, acc[g]);
                        acc[g] = fmaf(x[g][u].w, w.w, acc[g]);
                    }
            }
            for (; j < nj; j++) {
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const float4 x = ldx(hrow[g] + 64 * j);
                    const float4 w = *reinterpret_cast<const float4*>(wsrc[g] + 64 * j);
                    acc[g] = fmaf(x.x, w.x, acc[g]);
                    acc[g] = fmaf(x.y, w.y, acc[g]);
                    acc[g] = fmaf(x.z, w.z, acc[g]);
                    acc[g] = fmaf(x.w, w.w, acc[g]);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < G; g++)
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) acc[g] += __shfl_xor(acc[g], m, 64);
        if (live && sub == 0) {
            float q[G];
#pragma unroll
            for (int g = 0; g < G; g++) {
                q[g] = q_value(acc[g], bias[g]);
                if (a.q_out[g]) a.q_out[g][row] = q[g];
            }
            if (a.backup) {
                const float qm = G == 2 ? q_min(q[0], q[G - 1]) : q[0];
                a.backup[row] = q_backup(a.reward[row], a.done[row], qm, a.logp != nullptr, a.logp ? a.logp[row] : 0.f, a.gamma, a.alpha);
            }
        }
    }
}

hipError_t launch_q_heads_backup(int G, int64_t M, int H, const float* const* h, const float* const* w, const float* const* b, float* const* q_out,
                                 const float* reward, const uint8_t* done, const float* logp, float gamma, float alpha, float* backup,
                                 hipStream_t s) {
    if (M == 0) return hipSuccess;
    if (H > MMS_Q_MAX_H) return hipErrorInvalidValue;     // (the entry's check refuses it with a message)
    QArgs a = {};
    for (int g = 0; g < G; g++) { a.h[g] = h[g]; a.w[g] = w[g]; a.b[g] = b[g]; a.q_out[g] = q_out[g]; }
    a.reward = reward; a.done = done; a.logp = logp; a.backup = backup;
    a.gamma = gamma; a.alpha = alpha; a.M = M; a.H = H;
    // about 1024 blocks (4 per CU) where M allows, so that the weights are staged once per 16 .. 128 rows and M = 8192 still gives
    // every CU two blocks; the result does not depend on this choice
    const int64_t groups = (M + kQRows - 1) / kQRows;
    int64_t iters = (groups + 1023) / 1024;
    iters = iters < 1 ? 1 : iters > 8 ? 8 : iters;
    a.iters = (int)iters;
    const int64_t blocks = (groups + iters - 1) / iters;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const size_t lds = (size_t)G * H * sizeof(float);
    const dim3 grid((unsigned)blocks), block(kQThreads);
    if (G == 2) hipLaunchKernelGGL((q_heads_backup_kernel<2>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((q_heads_backup_kernel<1>), grid, block, lds, s, a);
    return hipGetLastError();
}

}  // namespace mms
