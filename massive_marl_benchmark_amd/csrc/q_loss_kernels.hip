// q_loss_kernels.hip -- the critics' loss heads WITH a gradient for gfx950 (mms_q_heads_loss, include/mms.h): the last layer of one or
// two critics, the loss (MSE against a target, or the policy loss's min), and the whole backward of that tail in one streaming pass.
//
//   q_heads_loss_kernel   per row: q_g = dot(h_g, w_g) + b_g with q_kernels.hip's lane roles and summation order (the same bits),
//                         d loss / d q_g (q_loss_lane.h), dh_g = dq_g w_g written at once, and dq_g h_g added to the thread's double
//                         column sums; per workgroup one partial of every column, in a fixed order
//   q_heads_loss_finish   the partials of every column added over the workgroups in a fixed order, rounded once
//
// d loss / d q is known the moment q is known (the backward starts from 1), so each [M, H] activation block is read from memory
// ONCE: a row belongs to the 16 lanes of a quarter wave, which keep it in registers (H <= 1024: 64 floats per lane and network) from
// the dot product to the column sums.  Traffic: 4 G M H bytes in, 4 G M H out where dh is wanted: HBM bandwidth is the bound, and
// the double accumulators (H / 16 per lane and network) are paid in registers, not in time.  No atomics, no memset: every workgroup
// writes all of its columns, the finish pass reads exactly those.  Built without fast-math (the Makefile's PARAM_FLAGS): IEEE
// division, no contraction, every statement of q_loss_lane.h rounded as in the CPU build.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mms_lane.h"
#include "q_loss_lane.h"

namespace mms {

constexpr int kQLossThreads = 256;              // 4 waves: kQLossRows rows per pass
static_assert(kQLossThreads / 16 == kQLossRows, "a quarter wave per row");

struct QLossArgs {
    const float* h[2]; const float* w[2]; const float* b[2];
    const float* target; const float* logp;
    float* q_out[2]; float* dh[2];
    float* loss; float* dw[2]; float* db[2];
    double* part;                               // [blocks][q_loss_columns(G, H)]
    float alpha, scale;
    int64_t M, iters, blocks, per_segment;
    int H, mode;
};

// the activations are read once (q_kernels.hip: a non-temporal 16-byte load)
__device__ __forceinline__ float4 ldx_once(const float* p) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

// NJ: an upper bound of H / 64 (1, 2, 4, 8, 16), so that a row's registers are indexed statically
template <int G, int NJ>
__global__ void __launch_bounds__(kQLossThreads) q_heads_loss_kernel(QLossArgs a) {
    extern __shared__ __attribute__((aligned(16))) double s_red[];          // [4][H] doubles: the waves' column sums of one network
    __shared__ double s_slot[kQLossRows][3];                                // db_0, db_1, loss term per row slot
    const int tid = (int)threadIdx.x, sub = tid & 15, slot = tid >> 4;
    const int H = a.H, nj = H / 64;
    float* s_w = reinterpret_cast<float*>(s_red + 4 * (size_t)H);           // [G][H]
#pragma unroll
    for (int g = 0; g < G; g++) {
        const float4* src = reinterpret_cast<const float4*>(a.w[g]);
        float4* dst = reinterpret_cast<float4*>(s_w + (size_t)g * H);
        for (int i = tid; i < H / 4; i += kQLossThreads) dst[i] = src[i];
    }
    __syncthreads();
    float bias[G];
    bool want_dw[G];
#pragma unroll
    for (int g = 0; g < G; g++) { bias[g] = a.b[g][0]; want_dw[g] = a.dw[g] != nullptr; }

    double cw[G][NJ][4];                        // this thread's column sums: columns 64 j + 4 sub + c over its row slot's rows
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
            for (int c = 0; c < 4; c++) cw[g][j][c] = 0.0;
    double cb[G], closs = 0.0;
#pragma unroll
    for (int g = 0; g < G; g++) cb[g] = 0.0;
    const double m_rows = (double)a.M;

    for (int64_t it = 0; it < a.iters; it++) {
        const int64_t row = ((int64_t)blockIdx.x * a.iters + it) * kQLossRows + slot;
        const bool live = row < a.M;            // rows past M are neither read nor written
        float4 x[G][NJ];
        float acc[G];
#pragma unroll
        for (int g = 0; g < G; g++) acc[g] = 0.f;
        if (live) {
#pragma unroll
            for (int j = 0; j < NJ; j++)
#pragma unroll
                for (int g = 0; g < G; g++)
                    if (j < nj) x[g][j] = ldx_once(a.h[g] + row * (int64_t)H + 64 * j + 4 * sub);
#pragma unroll
            for (int j = 0; j < NJ; j++)
#pragma unroll
                for (int g = 0; g < G; g++)
                    if (j < nj) {
                        const float4 w = *reinterpret_cast<const float4*>(s_w + (size_t)g * H + 64 * j + 4 * sub);
                        acc[g] = fmaf(x[g][j].x, w.x, acc[g]);
                        acc[g] = fmaf(x[g][j].y, w.y, acc[g]);
                        acc[g] = fmaf(x[g][j].z, w.z, acc[g]);
                        acc[g] = fmaf(x[g][j].w, w.w, acc[g]);
                    }
        }
#pragma unroll
        for (int g = 0; g < G; g++)
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) acc[g] += __shfl_xor(acc[g], m, 64);
        if (!live) continue;                    // (the shuffles above are the last wave-wide operation of the pass)
        float q[G];
        double dq[G];
#pragma unroll
        for (int g = 0; g < G; g++) q[g] = q_value(acc[g], bias[g]);
        const float target = a.mode == 0 ? a.target[row] : 0.f;
        const float logp = a.logp ? a.logp[row] : 0.f;
        const double term = q_loss_row<G>(a.mode, q, target, a.logp != nullptr, logp, a.alpha, a.scale, m_rows, dq);
        if (sub == 0) {
            closs += term;
#pragma unroll
            for (int g = 0; g < G; g++) {
                if (a.q_out[g]) a.q_out[g][row] = q[g];
                cb[g] += dq[g];
            }
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            if (a.dh[g]) {
                float* out = a.dh[g] + row * (int64_t)H + 4 * sub;
#pragma unroll
                for (int j = 0; j < NJ; j++)
                    if (j < nj) {
                        const float4 w = *reinterpret_cast<const float4*>(s_w + (size_t)g * H + 64 * j + 4 * sub);
                        *reinterpret_cast<float4*>(out + 64 * j) = make_float4(q_loss_dh(a.mode, dq[g], w.x), q_loss_dh(a.mode, dq[g], w.y), q_loss_dh(a.mode, dq[g], w.z), q_loss_dh(a.mode, dq[g], w.w));
                    }
            }
            if (want_dw[g]) {
                const double d = dq[g];
#pragma unroll
                for (int j = 0; j < NJ; j++)
                    if (j < nj) {
                        cw[g][j][0] += d * (double)x[g][j].x;
                        cw[g][j][1] += d * (double)x[g][j].y;
                        cw[g][j][2] += d * (double)x[g][j].z;
                        cw[g][j][3] += d * (double)x[g][j].w;
                    }
            }
        }
    }

    // the workgroup's partial of every column: q_loss_slot_sum's order (the quarters of a wave pairwise, then the waves ascending)
    const int NC = q_loss_columns(G, H);
    double* part = a.part + (int64_t)blockIdx.x * NC;
#pragma unroll
    for (int g = 0; g < G; g++) {
        if (!want_dw[g]) continue;              // uniform over the workgroup
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                double v = cw[g][j][c];
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 32, 64);
                if (j < nj && (tid & 63) < 16) s_red[(size_t)(tid >> 6) * H + 64 * j + 4 * sub + c] = v;
            }
        __syncthreads();
        for (int k = tid; k < H; k += kQLossThreads)
            part[g * (H + 1) + k] = ((s_red[k] + s_red[(size_t)H + k]) + s_red[2 * (size_t)H + k]) + s_red[3 * (size_t)H + k];
        __syncthreads();
    }
    if (sub == 0) {
        s_slot[slot][0] = cb[0];
        s_slot[slot][1] = cb[G - 1];
        s_slot[slot][2] = closs;
    }
    __syncthreads();
    if (tid < 3) {
        double v[kQLossRows];
#pragma unroll
        for (int r = 0; r < kQLossRows; r++) v[r] = s_slot[r][tid];
        const double s = q_loss_slot_sum(v);
        if (tid == 2) part[NC - 1] = s;
        else if (tid < G && want_dw[tid == 0 ? 0 : G - 1]) part[tid * (H + 1) + H] = s;
    }
}

// One thread per (column, segment): 16 columns x kQLossSegments segments a workgroup, the segments met through LDS in ascending order.
__global__ void __launch_bounds__(256) q_heads_loss_finish(QLossArgs a, int G) {
    __shared__ double s_seg[kQLossSegments][16];
    const int tid = (int)threadIdx.x, lane = tid & 15, seg = tid >> 4;
    const int H = a.H, NC = q_loss_columns(G, H);
    const int col = (int)blockIdx.x * 16 + lane;
    float* dst = nullptr;                       // where the column goes; NULL: not computed (its partials were not written)
    if (col == NC - 1) dst = a.loss;
    else if (col < NC - 1) {
        const int g = col / (H + 1), k = col % (H + 1);
        if (a.dw[g]) dst = k < H ? a.dw[g] + k : a.db[g];
    }
    double s = 0.0;
    if (dst) {
        const int64_t first = (int64_t)seg * a.per_segment;
        int64_t last = first + a.per_segment;
        last = last < a.blocks ? last : a.blocks;
        s = q_loss_segment_sum(a.part + col, NC, first, last);
    }
    s_seg[seg][lane] = s;
    __syncthreads();
    if (seg == 0 && dst) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < kQLossSegments; i++) t += s_seg[i][lane];
        *dst = col == NC - 1 ? (float)(t / (double)a.M) : (float)t;
    }
}

int64_t q_loss_ws_bytes(int64_t M, int H, int G) {
    const QLossPartition p = q_loss_partition(M, H);
    return (p.blocks * q_loss_columns(G, H) * (int64_t)sizeof(double) + 255) / 256 * 256;
}

template <int G>
static void launch_main(int H, dim3 grid, size_t lds, hipStream_t s, const QLossArgs& a) {
    const int nj = H / 64;
    if (nj <= 1) hipLaunchKernelGGL((q_heads_loss_kernel<G, 1>), grid, dim3(kQLossThreads), lds, s, a);
    else if (nj <= 2) hipLaunchKernelGGL((q_heads_loss_kernel<G, 2>), grid, dim3(kQLossThreads), lds, s, a);
    else if (nj <= 4) hipLaunchKernelGGL((q_heads_loss_kernel<G, 4>), grid, dim3(kQLossThreads), lds, s, a);
    else if (nj <= 8) hipLaunchKernelGGL((q_heads_loss_kernel<G, 8>), grid, dim3(kQLossThreads), lds, s, a);
    else hipLaunchKernelGGL((q_heads_loss_kernel<G, 16>), grid, dim3(kQLossThreads), lds, s, a);
}

// the launches of a checked call (mms_host.h: check_q_heads_loss): 1 <= M <= 0x7fffffff, H a multiple of 64 up to MMS_Q_LOSS_MAX_H
hipError_t launch_q_heads_loss(int G, int64_t M, int H, const float* const* h, const float* const* w, const float* const* b, int mode,
                               const float* target, const float* logp, float alpha, float scale, float* loss, float* const* q_out,
                               float* const* dh, float* const* dw, float* const* db, void* workspace, hipStream_t s) {
    if (M < 1 || H > MMS_Q_LOSS_MAX_H) return hipErrorInvalidValue;          // (the entry's check refuses both with a message)
    const QLossPartition p = q_loss_partition(M, H);
    if (p.blocks > 0x7fffffff) return hipErrorInvalidValue;
    QLossArgs a = {};
    for (int g = 0; g < G; g++) {
        a.h[g] = h[g]; a.w[g] = w[g]; a.b[g] = b[g]; a.q_out[g] = q_out[g]; a.dh[g] = dh[g];
        a.dw[g] = dw[g] && db[g] ? dw[g] : nullptr; a.db[g] = a.dw[g] ? db[g] : nullptr;
    }
    a.target = target; a.logp = mode == 1 ? logp : nullptr; a.loss = loss;
    a.part = static_cast<double*>(workspace);
    a.alpha = alpha; a.scale = scale; a.M = M; a.iters = p.iters; a.blocks = p.blocks; a.per_segment = p.per_segment;
    a.H = H; a.mode = mode;
    const size_t lds = 4 * (size_t)H * sizeof(double) + (size_t)G * H * sizeof(float);
    const dim3 grid((unsigned)p.blocks);
    if (G == 2) launch_main<2>(H, grid, lds, s, a);
    else launch_main<1>(H, grid, lds, s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const int NC = q_loss_columns(G, H);
    hipLaunchKernelGGL(q_heads_loss_finish, dim3((unsigned)((NC + 15) / 16)), dim3(256), 0, s, a, G);
    return hipGetLastError();
}

}  // namespace mms
