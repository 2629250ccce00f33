// sac_grad_kernels.hip -- the backward of SAC's squashed-Gaussian head epilogue for gfx950 (mms_sac_heads_grad, include/mms.h):
//   sac_grad_rows_kernel    dy [N, 2A] = (dmu | dlog_std) from the forward's saved u, mu, log_std and the incoming gradients
//                           (sac_grad_lane.h); per workgroup the 2A column sums of its rows, in double
//   sac_grad_finish_kernel  one wave per column adds the workgroups' partials in a fixed order and rounds once: dbias [2A]
// A streaming pass: 16 A + 4 bytes in and 8 A bytes out per row.  The inputs are [N,A] and dy is [N,2A], so a flat 16-byte access of
// the inputs does not map to one of dy unless A is a multiple of 4.  A workgroup therefore owns TILES of R whole rows
// (R = sac_grad_tile_rows(A): a multiple of 4 with R A <= 1024, so every tile of a 16-byte aligned array starts 16-byte aligned):
// thread t loads elements 4 t .. 4 t + 3 of the tile from each input as one float4 (whatever A is; the elements past the last row's
// end one by one), writes its results to the tile's dy image in LDS, and the image leaves as flat float4 stores.  With a base that is
// not 16-byte aligned every access is scalar; the arithmetic and every sum's order are the same.
// Tiles go to workgroups round robin (tile, tile + grid, ..; grid = min(tiles, 1024)): the number of partial rows is bounded.
// Order of the column sums.  The 256 threads form P = 256 / (2A) row groups of 2A columns; thread (p, c) adds dy[r][c] of the LDS image
// for r = p, p + P, .. of each of its workgroup's tiles in tile order, in double; the P partials of a column are added in ascending
// p; block b stores its 2A doubles at part[b 2A + c]; the finish pass gives a column a wave: lane t adds the partials of blocks t,
// t + 64, .. in ascending order, then an xor butterfly (32 .. 1); one rounding to fp32.  No atomics, no memset: every word
// of the workspace that the finish pass reads was written by the row pass of the same call.
// Built like param_step_kernels.hip (csrc/Makefile: PARAM_FLAGS): no fast-math, -ffp-contract=off, so the vector and the scalar
// path, and the CPU build's evaluation of sac_grad_lane.h, round every operation alike.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sac_grad_lane.h"

namespace mms {

constexpr int kSgThreads = 256;
constexpr int kSgMaxBlocks = 1024;              // 4 per CU: rows of partials the finish pass adds per column
constexpr int kSgMaxA = 128;

struct SacGradArgs {
    const float *u, *mu, *log_std, *grad_action, *grad_logp;
    float* dy;
    float* dbias;
    double* part;
    int64_t N, tiles;
    int A, R, blocks;
    float act_limit, epsilon;
};

struct SacGradPlan { int R, blocks; int64_t tiles, bytes; };

static SacGradPlan sac_grad_plan(int64_t N, int A) {
    SacGradPlan p;
    p.R = sac_grad_tile_rows(A);
    p.tiles = (N + p.R - 1) / p.R;
    p.blocks = (int)(p.tiles < kSgMaxBlocks ? p.tiles : kSgMaxBlocks);
    p.bytes = (((int64_t)p.blocks * 2 * A * (int64_t)sizeof(double)) + 255) & ~(int64_t)255;
    return p;
}

int64_t sac_grad_ws_bytes(int64_t N, int A) { return sac_grad_plan(N, A).bytes; }

// elements k0 .. k0 + 3 of a tile of cnt elements (past cnt: 0); tile is 16-byte aligned when VEC
template <bool VEC>
__device__ __forceinline__ void sg_load4(const float* tile, int k0, int cnt, float (&x)[4]) {
    if (VEC && k0 + 3 < cnt) {
        const float4 v = *reinterpret_cast<const float4*>(tile + k0);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = (k0 + k < cnt) ? tile[k0 + k] : 0.f;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(kSgThreads) sac_grad_rows_kernel(SacGradArgs a) {
    __shared__ __align__(16) float s_dy[2 * kSacGradTile];     // the tile's rows of dy
    __shared__ float s_gl[kSacGradTile];                        // grad_logp of the tile's rows (R <= 1024: A = 1)
    __shared__ double s_col[kSgThreads];
    const int tid = (int)threadIdx.x, A = a.A, C = 2 * A, R = a.R;
    const int P = kSgThreads / C, p = tid / C, c = tid - p * C;
    const bool sums = a.part != nullptr && p < P;
    const int k0 = 4 * tid;
    double acc = 0.0;

    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t row0 = tile * R;
        const int rows = (a.N - row0 < R) ? (int)(a.N - row0) : R;              // rows past N are neither read nor written
        const int cnt = rows * A;
        const int64_t e0 = row0 * A;
        for (int r = tid; r < rows; r += kSgThreads) s_gl[r] = a.grad_logp ? a.grad_logp[row0 + r] : 0.f;
        float xu[4], xm[4], xl[4], xg[4] = {0.f, 0.f, 0.f, 0.f};
        sg_load4<VEC>(a.u + e0, k0, cnt, xu);
        sg_load4<VEC>(a.mu + e0, k0, cnt, xm);
        sg_load4<VEC>(a.log_std + e0, k0, cnt, xl);
        if (a.grad_action) sg_load4<VEC>(a.grad_action + e0, k0, cnt, xg);
        __syncthreads();
        if (k0 < cnt) {
            int r = k0 / A, j = k0 - r * A;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (k0 + k < cnt) {
                    float dmu, dls;
                    sac_grad_one(xu[k], xm[k], xl[k], xg[k], s_gl[r], a.act_limit, a.epsilon, dmu, dls);
                    s_dy[r * C + j] = dmu;
                    s_dy[r * C + A + j] = dls;
                    if (++j == A) { j = 0; r++; }
                }
            }
        }
        __syncthreads();
        const int out = rows * C;                                                // <= 2 kSacGradTile
        float* dst = a.dy + row0 * C;
        const int nvec = VEC ? out >> 2 : 0;
        for (int i = tid; i < nvec; i += kSgThreads) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(s_dy)[i];
        for (int i = 4 * nvec + tid; i < out; i += kSgThreads) dst[i] = s_dy[i];
        if (sums)
            for (int r = p; r < rows; r += P) acc += (double)s_dy[r * C + c];
        __syncthreads();                                                         // the next tile rewrites s_dy and s_gl
    }

    if (a.part == nullptr) return;
    s_col[tid] = acc;
    __syncthreads();
    if (tid < C) {
        double s = s_col[tid];
        for (int q = 1; q < P; q++) s += s_col[q * C + tid];
        a.part[(int64_t)blockIdx.x * C + tid] = s;
    }
}

// A wave per column (four columns per workgroup): lane t adds the partials of blocks t, t + 64, .. in ascending order (at most 16,
// every load in flight at once; a slot past `blocks` adds 0.0, which changes nothing), then the xor butterfly 32 .. 1; one rounding.
// (One THREAD per column walking all 1024 partials took 41 us at SAC's shapes, four times the row pass: a chain of load latencies.)
__global__ void __launch_bounds__(kSgThreads) sac_grad_finish_kernel(SacGradArgs a) {
    const int C = 2 * a.A, lane = (int)threadIdx.x & 63;
    const int col = (int)blockIdx.x * (kSgThreads / 64) + ((int)threadIdx.x >> 6);
    if (col >= C) return;                                            // (wave-uniform)
    const double* p = a.part + col;
    double v[kSgMaxBlocks / 64];
#pragma unroll
    for (int k = 0; k < kSgMaxBlocks / 64; k++) {
        const int b = 64 * k + lane;
        v[k] = b < a.blocks ? p[(int64_t)b * C] : 0.0;
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kSgMaxBlocks / 64; k++) s += v[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) a.dbias[col] = (float)s;
}

// the launches of a checked call (mms_host.h: check_sac_heads_grad); N >= 1
hipError_t launch_sac_heads_grad(int64_t N, int A, float act_limit, float epsilon, const float* u, const float* mu, const float* log_std,
                                 const float* grad_action, const float* grad_logp, float* dy, float* dbias, void* workspace, hipStream_t s) {
    if (N < 1 || N > 0x7fffffff || A < 1 || A > kSgMaxA) return hipErrorInvalidValue;      // (the entry's check refuses it with a message)
    const SacGradPlan p = sac_grad_plan(N, A);
    SacGradArgs a = {};
    a.u = u; a.mu = mu; a.log_std = log_std; a.grad_action = grad_action; a.grad_logp = grad_logp;
    a.dy = dy; a.dbias = dbias;
    a.part = dbias ? static_cast<double*>(workspace) : nullptr;
    a.N = N; a.tiles = p.tiles; a.A = A; a.R = p.R; a.blocks = p.blocks;
    a.act_limit = act_limit; a.epsilon = epsilon;
    const uintptr_t bases = reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(mu) | reinterpret_cast<uintptr_t>(log_std) |
                            reinterpret_cast<uintptr_t>(grad_action) | reinterpret_cast<uintptr_t>(dy);
    const dim3 grid((unsigned)p.blocks), block(kSgThreads);
    if ((bases & 15) == 0) hipLaunchKernelGGL((sac_grad_rows_kernel<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((sac_grad_rows_kernel<false>), grid, block, 0, s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || !dbias) return err;
    hipLaunchKernelGGL(sac_grad_finish_kernel, dim3((unsigned)((2 * A + 3) / 4)), block, 0, s, a);
    return hipGetLastError();
}

}  // namespace mms
