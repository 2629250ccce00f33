// det_head_kernels.hip -- the backward of the deterministic actor head's epilogue for gfx950 (mms_det_heads_grad, include/mms.h):
//   det_grad_rows_kernel    dy [N,A] = (act_limit g) (1 - t^2) from the forward's saved t = tanh(pre) and the incoming gradient g
//                           (det_head_lane.h); per workgroup the A column sums of its rows, in double
//   det_grad_finish_kernel  one wave per column adds the workgroups' partials in a fixed order and rounds once: dbias [A]
// (The forward, mms_det_heads_act, is maddpg_kernels.hip's det_heads_act_kernel with one group: its bits are the grouped entry's.)
// A streaming pass on sac_grad_kernels.hip's plan: a workgroup owns TILES of R whole rows (R = det_grad_tile_rows(A): a multiple of 4
// with R A <= 1024, so every tile of a 16-byte aligned dense array starts 16-byte aligned); thread i owns elements 4 i .. 4 i + 3 of the
// tile: t in as one float4 and dy out as one float4 whatever A is (the elements past the last row's end one by one).  g is NOT dense:
// it is read where it lies, A columns of rows that are grad_pitch floats apart (the action columns of the critic's input gradient), as
// one float4 where the thread's four elements are four consecutive floats of one row at a 16-byte boundary (A and grad_pitch multiples
// of 4, g 16-byte aligned), one by one otherwise.  With a t or dy that is not 16-byte aligned every access is scalar.  The arithmetic
// and every sum's order are the same on all three paths.
// Tiles go to workgroups round robin (tile, tile + grid, ..; grid = min(tiles, 1024)): the number of partial rows is bounded.
// Order of the column sums.  The 256 threads form P = 256 / A row groups of A columns; thread (p, c) adds dy[r][c] of the tile's LDS
// image for r = p, p + P, .. of each of its workgroup's tiles in tile order, in double; the P partials of a column are added in
// ascending p; block b stores its A doubles at part[b A + c]; the finish pass gives a column a wave: lane l adds the partials of
// blocks l, l + 64, .. in ascending order, then an xor butterfly (32 .. 1); one rounding to fp32.  No atomics, no memset: every word of
// the workspace that the finish pass reads was written by the row pass of the same call.
// Built like sac_grad_kernels.hip (csrc/Makefile: PARAM_FLAGS): no fast-math, -ffp-contract=off, so the three paths and the CPU
// build's evaluation of det_head_lane.h round every operation alike.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "det_head_lane.h"

namespace mms {

constexpr int kDgThreads = 256;
constexpr int kDgMaxBlocks = 1024;              // 4 per CU: rows of partials the finish pass adds per column
constexpr int kDgMaxA = 128;

struct DetGradArgs {
    const float *t, *g;
    float* dy;
    float* dbias;
    double* part;
    int64_t N, tiles, grad_pitch;
    int A, R, blocks;
    float act_limit;
};

struct DetGradPlan { int R, blocks; int64_t tiles, bytes; };

static DetGradPlan det_grad_plan(int64_t N, int A) {
    DetGradPlan p;
    p.R = det_grad_tile_rows(A);
    p.tiles = (N + p.R - 1) / p.R;
    p.blocks = (int)(p.tiles < kDgMaxBlocks ? p.tiles : kDgMaxBlocks);
    p.bytes = (((int64_t)p.blocks * A * (int64_t)sizeof(double)) + 255) & ~(int64_t)255;
    return p;
}

int64_t det_grad_ws_bytes(int64_t N, int A) { return det_grad_plan(N, A).bytes; }

// VEC: t and dy 16-byte aligned.  GVEC (needs VEC): A % 4 == 0, grad_pitch % 4 == 0 and g 16-byte aligned.
template <bool VEC, bool GVEC>
__global__ void __launch_bounds__(kDgThreads) det_grad_rows_kernel(DetGradArgs a) {
    __shared__ __align__(16) float s_dy[kDetGradTile];         // the tile's rows of dy
    __shared__ double s_col[kDgThreads];
    const int tid = (int)threadIdx.x, A = a.A, R = a.R;
    const int P = kDgThreads / A, p = tid / A, c = tid - p * A;
    const bool sums = a.part != nullptr && p < P;
    const int k0 = 4 * tid;
    double acc = 0.0;

    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t row0 = tile * R;
        const int rows = (a.N - row0 < R) ? (int)(a.N - row0) : R;              // rows past N are neither read nor written
        const int cnt = rows * A;                                                // <= kDetGradTile
        if (k0 < cnt) {
            const float* tt = a.t + row0 * A;
            const int r = k0 / A, j = k0 - r * A;
            float xt[4], xg[4];
            const bool full = k0 + 3 < cnt;
            if (VEC && full) {
                const float4 v = *reinterpret_cast<const float4*>(tt + k0);
                xt[0] = v.x; xt[1] = v.y; xt[2] = v.z; xt[3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) xt[k] = (k0 + k < cnt) ? tt[k0 + k] : 0.f;
            }
            if (GVEC && full) {                                                  // j % 4 == 0 and j + 3 < A: one row, one 16-byte word
                const float4 v = *reinterpret_cast<const float4*>(a.g + (row0 + r) * a.grad_pitch + j);
                xg[0] = v.x; xg[1] = v.y; xg[2] = v.z; xg[3] = v.w;
            } else {
                int rr = r, jj = j;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    xg[k] = (k0 + k < cnt) ? a.g[(row0 + rr) * a.grad_pitch + jj] : 0.f;
                    if (++jj == A) { jj = 0; rr++; }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k0 + k < cnt) s_dy[k0 + k] = det_head_grad_one(xt[k], xg[k], a.act_limit);
        }
        __syncthreads();
        float* dst = a.dy + row0 * A;
        const int nvec = VEC ? cnt >> 2 : 0;
        for (int i = tid; i < nvec; i += kDgThreads) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(s_dy)[i];
        for (int i = 4 * nvec + tid; i < cnt; i += kDgThreads) dst[i] = s_dy[i];
        if (sums)
            for (int r = p; r < rows; r += P) acc += (double)s_dy[r * A + c];
        __syncthreads();                                                         // the next tile rewrites s_dy
    }

    if (a.part == nullptr) return;
    s_col[tid] = acc;
    __syncthreads();
    if (tid < A) {
        double s = s_col[tid];
        for (int q = 1; q < P; q++) s += s_col[q * A + tid];
        a.part[(int64_t)blockIdx.x * A + tid] = s;
    }
}

// A wave per column (four columns per workgroup): lane l adds the partials of blocks l, l + 64, .. in ascending order (at most 16,
// every load in flight at once; a slot past `blocks` adds 0.0, which changes nothing), then the xor butterfly 32 .. 1; one rounding.
__global__ void __launch_bounds__(kDgThreads) det_grad_finish_kernel(DetGradArgs a) {
    const int A = a.A, lane = (int)threadIdx.x & 63;
    const int col = (int)blockIdx.x * (kDgThreads / 64) + ((int)threadIdx.x >> 6);
    if (col >= A) return;                                            // (wave-uniform)
    const double* p = a.part + col;
    double v[kDgMaxBlocks / 64];
#pragma unroll
    for (int k = 0; k < kDgMaxBlocks / 64; k++) {
        const int b = 64 * k + lane;
        v[k] = b < a.blocks ? p[(int64_t)b * A] : 0.0;
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kDgMaxBlocks / 64; k++) s += v[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) a.dbias[col] = (float)s;
}

// the launches of a checked call (mms_host.h: check_det_heads_grad); N >= 1
hipError_t launch_det_heads_grad(int64_t N, int A, float act_limit, const float* t, const float* g, int64_t grad_pitch, float* dy, float* dbias,
                                 void* workspace, hipStream_t s) {
    if (N < 1 || N > 0x7fffffff || A < 1 || A > kDgMaxA || grad_pitch < A) return hipErrorInvalidValue;   // (the entry's check refuses it with a message)
    const DetGradPlan p = det_grad_plan(N, A);
    DetGradArgs a = {};
    a.t = t; a.g = g; a.dy = dy; a.dbias = dbias;
    a.part = dbias ? static_cast<double*>(workspace) : nullptr;
    a.N = N; a.tiles = p.tiles; a.grad_pitch = grad_pitch; a.A = A; a.R = p.R; a.blocks = p.blocks;
    a.act_limit = act_limit;
    const bool vec = ((reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(dy)) & 15) == 0;
    const bool gvec = vec && (reinterpret_cast<uintptr_t>(g) & 15) == 0 && A % 4 == 0 && grad_pitch % 4 == 0;
    const dim3 grid((unsigned)p.blocks), block(kDgThreads);
    if (gvec) hipLaunchKernelGGL((det_grad_rows_kernel<true, true>), grid, block, 0, s, a);
    else if (vec) hipLaunchKernelGGL((det_grad_rows_kernel<true, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((det_grad_rows_kernel<false, false>), grid, block, 0, s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || !dbias) return err;
    hipLaunchKernelGGL(det_grad_finish_kernel, dim3((unsigned)((A + 3) / 4)), block, 0, s, a);
    return hipGetLastError();
}

}  // namespace mms
