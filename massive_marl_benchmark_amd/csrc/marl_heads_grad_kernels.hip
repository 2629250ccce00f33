// marl_heads_grad_kernels.hip -- the output heads of the MAPPO / HAPPO update, forward and backward, for up to MMS_MAX_GROUPS networks
// per call (mms_marl_heads_fwd_group, mms_marl_heads_grad_group, include/mms.h; the arithmetic is marl_heads_grad_lane.h's).  A network
// is (f [M, H], w [A, H], b [A]) with A = 1 .. 16: an actor's DiagGaussian.fc_mean, or (A = 1) a critic's v_out.
//   heads_fwd_kernel          per row out = b + w f, and per group std = sigmoid(log_std / x_coef) y_coef
//   heads_grad_kernel         per row df = dout w; per workgroup the A (H + 1) sums over its rows [dout^T f | dout^T 1], in double
//   heads_grad_finish_kernel  one wave per element of [dw | db] adds the workgroups' partials in a fixed order and rounds once;
//                             dlog_std from dstd
// With N = A <= 16 these are not matrix products but streaming passes over [M, H], laid out as elu_ln_kernels.hip: one item = four
// consecutive columns of one row, moved with 16-byte accesses; the q = H / 4 threads of a row sit side by side, P = 256 / q rows are in
// flight per workgroup and thread (p, c) keeps its four columns, so its columns of w stay in registers.
// Registers: the action dimension is walked in tiles of AT = 1, 4 or 8 outputs (A = 1; A <= 4; otherwise), chosen per group and
// uniform over a workgroup; a tile keeps 4 AT weights and, backward, 4 AT + AT double accumulators per thread.  A > 8 takes two tiles:
// the second walks the workgroup's rows of f once more (they are the rows it has just read: 8 P or more, a few hundred KB), and df,
// which needs every j in ascending order under one rounding, is formed in the first tile with w's rows 8 .. A - 1 read through the cache.
// A row's sums over H (forward), in double: a thread adds its four columns in ascending order, then row_sum adds the row's q partials in
// an order that depends on q alone (elu_ln_kernels.hip's three shapes), so a row's outputs are a function of that row alone.
// Order of the sums over rows (backward): thread (p, c) adds its rows in ascending order; the P partials of an element are added in
// ascending p through LDS; chunk b of group g stores its A (H + 1) doubles at part[part_off[g] + b A (H + 1)]; the finish pass gives
// an element a wave: lane t adds the partials of chunks t and t + 64, then an xor butterfly (32 .. 1); one rounding to fp32.  No
// atomics, no memset: every word of the workspace that the finish pass reads was written by the row pass of the same call.  The
// partition is a function of (M, H), so nothing depends on `groups` and runs are bit-identical.
// Built with csrc/Makefile's PARAM_FLAGS: no fast-math, -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marl_heads_grad_args.h"
#include "marl_heads_grad_lane.h"

namespace mms {

int64_t marl_heads_grad_ws_bytes(int groups, int64_t M, int H, const int32_t* A) {
    int64_t doubles = 0;
    for (int g = 0; g < groups; g++) doubles += heads_chunks(M, H) * heads_part_doubles(A[g], H);
    return (doubles * (int64_t)sizeof(double) + 255) & ~(int64_t)255;
}

namespace {

__device__ __forceinline__ float4 hd_load(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 hd_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// v[k] <- the sum of v[k] over the q threads of the caller's row (threads p q .. p q + q - 1), the same bits in each of them: the three
// shapes of elu_ln_kernels.hip's row_sum.  Every thread of the workgroup calls it (live = false: a thread past the last row slot).
// s: a [K][256] LDS buffer that the previous call did not use.
template <int K>
__device__ __forceinline__ void hd_row_sum(double (&v)[K], int q, int p, bool live, int tid, double (*s)[kHeadsBlock]) {
    if ((q & (q - 1)) == 0) {                                       // (uniform over the workgroup, as every branch on q)
        for (int m = (q < 64 ? q : 64) >> 1; m >= 1; m >>= 1)
#pragma unroll
            for (int k = 0; k < K; k++) v[k] += __shfl_xor(v[k], m, 64);
        if (q <= 64) return;
        if ((tid & 63) == 0)
#pragma unroll
            for (int k = 0; k < K; k++) s[k][tid >> 6] = v[k];
        __syncthreads();
        const int w0 = (p * q) >> 6, n = q >> 6;                    // w0 + n <= 4
#pragma unroll
        for (int k = 0; k < K; k++) {
            double t = s[k][w0];
            for (int i = 1; i < n; i++) t += s[k][w0 + i];
            v[k] = t;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < K; k++) s[k][tid] = v[k];
    __syncthreads();
    if (!live) return;
    const int t0 = p * q;                                           // t0 + q <= P q <= 256
#pragma unroll
    for (int k = 0; k < K; k++) {
        double t = s[k][t0];
        for (int i = 1; i < q; i++) t += s[k][t0 + i];
        v[k] = t;
    }
}

// blockIdx.x: a slot of P rows, walking the rows with the stride of the grid
template <int AT>
__device__ __forceinline__ void heads_fwd_rows(const MarlHeadsFwdArgs& a, int g, double (*s_red)[8][kHeadsBlock]) {
    const int tid = (int)threadIdx.x, A = a.A[g];
    const int H = a.H, q = H >> 2, P = kHeadsBlock / q;             // q <= 256 items per row, P >= 1 rows in flight
    const int p = tid / q, c = tid - p * q, j = 4 * c;              // j + 3 < H
    const bool live = p < P;
    const float *f = a.f[g], *w = a.w[g], *b = a.b[g];
    float* out = a.out[g];
    int turn = 0;
    for (int j0 = 0; j0 < A; j0 += AT) {                            // (the same trips for the whole workgroup)
        float4 wr[AT];
        float bias[AT];
#pragma unroll
        for (int i = 0; i < AT; i++) {
            const bool has = live && j0 + i < A;
            wr[i] = has ? hd_load(w + (int64_t)(j0 + i) * H + j) : hd_zero();
            bias[i] = has ? b[j0 + i] : 0.f;
        }
        for (int64_t base = (int64_t)blockIdx.x * P; base < a.M; base += (int64_t)gridDim.x * P, turn ^= 1) {
            const int64_t row = base + p;
            const bool on = live && row < a.M;                      // rows past M are neither read nor written
            const float4 fv = on ? hd_load(f + row * a.f_pitch + j) : hd_zero();
            double v[AT];
#pragma unroll
            for (int i = 0; i < AT; i++)
                v[i] = ((heads_prod(fv.x, wr[i].x) + heads_prod(fv.y, wr[i].y)) + heads_prod(fv.z, wr[i].z)) + heads_prod(fv.w, wr[i].w);
            hd_row_sum<AT>(v, q, p, live, tid, s_red[turn]);
            if (on && c == 0) {
#pragma unroll
                for (int i = 0; i < AT; i++)
                    if (j0 + i < A) out[row * A + j0 + i] = heads_out(v[i], bias[i]);
            }
        }
    }
}

__global__ void __launch_bounds__(kHeadsBlock, 2) heads_fwd_kernel(MarlHeadsFwdArgs a) {
    __shared__ double s_red[2][8][kHeadsBlock];
    const int g = blockIdx.y, A = a.A[g];
    if (blockIdx.x == 0 && (int)threadIdx.x < A && a.log_std[g] != nullptr)
        a.std[g][threadIdx.x] = heads_std(a.log_std[g][threadIdx.x], a.x_coef, a.y_coef);
    if (A == 1) heads_fwd_rows<1>(a, g, s_red);
    else if (A <= 4) heads_fwd_rows<4>(a, g, s_red);
    else heads_fwd_rows<8>(a, g, s_red);
}

// blockIdx.x: the chunk of rows (marl_heads_grad_lane.h: heads_chunk_rows)
template <int AT>
__device__ __forceinline__ void heads_grad_rows(const MarlHeadsGradArgs& a, int g, double (*s_part)[kHeadsBlock]) {
    const int tid = (int)threadIdx.x, A = a.A[g];
    const int H = a.H, q = H >> 2, P = kHeadsBlock / q;
    const int p = tid / q, c = tid - p * q, j = 4 * c;              // j + 3 < H
    const bool live = p < P, sums = a.part != nullptr && a.dw[g] != nullptr;
    const float *f = a.f[g], *w = a.w[g], *dout = a.dout[g];
    float* df = a.df[g];
    if (!sums && df == nullptr) return;                             // (uniform over the workgroup)
    const int64_t row0 = (int64_t)blockIdx.x * a.chunk_rows;
    const int64_t row1 = row0 + a.chunk_rows < a.M ? row0 + a.chunk_rows : (int64_t)a.M;       // rows past M are neither read nor written
    double* part = sums ? a.part + a.part_off[g] + (int64_t)blockIdx.x * heads_part_doubles(A, H) : nullptr;
    for (int j0 = 0; j0 < A; j0 += AT) {                            // (the same trips for the whole workgroup)
        if (j0 > 0 && !sums) break;                                 // df is complete behind the first tile
        float4 wr[AT];
#pragma unroll
        for (int i = 0; i < AT; i++) wr[i] = (live && j0 + i < A) ? hd_load(w + (int64_t)(j0 + i) * H + j) : hd_zero();
        double acc[AT][4], accb[AT];
#pragma unroll
        for (int i = 0; i < AT; i++) { acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0; accb[i] = 0.0; }
        if (live)
            for (int64_t row = row0 + p; row < row1; row += P) {    // this thread's rows in ascending order
                float d[AT];
#pragma unroll
                for (int i = 0; i < AT; i++) d[i] = j0 + i < A ? dout[row * A + j0 + i] : 0.f;
                if (j0 == 0 && df != nullptr) {                     // df = sum_j dout[j] w[j, :], j ascending, rounded once
                    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
                    for (int i = 0; i < AT; i++) {                  // (an i past A adds 0 x 0)
                        s0 += heads_prod(d[i], wr[i].x); s1 += heads_prod(d[i], wr[i].y);
                        s2 += heads_prod(d[i], wr[i].z); s3 += heads_prod(d[i], wr[i].w);
                    }
                    for (int jj = AT; jj < A; jj++) {               // the second tile's rows of w, through the cache
                        const float dj = dout[row * A + jj];
                        const float4 wv = hd_load(w + (int64_t)jj * H + j);
                        s0 += heads_prod(dj, wv.x); s1 += heads_prod(dj, wv.y); s2 += heads_prod(dj, wv.z); s3 += heads_prod(dj, wv.w);
                    }
                    *reinterpret_cast<float4*>(df + row * a.df_pitch + j) = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
                }
                if (sums) {
                    const float4 fv = hd_load(f + row * a.f_pitch + j);
#pragma unroll
                    for (int i = 0; i < AT; i++) {
                        acc[i][0] += heads_prod(d[i], fv.x); acc[i][1] += heads_prod(d[i], fv.y);
                        acc[i][2] += heads_prod(d[i], fv.z); acc[i][3] += heads_prod(d[i], fv.w);
                        accb[i] += (double)d[i];
                    }
                }
            }
        if (!sums) break;
#pragma unroll
        for (int i = 0; i < AT; i++) {
            if (j0 + i >= A) break;                                 // (uniform)
            s_part[0][tid] = acc[i][0]; s_part[1][tid] = acc[i][1]; s_part[2][tid] = acc[i][2]; s_part[3][tid] = acc[i][3];
            s_part[4][tid] = accb[i];                               // (the row's first thread's counts: c == 0)
            __syncthreads();
            for (int o = tid; o < 4 * q + 1; o += kHeadsBlock) {    // o = k q + cc: column k of item cc; o = 4 q: the bias sum
                const int k = o / q, cc = o - k * q;
                double s = s_part[k][cc];
                for (int pp = 1; pp < P; pp++) s += s_part[k][pp * q + cc];
                if (k < 4) part[(int64_t)(j0 + i) * H + 4 * cc + k] = s;        // < A H
                else part[(int64_t)A * H + j0 + i] = s;                         // < A (H + 1)
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(kHeadsBlock, 2) heads_grad_kernel(MarlHeadsGradArgs a) {
    __shared__ double s_part[5][kHeadsBlock];
    const int g = blockIdx.y, A = a.A[g];
    if (A == 1) heads_grad_rows<1>(a, g, s_part);
    else if (A <= 4) heads_grad_rows<4>(a, g, s_part);
    else heads_grad_rows<8>(a, g, s_part);
}

// A wave per element of [dw | db] (four per workgroup, the group on blockIdx.y): lane t adds the partials of chunks t and t + 64 (a
// slot past `chunks` adds 0.0), then the xor butterfly 32 .. 1; one rounding.  chunks == 0 (M == 0): zeros.  The first workgroup of a
// group also turns dstd into dlog_std.
__global__ void __launch_bounds__(kHeadsBlock) heads_grad_finish_kernel(MarlHeadsGradArgs a) {
    static_assert(kHeadsMaxChunks == 128, "a finish-pass lane adds two partials");
    const int g = blockIdx.y, A = a.A[g], H = a.H, lane = (int)threadIdx.x & 63;
    const int C = A * (H + 1);
    if (blockIdx.x == 0 && (int)threadIdx.x < A && a.log_std[g] != nullptr && a.dlog_std[g] != nullptr)
        a.dlog_std[g][threadIdx.x] = heads_dlog_std(a.dstd[g][threadIdx.x], a.log_std[g][threadIdx.x], a.x_coef, a.y_coef);
    const int col = (int)blockIdx.x * (kHeadsBlock / 64) + ((int)threadIdx.x >> 6);
    if (col >= C || a.dw[g] == nullptr) return;                     // (wave-uniform)
    double s = 0.0;
    if (a.chunks > 0) {
        const double* p = a.part + a.part_off[g] + col;
        const double v0 = lane < a.chunks ? p[(int64_t)lane * C] : 0.0;
        const double v1 = lane + 64 < a.chunks ? p[(int64_t)(lane + 64) * C] : 0.0;
        s = v0 + v1;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane != 0) return;
    if (col < A * H) a.dw[g][col] = (float)s;
    else a.db[g][col - A * H] = (float)s;
}

bool heads_shapes_ok(int groups, int64_t M, int H, const int32_t* A) {
    if (groups < 1 || groups > MMS_MAX_GROUPS || M < 0 || M > 0x7fffffff || H < 4 || H > kHeadsMaxH || (H & 3)) return false;
    for (int g = 0; g < groups; g++)
        if (A[g] < 1 || A[g] > kHeadsMaxA) return false;
    return true;
}

}  // namespace

// the launch of a checked call (mms_host.h: check_marl_heads_fwd_group).  M == 0: one workgroup per group for std.
hipError_t launch_marl_heads_fwd_group(const MarlHeadsFwdArgs& a, int groups, hipStream_t s) {
    if (!heads_shapes_ok(groups, a.M, a.H, a.A)) return hipErrorInvalidValue;
    const int64_t P = kHeadsBlock / (a.H >> 2), slots = (a.M + 4 * P - 1) / (4 * P);                // about four trips per workgroup, 4096 slots at the most
    hipLaunchKernelGGL(heads_fwd_kernel, dim3((unsigned)(slots < 1 ? 1 : (slots < 4096 ? slots : 4096)), (unsigned)groups), dim3(kHeadsBlock), 0, s, a);
    return hipGetLastError();
}

// the launches of a checked call (mms_host.h: check_marl_heads_grad_group); a.part_off, a.chunk_rows and a.chunks are set here
hipError_t launch_marl_heads_grad_group(const MarlHeadsGradArgs& in, int groups, hipStream_t s) {
    if (!heads_shapes_ok(groups, in.M, in.H, in.A)) return hipErrorInvalidValue;
    MarlHeadsGradArgs a = in;
    a.chunk_rows = heads_chunk_rows(a.M, a.H);
    a.chunks = (int)heads_chunks(a.M, a.H);                         // <= kHeadsMaxChunks; M == 0: none
    bool sums = false, rows = false, stds = false;
    int64_t off = 0;
    int widest = 0;
    for (int g = 0; g < groups; g++) {
        a.part_off[g] = off;
        off += (int64_t)a.chunks * heads_part_doubles(a.A[g], a.H);
        sums = sums || a.dw[g] != nullptr;
        rows = rows || a.dw[g] != nullptr || a.df[g] != nullptr;
        stds = stds || (a.log_std[g] != nullptr && a.dlog_std[g] != nullptr);
        widest = a.A[g] > widest ? a.A[g] : widest;
    }
    if (!sums) a.part = nullptr;
    if (a.chunks > 0 && rows) {
        hipLaunchKernelGGL(heads_grad_kernel, dim3((unsigned)a.chunks, (unsigned)groups), dim3(kHeadsBlock), 0, s, a);
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    if (!sums && !stds) return hipSuccess;
    const int cols = sums ? widest * (a.H + 1) : 1;                 // 4 elements per workgroup
    hipLaunchKernelGGL(heads_grad_finish_kernel, dim3((unsigned)((cols + 3) / 4), (unsigned)groups), dim3(kHeadsBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace mms
