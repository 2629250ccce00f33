// elu_ln_kernels.hip -- what a `Linear + ELU + LayerNorm` block does besides its matrix products, forward and backward, for up to
// MMS_MAX_GROUPS networks per call (mms_elu_ln_group, mms_elu_ln_planes16_group, mms_elu_ln_grad_group, include/mms.h; the arithmetic
// is elu_ln_lane.h's, the operand format planes16_lane.h's):
//   elu_ln_kernel          per row y = LayerNorm(ELU(z + bias)) and the row's (mean, rstd)
//   elu_ln_planes_kernel   the same rows by the same statements, and y once more as the H32 operand planes of the two-plane fp16 layer
//                          kernel (split16_kernels.hip) with the row's scale: what split16_planes_kernel would make of y, byte for byte
//   elu_ln_grad_kernel     per row dz from z, bias, gamma, the saved (mean, rstd) and dy; per workgroup the 3H column sums
//                          [dz | dy xhat | dy] of its rows, in double
//   elu_ln_finish_kernel   one wave per column adds the workgroups' partials in a fixed order and rounds once: dparams [3H]
// The products (z = x W^T, dW = dz^T x, dx = dz W) stay with the caller's library.
// Streaming passes with 16-byte accesses, laid out as gru_grad_kernels.hip: one item = four consecutive columns of one row; the
// q = H / 4 threads of a row sit side by side, P = 256 / q rows are in flight per workgroup and thread (p, c) keeps its four columns, so
// bias, gamma and beta are loaded once and the backward's twelve column sums stay in registers.  Forward: 1 load and 1 store per item
// (two passes over [M, H]); backward: 2 loads and 1 store (three passes).
// A row's sums (forward: sum a, then sum (a - mean)^2; backward: sum q and sum q xhat together), in double: a thread adds its four
// columns in ascending order, then row_sum adds the row's q partials in an order that depends on q alone --
//   q a power of two up to 64    the row is an aligned segment of one wave: xor butterfly q / 2 .. 1, no LDS, no barrier
//   q = 128, 256                 the butterfly 32 .. 1 in each of the row's 2 / 4 waves, the waves' sums through LDS in ascending order
//   any other q                  (rows straddle waves, 256 - P q threads idle) the q partials through LDS in ascending order
// so every thread of a row holds the same bits and a row's outputs are a function of that row alone.
// Order of the column sums (gru_grad_kernels.hip's): thread (p, c) adds its rows in ascending order, in double; the P partials of a
// column are added in ascending p through LDS; chunk b of group g stores its 3H doubles at part[(g chunks + b) 3H + col]; the finish
// pass gives a column a wave: lane t adds the partials of chunks t, t + 64, .. in ascending order, then an xor butterfly (32 .. 1); one
// rounding to fp32.  No atomics, no memset: every word of the workspace that the finish pass reads was written by the row pass of the
// same call.  The partition is a function of (M, H), so dparams does not depend on `groups` and runs are bit-identical.
// Built with csrc/Makefile's PARAM_FLAGS: accurate expm1f, no fast-math, -ffp-contract=off (the double division and square root are IEEE
// in any case).  The row pass of the backward is bounded to four waves per SIMD (126 VGPRs, no scratch): with the cap of 512 chunks that
// is four resident workgroups per CU for two networks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "elu_ln_args.h"
#include "elu_ln_lane.h"
#include "planes16_lane.h"

namespace mms {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

int64_t elu_ln_grad_ws_bytes(int groups, int64_t M, int H) {
    return (((int64_t)groups * elu_ln_chunks(M, H) * 3 * H * (int64_t)sizeof(double)) + 255) & ~(int64_t)255;
}

__device__ __forceinline__ float4 el_load(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void el_store(float* p, float a, float b, float c, float d) { *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d); }
__device__ __forceinline__ double el_sum4(double a, double b, double c, double d) { return ((a + b) + c) + d; }

// v[k] <- the sum of v[k] over the q threads of the caller's row (threads p q .. p q + q - 1), the same bits in each of them.  Every
// thread of the workgroup calls it (a thread without a row passes zeros; live = false: a thread past the last row slot, p >= P).  s: a
// [K][256] LDS buffer that the previous call did not use (its readers may still be at work; two buffers in turn are enough, since
// every call that touches LDS has a barrier between its writes and its reads).
template <int K>
__device__ __forceinline__ void row_sum(double (&v)[K], int q, int p, bool live, int tid, double (*s)[kEluLnBlock]) {
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

// v <- the largest v over the q threads of the caller's row, in row_sum's three shapes (a maximum does not depend on the order, so
// the shape only decides who talks to whom).  s: a [256] LDS buffer of its own.
__device__ __forceinline__ float row_max(float v, int q, int p, bool live, int tid, float* s) {
    if ((q & (q - 1)) == 0) {
        for (int m = (q < 64 ? q : 64) >> 1; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
        if (q <= 64) return v;
        if ((tid & 63) == 0) s[tid >> 6] = v;
        __syncthreads();
        const int w0 = (p * q) >> 6, n = q >> 6;                    // w0 + n <= 4
        float t = s[w0];
        for (int i = 1; i < n; i++) t = fmaxf(t, s[w0 + i]);
        return t;
    }
    s[tid] = v;
    __syncthreads();
    if (!live) return v;
    const int t0 = p * q;                                           // t0 + q <= P q <= 256
    float t = s[t0];
    for (int i = 1; i < q; i++) t = fmaxf(t, s[t0 + i]);
    return t;
}

// four columns of a row into its H32 planes (planes16_lane.h: element k of row `row`, its lo value 32 halves on), 8 bytes each
__device__ __forceinline__ void el_store_planes(_Float16* planes, int64_t row, int KC, int k, float scale, float a, float b, float c, float d) {
    const float t[4] = {a * scale, b * scale, c * scale, d * scale};
    f16x4 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        hi[i] = (_Float16)t[i];
        lo[i] = (_Float16)planes16_lo(t[i], (float)hi[i]);
    }
    _Float16* dst = planes16_elem(planes, row, KC, k);              // k a multiple of 4: 8-byte aligned, inside one 32-column chunk
    *reinterpret_cast<f16x4*>(dst) = hi;
    *reinterpret_cast<f16x4*>(dst + 32) = lo;
}

// blockIdx.x: a slot of P rows, walking the rows with the stride of the grid; blockIdx.y: the group.
// PLANES (mms_elu_ln_planes16_group): the thread still holds its four y when they are stored, so one more reduction over the row -- its
// largest |y| -- gives the row's power-of-two scale (pow2_scale), and the thread stores its four columns of the hi and of the lo plane
// as well: what mms_split_planes16_group would make of y, without reading y again.  The columns from H to the next multiple of 32 are
// written as zero by the row's first threads.  s_max: LDS of its own, the third buffer in turn.
template <bool PLANES>
__device__ __forceinline__ void elu_ln_rows(const EluLnArgs& a, const EluLnPlanesArgs* pl, double (*s_red)[1][kEluLnBlock], float* s_max) {
    const int g = blockIdx.y, tid = (int)threadIdx.x;
    const int H = a.H, q = H >> 2, P = kEluLnBlock / q;             // q <= 256 items per row, P >= 1 rows in flight
    const int p = tid / q, c = tid - p * q, j = 4 * c;              // j + 3 < H
    const bool live = p < P;
    const int KC = (H + 31) >> 5;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f), ga = b, be = b;
    if (live) { b = el_load(a.bias[g] + j); ga = el_load(a.gamma[g] + j); be = el_load(a.beta[g] + j); }
    for (int64_t base = (int64_t)blockIdx.x * P; base < a.M; base += (int64_t)gridDim.x * P) {      // (the same trips for the whole workgroup)
        const int64_t row = base + p;
        const bool on = live && row < a.M;                          // rows past M are neither read nor written
        float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) zv = el_load(a.z[g] + row * a.z_pitch + j);
        const float ax = elu_ln_act(elu_ln_u(zv.x, b.x)), ay = elu_ln_act(elu_ln_u(zv.y, b.y));
        const float az = elu_ln_act(elu_ln_u(zv.z, b.z)), aw = elu_ln_act(elu_ln_u(zv.w, b.w));
        double s[1] = {on ? el_sum4(ax, ay, az, aw) : 0.0};
        row_sum<1>(s, q, p, live, tid, s_red[0]);
        const float mean = elu_ln_mean(s[0], H);
        double v[1] = {on ? el_sum4(elu_ln_dev2(ax, mean), elu_ln_dev2(ay, mean), elu_ln_dev2(az, mean), elu_ln_dev2(aw, mean)) : 0.0};
        row_sum<1>(v, q, p, live, tid, s_red[1]);
        const float rstd = elu_ln_rstd(v[0], H, a.eps);
        const float yx = elu_ln_out(elu_ln_xhat(ax, mean, rstd), ga.x, be.x), yy = elu_ln_out(elu_ln_xhat(ay, mean, rstd), ga.y, be.y);
        const float yz = elu_ln_out(elu_ln_xhat(az, mean, rstd), ga.z, be.z), yw = elu_ln_out(elu_ln_xhat(aw, mean, rstd), ga.w, be.w);
        if (on) {
            el_store(a.y[g] + row * a.y_pitch + j, yx, yy, yz, yw);
            if (c == 0) *reinterpret_cast<float2*>(a.stat[g] + 2 * row) = make_float2(mean, rstd);
        }
        if (PLANES) {
            const float big = row_max(on ? fmaxf(fmaxf(fabsf(yx), fabsf(yy)), fmaxf(fabsf(yz), fabsf(yw))) : 0.f, q, p, live, tid, s_max);
            if (!on) continue;
            float scale, inv;
            pow2_scale(big, scale, inv);
            _Float16* planes = reinterpret_cast<_Float16*>(pl->planes[g]);
            el_store_planes(planes, row, KC, j, scale, yx, yy, yz, yw);
            for (int k = H + j; k < 32 * KC; k += H) el_store_planes(planes, row, KC, k, scale, 0.f, 0.f, 0.f, 0.f);     // the zero tail: at most 7 items
            if (c == 0) {
                if (pl->scale[g]) pl->scale[g][row] = scale;
                if (pl->inv[g]) pl->inv[g][row] = inv;
            }
        }
    }
}

__global__ void __launch_bounds__(kEluLnBlock) elu_ln_kernel(EluLnArgs a) {
    __shared__ double s_red[2][1][kEluLnBlock];
    elu_ln_rows<false>(a, nullptr, s_red, nullptr);
}

__global__ void __launch_bounds__(kEluLnBlock) elu_ln_planes_kernel(EluLnPlanesArgs a) {
    __shared__ double s_red[2][1][kEluLnBlock];
    __shared__ float s_max[kEluLnBlock];
    elu_ln_rows<true>(a.e, &a, s_red, s_max);
}

// blockIdx.x: the chunk of rows (elu_ln_lane.h: elu_ln_chunk_rows), blockIdx.y: the group
__global__ void __launch_bounds__(kEluLnBlock, 4) elu_ln_grad_kernel(EluLnGradArgs a) {
    __shared__ double s_part[12][kEluLnBlock];                      // [3 sums x 4 columns][thread]
    __shared__ double s_red[2][2][kEluLnBlock];
    const int g = blockIdx.y, tid = (int)threadIdx.x;
    const int H = a.H, q = H >> 2, P = kEluLnBlock / q;
    const int p = tid / q, c = tid - p * q, j = 4 * c;              // j + 3 < H
    const bool live = p < P, sums = a.part != nullptr && a.dparams[g] != nullptr;
    const int64_t row0 = (int64_t)blockIdx.x * a.chunk_rows;
    const int64_t row1 = row0 + a.chunk_rows < a.M ? row0 + a.chunk_rows : (int64_t)a.M;       // rows past M are neither read nor written
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f), ga = b;
    if (live) { b = el_load(a.bias[g] + j); ga = el_load(a.gamma[g] + j); }
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.0;

    // a row's three loads are issued one trip ahead, so they are in flight while the trip before them is in its row sums
    struct Row { float4 z, dy; float2 st; };
    const auto fetch = [&](int64_t row) {
        Row r = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float2(0.f, 0.f)};
        if (live && row < row1) {
            r.z = el_load(a.z[g] + row * a.z_pitch + j);
            r.dy = el_load(a.dy[g] + row * a.dy_pitch + j);
            r.st = *reinterpret_cast<const float2*>(a.stat[g] + 2 * row);
        }
        return r;
    };
    Row next = fetch(row0 + p);
    int turn = 0;
    for (int64_t base = row0; base < row1; base += P, turn ^= 1) {  // (the same trips for the whole workgroup)
        const int64_t row = base + p;
        const bool on = live && row < row1;
        const float4 zv = next.z, d = next.dy;
        const float2 st = next.st;
        next = fetch(row + P);
        const float ux = elu_ln_u(zv.x, b.x), uy = elu_ln_u(zv.y, b.y), uz = elu_ln_u(zv.z, b.z), uw = elu_ln_u(zv.w, b.w);
        const float ax = elu_ln_act(ux), ay = elu_ln_act(uy), az = elu_ln_act(uz), aw = elu_ln_act(uw);
        const double hx = elu_ln_xhat(ax, st.x, st.y), hy = elu_ln_xhat(ay, st.x, st.y), hz = elu_ln_xhat(az, st.x, st.y), hw = elu_ln_xhat(aw, st.x, st.y);
        const double qx = elu_ln_q(d.x, ga.x), qy = elu_ln_q(d.y, ga.y), qz = elu_ln_q(d.z, ga.z), qw = elu_ln_q(d.w, ga.w);
        double r[2] = {on ? el_sum4(qx, qy, qz, qw) : 0.0, on ? el_sum4(qx * hx, qy * hy, qz * hz, qw * hw) : 0.0};
        row_sum<2>(r, q, p, live, tid, s_red[turn]);
        if (!on) continue;
        const double c1 = elu_ln_row_mean(r[0], H), c2 = elu_ln_row_mean(r[1], H);
        const float gx = elu_ln_dz(ux, ax, hx, st.y, qx, c1, c2), gy = elu_ln_dz(uy, ay, hy, st.y, qy, c1, c2);
        const float gz = elu_ln_dz(uz, az, hz, st.y, qz, c1, c2), gw = elu_ln_dz(uw, aw, hw, st.y, qw, c1, c2);
        el_store(a.dz[g] + row * a.dz_pitch + j, gx, gy, gz, gw);
        if (sums) {
            acc[0] += (double)gx;          acc[1] += (double)gy;          acc[2] += (double)gz;           acc[3] += (double)gw;
            acc[4] += (double)d.x * hx;    acc[5] += (double)d.y * hy;    acc[6] += (double)d.z * hz;     acc[7] += (double)d.w * hw;
            acc[8] += (double)d.x;         acc[9] += (double)d.y;         acc[10] += (double)d.z;         acc[11] += (double)d.w;
        }
    }

    if (!sums) return;                                              // (uniform over the workgroup)
#pragma unroll
    for (int k = 0; k < 12; k++) s_part[k][tid] = acc[k];
    __syncthreads();
    double* part = a.part + ((int64_t)g * a.chunks + blockIdx.x) * (3 * (int64_t)H);
    for (int o = tid; o < 12 * q; o += kEluLnBlock) {               // o = k q + cc: sum k (which of the three, which column) of item cc
        const int k = o / q, cc = o - k * q;
        double s = s_part[k][cc];
        for (int pp = 1; pp < P; pp++) s += s_part[k][pp * q + cc];
        part[(k >> 2) * H + 4 * cc + (k & 3)] = s;                  // < 3H: k < 12, cc < q
    }
}

// A wave per column (four columns per workgroup, the group on blockIdx.y): lane t adds the partials of chunks t, t + 64, .. in
// ascending order (a slot past `chunks` adds 0.0, which changes nothing), then the xor butterfly 32 .. 1; one rounding.  chunks == 0
// (M == 0): zeros.
__global__ void __launch_bounds__(kEluLnBlock) elu_ln_finish_kernel(EluLnGradArgs a) {
    const int g = blockIdx.y, C = 3 * a.H, lane = (int)threadIdx.x & 63;
    const int col = (int)blockIdx.x * (kEluLnBlock / 64) + ((int)threadIdx.x >> 6);
    float* out = a.dparams[g];
    if (col >= C || out == nullptr) return;                         // (wave-uniform)
    const double* p = a.part + (int64_t)g * a.chunks * C + col;
    double v[kEluLnMaxChunks / 64];
#pragma unroll
    for (int k = 0; k < kEluLnMaxChunks / 64; k++) {
        const int b = 64 * k + lane;
        v[k] = b < a.chunks ? p[(int64_t)b * C] : 0.0;
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kEluLnMaxChunks / 64; k++) s += v[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) out[col] = (float)s;
}

// the launch of a checked call (mms_host.h: check_elu_ln_group)
hipError_t launch_elu_ln_group(const EluLnArgs& a, int groups, hipStream_t s) {
    if (a.M == 0 || groups == 0) return hipSuccess;
    if (groups < 0 || groups > MMS_MAX_GROUPS || a.M < 0 || a.H < 4 || a.H > kEluLnMaxH || (a.H & 3)) return hipErrorInvalidValue;
    const int64_t P = kEluLnBlock / (a.H >> 2), slots = (a.M + 4 * P - 1) / (4 * P);                // about four trips per workgroup, 4096 slots at the most
    hipLaunchKernelGGL(elu_ln_kernel, dim3((unsigned)(slots < 4096 ? slots : 4096), (unsigned)groups), dim3(kEluLnBlock), 0, s, a);
    return hipGetLastError();
}

// the launch of a checked call (mms_host.h: check_elu_ln_planes16_group): elu_ln_kernel's grid
hipError_t launch_elu_ln_planes16_group(const EluLnPlanesArgs& a, int groups, hipStream_t s) {
    const EluLnArgs& e = a.e;
    if (e.M == 0 || groups == 0) return hipSuccess;
    if (groups < 0 || groups > MMS_MAX_GROUPS || e.M < 0 || e.H < 4 || e.H > kEluLnMaxH || (e.H & 3)) return hipErrorInvalidValue;
    const int64_t P = kEluLnBlock / (e.H >> 2), slots = (e.M + 4 * P - 1) / (4 * P);
    hipLaunchKernelGGL(elu_ln_planes_kernel, dim3((unsigned)(slots < 4096 ? slots : 4096), (unsigned)groups), dim3(kEluLnBlock), 0, s, a);
    return hipGetLastError();
}

// the launches of a checked call (mms_host.h: check_elu_ln_grad_group); a.part, a.chunk_rows and a.chunks are set here
hipError_t launch_elu_ln_grad_group(const EluLnGradArgs& in, int groups, hipStream_t s) {
    if (groups == 0) return hipSuccess;
    if (groups < 0 || groups > MMS_MAX_GROUPS || in.M < 0 || in.H < 4 || in.H > kEluLnMaxH || (in.H & 3)) return hipErrorInvalidValue;
    EluLnGradArgs a = in;
    a.chunk_rows = elu_ln_chunk_rows(a.M, a.H);
    a.chunks = (int)elu_ln_chunks(a.M, a.H);                        // <= kEluLnMaxChunks; M == 0: none
    bool sums = false;
    for (int g = 0; g < groups; g++) sums = sums || a.dparams[g] != nullptr;
    if (!sums) a.part = nullptr;
    if (a.chunks > 0) {
        hipLaunchKernelGGL(elu_ln_grad_kernel, dim3((unsigned)a.chunks, (unsigned)groups), dim3(kEluLnBlock), 0, s, a);
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    if (!sums) return hipSuccess;
    hipLaunchKernelGGL(elu_ln_finish_kernel, dim3((unsigned)((3 * a.H + 3) / 4), (unsigned)groups), dim3(kEluLnBlock), 0, s, a);   // 3H columns, 4 per workgroup
    return hipGetLastError();
}

}  // namespace mms
