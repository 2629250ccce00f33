// gru_grad_kernels.hip -- the backward of the GRU gate step for up to MMS_MAX_GROUPS networks per call (mms_gru_gates_grad_group,
// include/mms.h; the forward is gru_gates_kernels.hip):
//   gru_gates_grad_kernel    per row and hidden unit dgi, dgh [M, 3H] and the direct dh [M, H] from the forward's inputs and the incoming
//                            gradient (gru_grad_lane.h recomputes r, z, n by gru_lane.h's statements); per workgroup the 4H column sums
//                            [dpr | dpz | dpn | r dpn] of its rows, in double
//   gru_grad_finish_kernel   one wave per column adds the workgroups' partials in a fixed order and rounds once: dbias [4H]
// The matrix products of the step (dh += dgh W_hh, and after the loop dW_ih, dW_hh, dX) stay with the caller's library.
// A streaming pass with 16-byte accesses.  One item = four consecutive hidden units of one row: twelve loads (r, z, n of gi and of gh, h,
// dh_out, dy, and three of b_hh that a thread loads once) and seven stores.  Unlike the forward's roaming item index a thread keeps its
// four columns: the H / 4 threads of a row sit side by side (a row's accesses are H * 4 consecutive bytes per array), P = 256 / (H / 4)
// rows are in flight per workgroup, and thread (p, c) walks rows p, p + P, .. of the workgroup's chunk, so its sixteen column sums stay
// in registers.  Chunks: gru_grad_lane.h's gru_grad_chunk_rows(M, H), the chunk on blockIdx.x and the group on blockIdx.y.
// Order of the column sums: thread (p, c) adds its rows in ascending order, in double; the P partials of a column are added in ascending
// p through LDS; chunk b of group g stores its 4H doubles at part[(g chunks + b) 4H + col]; the finish pass gives a column a wave: lane
// t adds the partials of chunks t, t + 64, .. in ascending order, then an xor butterfly (32 .. 1); one rounding to fp32.  No atomics, no
// memset: every word of the workspace that the finish pass reads was written by the row pass of the same call.  The partition is a
// function of (M, H), so dbias does not depend on `groups` and runs are bit-identical.
// Built like gru_gates_kernels.hip (csrc/Makefile: PARAM_FLAGS): accurate expf / tanhf, IEEE division, -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gru_grad_args.h"
#include "gru_grad_lane.h"

namespace mms {

int64_t gru_grad_ws_bytes(int groups, int64_t M, int H) {
    return (((int64_t)groups * gru_grad_chunks(M, H) * 4 * H * (int64_t)sizeof(double)) + 255) & ~(int64_t)255;
}

__device__ __forceinline__ float4 gg_load(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void gg_store(float* p, float a, float b, float c, float d) { *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d); }

__global__ void __launch_bounds__(kGruGradBlock) gru_gates_grad_kernel(GruGradArgs a) {
    __shared__ double s_part[16][kGruGradBlock];                   // [4 sums x 4 units][thread]
    const int g = blockIdx.y, tid = (int)threadIdx.x;
    const int H = a.H, q = H >> 2, P = kGruGradBlock / q;          // q <= 256 items per row, P >= 1 rows in flight
    const int p = tid / q, c = tid - p * q, j = 4 * c;             // j + 3 < H
    const float* __restrict__ Mk = a.mask[g];
    const float* __restrict__ Dy = a.dy[g];
    const bool masked = Mk != nullptr, sums = a.part != nullptr && a.dbias[g] != nullptr;
    const int64_t row0 = (int64_t)blockIdx.x * a.chunk_rows;
    const int64_t row1 = row0 + a.chunk_rows < a.M ? row0 + a.chunk_rows : (int64_t)a.M;       // rows past M are neither read nor written
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = 0.0;

    if (p < P) {
        const float* Bh = a.b_hh[g] + j;
        const float4 br = gg_load(Bh), bz = gg_load(Bh + H), bn = gg_load(Bh + 2 * H);
        for (int64_t row = row0 + p; row < row1; row += P) {
            const float* gi = a.gi[g] + row * a.g_pitch + j;
            const float* gh = a.gh[g] + row * a.g_pitch + j;
            const float4 ir = gg_load(gi), iz = gg_load(gi + H), in = gg_load(gi + 2 * H);
            const float4 hr = gg_load(gh), hz = gg_load(gh + H), hn = gg_load(gh + 2 * H);
            const float4 hv = gg_load(a.h[g] + row * a.h_pitch + j);
            float4 G = gg_load(a.dh_out[g] + row * a.dh_out_pitch + j);
            if (Dy) {
                const float4 d = gg_load(Dy + row * a.dy_pitch + j);
                G.x += d.x; G.y += d.y; G.z += d.z; G.w += d.w;
            }
            const float m = masked ? Mk[row * a.mask_pitch] : 1.f;
            const GruGateGrad x = gru_gates_grad(masked, m, ir.x, iz.x, in.x, hr.x, hz.x, hn.x, br.x, bz.x, bn.x, hv.x, G.x);
            const GruGateGrad y = gru_gates_grad(masked, m, ir.y, iz.y, in.y, hr.y, hz.y, hn.y, br.y, bz.y, bn.y, hv.y, G.y);
            const GruGateGrad z = gru_gates_grad(masked, m, ir.z, iz.z, in.z, hr.z, hz.z, hn.z, br.z, bz.z, bn.z, hv.z, G.z);
            const GruGateGrad w = gru_gates_grad(masked, m, ir.w, iz.w, in.w, hr.w, hz.w, hn.w, br.w, bz.w, bn.w, hv.w, G.w);
            float* di = a.dgi[g] + row * a.dg_pitch + j;
            float* dg = a.dgh[g] + row * a.dg_pitch + j;
            gg_store(di, x.dpr, y.dpr, z.dpr, w.dpr);
            gg_store(di + H, x.dpz, y.dpz, z.dpz, w.dpz);
            gg_store(di + 2 * H, x.dpn, y.dpn, z.dpn, w.dpn);
            gg_store(dg, x.dgh_r, y.dgh_r, z.dgh_r, w.dgh_r);
            gg_store(dg + H, x.dgh_z, y.dgh_z, z.dgh_z, w.dgh_z);
            gg_store(dg + 2 * H, x.dgh_n, y.dgh_n, z.dgh_n, w.dgh_n);
            gg_store(a.dh[g] + row * a.dh_pitch + j, x.dh, y.dh, z.dh, w.dh);
            if (sums) {
                acc[0] += (double)x.dpr;   acc[1] += (double)y.dpr;   acc[2] += (double)z.dpr;   acc[3] += (double)w.dpr;
                acc[4] += (double)x.dpz;   acc[5] += (double)y.dpz;   acc[6] += (double)z.dpz;   acc[7] += (double)w.dpz;
                acc[8] += (double)x.dpn;   acc[9] += (double)y.dpn;   acc[10] += (double)z.dpn;  acc[11] += (double)w.dpn;
                acc[12] += (double)x.rdpn; acc[13] += (double)y.rdpn; acc[14] += (double)z.rdpn; acc[15] += (double)w.rdpn;
            }
        }
    }

    if (!sums) return;                                              // (uniform over the workgroup)
#pragma unroll
    for (int k = 0; k < 16; k++) s_part[k][tid] = acc[k];
    __syncthreads();
    double* part = a.part + ((int64_t)g * a.chunks + blockIdx.x) * (4 * (int64_t)H);
    for (int o = tid; o < 16 * q; o += kGruGradBlock) {             // o = k q + cc: sum k (which of the four, which unit) of item cc
        const int k = o / q, cc = o - k * q;
        double s = s_part[k][cc];
        for (int pp = 1; pp < P; pp++) s += s_part[k][pp * q + cc];
        part[(k >> 2) * H + 4 * cc + (k & 3)] = s;                  // < 4H: k < 16, cc < q
    }
}

// A wave per column (four columns per workgroup, the group on blockIdx.y): lane t adds the partials of chunks t, t + 64, .. in
// ascending order (a slot past `chunks` adds 0.0, which changes nothing), then the xor butterfly 32 .. 1; one rounding.
__global__ void __launch_bounds__(kGruGradBlock) gru_grad_finish_kernel(GruGradArgs a) {
    const int g = blockIdx.y, C = 4 * a.H, lane = (int)threadIdx.x & 63;
    const int col = (int)blockIdx.x * (kGruGradBlock / 64) + ((int)threadIdx.x >> 6);
    float* out = a.dbias[g];
    if (col >= C || out == nullptr) return;                         // (wave-uniform)
    const double* p = a.part + (int64_t)g * a.chunks * C + col;
    double v[kGruGradMaxChunks / 64];
#pragma unroll
    for (int k = 0; k < kGruGradMaxChunks / 64; k++) {
        const int b = 64 * k + lane;
        v[k] = b < a.chunks ? p[(int64_t)b * C] : 0.0;
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kGruGradMaxChunks / 64; k++) s += v[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) out[col] = (float)s;
}

// the launches of a checked call (mms_host.h: check_gru_gates_grad_group); a.part, a.chunk_rows and a.chunks are set here
hipError_t launch_gru_gates_grad_group(const GruGradArgs& in, int groups, hipStream_t s) {
    if (in.M == 0 || groups == 0) return hipSuccess;
    if (groups < 0 || groups > MMS_MAX_GROUPS || in.M < 0 || in.H < 4 || in.H > kGruMaxH || (in.H & 3)) return hipErrorInvalidValue;
    GruGradArgs a = in;
    a.chunk_rows = gru_grad_chunk_rows(a.M, a.H);
    a.chunks = (int)gru_grad_chunks(a.M, a.H);                      // <= kGruGradMaxChunks
    bool sums = false;
    for (int g = 0; g < groups; g++) sums = sums || a.dbias[g] != nullptr;
    if (!sums) a.part = nullptr;
    hipLaunchKernelGGL(gru_gates_grad_kernel, dim3((unsigned)a.chunks, (unsigned)groups), dim3(kGruGradBlock), 0, s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || !sums) return err;
    hipLaunchKernelGGL(gru_grad_finish_kernel, dim3((unsigned)(a.H), (unsigned)groups), dim3(kGruGradBlock), 0, s, a);      // 4H columns, 4 per workgroup
    return hipGetLastError();
}

}  // namespace mms
