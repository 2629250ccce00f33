// gru_gates_kernels.hip -- the gate arithmetic of one GRU cell step for up to MMS_MAX_GROUPS networks per launch, on pre-activations
// that two layer launches left in memory (mms_gru_gates_group, include/mms.h): gi = x W_ih^T + b_ih and gh = h W_hh^T, [M, 3H] f32 each.
// It is the unfused counterpart of gru_kernels.hip's epilogue: there the products stay in accumulators of the exact-fp32 MFMA kernel,
// here they come from mms_linear_group_act_split16 (two fp16 planes per operand), which GroupedPolicyInference's rnn_format="f16x2"
// route runs instead.  The mask multiplies gh and h (gru_lane.h: gru_gates), which is the reference's nn.GRU on hxs * masks
// (agents/algorithms/utils/rnn.py:25-29) because a per-row mask commutes with the product.
//
// A streaming kernel: no LDS, no atomics, nothing to reduce.  One item = four consecutive hidden units j .. j + 3 of one row: ten 16-byte
// loads (r, z, n of gi and of gh, h, three of b_hh -- the bias vectors stay in L2) and one or two 16-byte stores, so that a wave's
// instruction moves 1 KiB of consecutive addresses wherever H / 4 >= 64.  Workgroups of 256 threads with the group on blockIdx.y; the
// grid over items is capped at 2048 workgroups (eight per CU) and strides over the rest, the items of a thread advancing by a constant
// (rows, columns) step so that the loop holds no division.  Row i's result is a function of row i and the group's bias alone.
// Built like gru_kernels.hip (csrc/Makefile: PARAM_FLAGS): accurate expf / tanhf, IEEE division, -ffp-contract=off, so every operation
// rounds as the CPU build's evaluation of gru_lane.h does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gru_gates_args.h"
#include "gru_lane.h"

namespace mms {

constexpr int kGatesBlock = 256, kGatesMaxBlocks = 2048;

__global__ void __launch_bounds__(kGatesBlock) gru_gates_group_kernel(GruGatesArgs a) {
    const int g = blockIdx.y;
    const float* __restrict__ Gi = a.gi[g];
    const float* __restrict__ Gh = a.gh[g];
    const float* __restrict__ Hs = a.h[g];
    const float* __restrict__ Mk = a.mask[g];
    const float* __restrict__ Bh = a.b_hh[g];
    float* __restrict__ Ho = a.h_out[g];
    float* __restrict__ Y = a.y[g];
    const int H = a.H, q = H >> 2;                                  // q items per row
    const int64_t M = a.M;
    // item = row * q + col; the first one and the stride both fit 32 bits (at most 2048 x 256 threads per group)
    const unsigned first = blockIdx.x * kGatesBlock + threadIdx.x, stride = gridDim.x * kGatesBlock;
    int64_t row = first / (unsigned)q;
    int col = (int)(first % (unsigned)q);
    const int drow = (int)(stride / (unsigned)q), dcol = (int)(stride % (unsigned)q);
    const bool masked = Mk != nullptr;
    for (; row < M; row += drow) {
        const int j = 4 * col;                                      // j + 3 < H: col < q
        const float* gi = Gi + row * a.g_pitch + j;
        const float* gh = Gh + row * a.g_pitch + j;
        const float4 ir = *reinterpret_cast<const float4*>(gi), iz = *reinterpret_cast<const float4*>(gi + H), in = *reinterpret_cast<const float4*>(gi + 2 * H);
        const float4 hr = *reinterpret_cast<const float4*>(gh), hz = *reinterpret_cast<const float4*>(gh + H), hn = *reinterpret_cast<const float4*>(gh + 2 * H);
        const float4 hv = *reinterpret_cast<const float4*>(Hs + row * a.h_pitch + j);
        const float4 br = *reinterpret_cast<const float4*>(Bh + j), bz = *reinterpret_cast<const float4*>(Bh + H + j), bn = *reinterpret_cast<const float4*>(Bh + 2 * H + j);
        const float m = masked ? Mk[row * a.mask_pitch] : 1.f;
        float4 o;
        o.x = gru_gates(masked, m, ir.x, iz.x, in.x, hr.x, hz.x, hn.x, br.x, bz.x, bn.x, hv.x);
        o.y = gru_gates(masked, m, ir.y, iz.y, in.y, hr.y, hz.y, hn.y, br.y, bz.y, bn.y, hv.y);
        o.z = gru_gates(masked, m, ir.z, iz.z, in.z, hr.z, hz.z, hn.z, br.z, bz.z, bn.z, hv.z);
        o.w = gru_gates(masked, m, ir.w, iz.w, in.w, hr.w, hz.w, hn.w, br.w, bz.w, bn.w, hv.w);
        *reinterpret_cast<float4*>(Ho + row * a.h_out_pitch + j) = o;
        if (Y) *reinterpret_cast<float4*>(Y + row * H + j) = o;
        col += dcol;
        if (col >= q) { col -= q; row++; }
    }
}

// the launch of a checked call (mms_host.h: check_gru_gates_group)
hipError_t launch_gru_gates_group(const GruGatesArgs& a, int groups, hipStream_t s) {
    if (a.M == 0 || groups == 0) return hipSuccess;
    if (groups < 0 || groups > MMS_MAX_GROUPS || a.M < 0 || a.H < 4 || a.H > kGruMaxH || (a.H & 3)) return hipErrorInvalidValue;
    const int64_t items = (int64_t)a.M * (a.H >> 2);
    const int64_t blocks = (items + kGatesBlock - 1) / kGatesBlock;
    const dim3 grid((unsigned)(blocks < kGatesMaxBlocks ? blocks : kGatesMaxBlocks), (unsigned)groups);
    hipLaunchKernelGGL(gru_gates_group_kernel, grid, dim3(kGatesBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace mms
