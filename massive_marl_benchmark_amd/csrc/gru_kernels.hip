// gru_kernels.hip -- one GRU cell step for up to MMS_MAX_GROUPS networks per launch (mms_gru_group, include/mms.h): the recurrent
// layer of the reference's MARL actors and critics (agents/algorithms/utils/rnn.py:7-80: nn.GRU on hxs * masks), which the reference
// runs agent by agent as two library products, two bias adds and a chain of gate kernels over [M, 3H] pre-activations.
//
// Both products are dense contractions, so they run on v_mfma_f32_32x32x2_f32 (exact fp32 products and sums; the networks are fp32),
// with the tiling of policy_kernels.hip's linear_act_kernel: 256 threads, operand tiles row-major in LDS at pitch 36, k-slices of 32,
// double buffered, one barrier per slice.  What differs is what a workgroup owns: 128 rows x 32 hidden units j, and for those units
// ALL THREE gates -- the weight tile of a slice is the rows {j, H + j, 2H + j} of w_ih (96 rows) -- so the gate arithmetic runs in the
// epilogue on accumulators and the [M, 3H] pre-activations never go to memory.  Two k-phases through the same pipeline: over x with
// w_ih, then over hm = mask * h with w_hh (the mask is applied while h is staged, so the product sees hm as torch's does).  Four
// accumulator sets per wave (32 rows x 32 units each, 64 registers): r and z summed across both phases, n's two halves kept apart
// because r multiplies the second (gru_lane.h); three more sets hold the sums of the slice at hand (multiply_slice).  LDS 2 x (128 + 96) x 36 x 4 B = 64.5 KB: two workgroups per CU.
// The order of every sum over k is a function of K and H alone and there are no atomics: row i's result depends on row i and network
// g's parameters only.  Built like param_step_kernels.hip (csrc/Makefile: PARAM_FLAGS): no fast-math, -ffp-contract=off, so the
// epilogue rounds every operation as the CPU build's evaluation of gru_lane.h does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gru_args.h"
#include "gru_lane.h"

namespace mms {

typedef float gru_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kGruTM = 128, kGruTU = 32, kGruBK = 32, kGruPitch = kGruBK + 4;
constexpr int kGruWRows = 3 * kGruTU;                                               // weight rows per slice: three gates of 32 units
constexpr size_t kGruLds = (size_t)2 * (kGruTM + kGruWRows) * kGruPitch * sizeof(float);

__global__ void __launch_bounds__(256, 2) gru_group_kernel(GruArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int g = blockIdx.z;
    const float* __restrict__ X = a.x[g];
    const float* __restrict__ Hs = a.h[g];
    const float* __restrict__ Mk = a.mask[g];
    const float* __restrict__ Wih = a.w_ih[g];
    const float* __restrict__ Whh = a.w_hh[g];
    const int M = a.M, K = a.K, H = a.H;
    const int m0 = blockIdx.x * kGruTM, u0 = blockIdx.y * kGruTU;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int li = lane & 31, lh = lane >> 5;
    float* As = smem;                                       // [2][128][kGruPitch]
    float* Bs = smem + 2 * kGruTM * kGruPitch;              // [2][96][kGruPitch]: gate q's unit u at row 32 q + u
    // staging: 128 + 96 rows x 8 float4 per slice: thread t takes k offset sk of rows sr + 32 j (j < 4) and of unit sr of each gate
    const int sr = t >> 3, sk = (t & 7) * 4;
    const bool unit_ok = u0 + sr < H;

    // (named scalars below: arrays of float4 that lambdas capture land in scratch)
#define MMS_GRU_ROW(j) (m0 + sr + 32 * (j))
#define MMS_GRU_MASK(j) ((Mk && MMS_GRU_ROW(j) < M) ? Mk[(int64_t)MMS_GRU_ROW(j) * a.mask_pitch] : 1.f)
    const float mrow0 = MMS_GRU_MASK(0), mrow1 = MMS_GRU_MASK(1), mrow2 = MMS_GRU_MASK(2), mrow3 = MMS_GRU_MASK(3);   // the mask of this thread's staging rows
#undef MMS_GRU_MASK

    const int nkx = (K + kGruBK - 1) / kGruBK, nkh = (H + kGruBK - 1) / kGruBK, nk = nkx + nkh;
    float4 ra0, ra1, ra2, ra3, rb0, rb1, rb2;
#define MMS_GRU_ZERO4 make_float4(0.f, 0.f, 0.f, 0.f)
    auto load_slice = [&](int s) {                          // slices 0 .. nkx - 1: x and w_ih; nkx .. nk - 1: hm and w_hh
        const bool ph = s >= nkx;
        const int k = (ph ? s - nkx : s) * kGruBK + sk;     // K % 4 == 0 and H % 4 == 0: k < KK implies k + 3 < KK
        const int KK = ph ? H : K;
        const float* src = ph ? Hs : X;
        const int64_t sp = ph ? a.h_pitch : a.x_pitch;
        const float* W = ph ? Whh : Wih;
        const bool masked = ph && Mk;
#define MMS_GRU_LDA(j)                                                                                                                   \
    {                                                                                                                                    \
        float4 v = (MMS_GRU_ROW(j) < M && k < KK) ? *reinterpret_cast<const float4*>(src + (int64_t)MMS_GRU_ROW(j) * sp + k) : MMS_GRU_ZERO4;    \
        if (masked) { v.x = gru_masked(mrow##j, v.x); v.y = gru_masked(mrow##j, v.y); v.z = gru_masked(mrow##j, v.z); v.w = gru_masked(mrow##j, v.w); } \
        ra##j = v;                                                                                                                       \
    }
#define MMS_GRU_LDB(q) rb##q = (unit_ok && k < KK) ? *reinterpret_cast<const float4*>(W + ((int64_t)(q) * H + u0 + sr) * KK + k) : MMS_GRU_ZERO4;
        MMS_GRU_LDA(0) MMS_GRU_LDA(1) MMS_GRU_LDA(2) MMS_GRU_LDA(3)
        MMS_GRU_LDB(0) MMS_GRU_LDB(1) MMS_GRU_LDB(2)
#undef MMS_GRU_LDA
#undef MMS_GRU_LDB
    };
    auto store_slice = [&](int buf) {
#define MMS_GRU_STA(j) *reinterpret_cast<float4*>(As + ((size_t)buf * kGruTM + sr + 32 * (j)) * kGruPitch + sk) = ra##j;
#define MMS_GRU_STB(q) *reinterpret_cast<float4*>(Bs + ((size_t)buf * kGruWRows + 32 * (q) + sr) * kGruPitch + sk) = rb##q;
        MMS_GRU_STA(0) MMS_GRU_STA(1) MMS_GRU_STA(2) MMS_GRU_STA(3)
        MMS_GRU_STB(0) MMS_GRU_STB(1) MMS_GRU_STB(2)
#undef MMS_GRU_STA
#undef MMS_GRU_STB
    };
#undef MMS_GRU_ROW
#undef MMS_GRU_ZERO4

    gru_f32x16 acc_r, acc_z, acc_ni, acc_nh;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc_r[r] = 0.f; acc_z[r] = 0.f; acc_ni[r] = 0.f; acc_nh[r] = 0.f; }

    // lane (i, h) supplies k = 8 c + 4 h .. + 3 of its row to four consecutive MFMAs, from both operands alike (policy_kernels.hip).
    // Blocked summation: a slice's 32 k are summed from zero (16 chained MFMAs) and the slice's sum is added to the running one, so an
    // output sees 16 + (K + H) / 32 roundings of partial sums instead of (K + H) / 2 -- at K = H = 512 a quarter of the chained
    // form's error for 48 VALU additions next to 48 MFMAs of 16 passes each.
    auto multiply_slice = [&](int buf, gru_f32x16& acc_n) {
        const float* a_base = As + ((size_t)buf * kGruTM + 32 * wave + li) * kGruPitch + 4 * lh;
        const float* b_base = Bs + ((size_t)buf * kGruWRows + li) * kGruPitch + 4 * lh;
        gru_f32x16 tr = {}, tz = {}, tn = {};
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float4 af = *reinterpret_cast<const float4*>(a_base + 8 * c);
            const float4 br = *reinterpret_cast<const float4*>(b_base + 8 * c);
            const float4 bz = *reinterpret_cast<const float4*>(b_base + 32 * kGruPitch + 8 * c);
            const float4 bn = *reinterpret_cast<const float4*>(b_base + 64 * kGruPitch + 8 * c);
#define MMS_GRU_STEP(e)                                                        \
    tr = __builtin_amdgcn_mfma_f32_32x32x2f32(af.e, br.e, tr, 0, 0, 0);        \
    tz = __builtin_amdgcn_mfma_f32_32x32x2f32(af.e, bz.e, tz, 0, 0, 0);        \
    tn = __builtin_amdgcn_mfma_f32_32x32x2f32(af.e, bn.e, tn, 0, 0, 0);
            MMS_GRU_STEP(x) MMS_GRU_STEP(y) MMS_GRU_STEP(z) MMS_GRU_STEP(w)
#undef MMS_GRU_STEP
        }
        acc_r += tr;
        acc_z += tz;
        acc_n += tn;
    };

    // slice s is multiplied out of buffer s & 1 while slice s + 1 is in flight into registers; it is stored into the other buffer,
    // which every wave left at the barrier of slice s - 1
    load_slice(0);
    store_slice(0);
    __syncthreads();
    for (int s = 0; s < nkx; s++) {
        if (s + 1 < nk) load_slice(s + 1);
        multiply_slice(s & 1, acc_ni);
        if (s + 1 < nk) store_slice((s + 1) & 1);
        __syncthreads();
    }
    for (int s = nkx; s < nk; s++) {
        if (s + 1 < nk) load_slice(s + 1);
        multiply_slice(s & 1, acc_nh);
        if (s + 1 < nk) store_slice((s + 1) & 1);
        __syncthreads();
    }

    // epilogue.  C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int col = u0 + li;
    if (col >= H) return;
    const float* __restrict__ bi = a.b_ih[g];
    const float* __restrict__ bh = a.b_hh[g];
    const float bi_r = bi[col], bi_z = bi[H + col], bi_n = bi[2 * H + col];
    const float bh_r = bh[col], bh_z = bh[H + col], bh_n = bh[2 * H + col];
    float* __restrict__ Ho = a.h_out[g];
    float* __restrict__ Y = a.y[g];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row < M) {
            float hm = Hs[(int64_t)row * a.h_pitch + col];
            if (Mk) hm = gru_masked(Mk[(int64_t)row * a.mask_pitch], hm);
            const float o = gru_cell(acc_r[r], acc_z[r], acc_ni[r], acc_nh[r], bi_r, bi_z, bi_n, bh_r, bh_z, bh_n, hm);
            Ho[(int64_t)row * a.h_out_pitch + col] = o;
            if (Y) Y[(int64_t)row * H + col] = o;
        }
    }
}

// the launch of a checked call (mms_host.h: check_gru_group)
hipError_t launch_gru_group(const GruArgs& a, int groups, hipStream_t s) {
    if (a.M == 0 || groups == 0) return hipSuccess;
    if (groups < 0 || groups > MMS_MAX_GROUPS || a.M < 0 || a.H < 4 || a.H > kGruMaxH || (a.H & 3) || a.K < 4 || (a.K & 3)) return hipErrorInvalidValue;
    static bool done[64] = {};                              // more than 64 KB of LDS per workgroup is an opt-in per device
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !done[dev]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(gru_group_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGruLds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) done[dev] = true;
    }
    const dim3 grid((unsigned)((a.M + kGruTM - 1) / kGruTM), (unsigned)((a.H + kGruTU - 1) / kGruTU), (unsigned)groups);
    hipLaunchKernelGGL(gru_group_kernel, grid, dim3(256), kGruLds, s, a);
    return hipGetLastError();
}

}  // namespace mms
