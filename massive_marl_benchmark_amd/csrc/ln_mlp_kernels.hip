// ln_mlp_kernels.hip -- J^T g and J v of the MARL actor's mean (agents/algorithms/utils/mlp.py:6-66 and fc_mean): a LayerNorm on the
// input, L blocks of Linear + ELU + LayerNorm, a Linear head.  The two passes of a Fisher-vector product of HATRPO
// (agents/algorithms/marl/hatrpo_trainer.py:170-179), whose KL is taken between a policy and itself, so that its Hessian is
// J^T diag(1 / (M std^2)) J over the parameters that feed mu.
//
//   u_0 = LN(x; g_0, t_0), a_l = u_{l-1} W_l^T + b_l, h_l = ELU(a_l), u_l = LN(h_l; g_l, t_l) (l = 1..L), mu = u_L W_m^T + b_m
// Saved state: x and h_l.  xhat_l = (h_l - mean) rstd, u_l = g_l xhat_l + t_l and f' = h + 1 (h <= 0) | 1 are re-derived from them; the
// row statistics are recomputed by every call in the two-pass form (mean, then the mean of squared deviations), over the true width.
//
//   grad:  du_L = g W_m;  per level l = L..0:  dg_l = sum_rows du_l xhat_l, dt_l = sum_rows du_l, q = du_l g_l,
//          dh_l = rstd (q - mean(q) - xhat mean(q xhat)), da_l = dh_l f'(h_l);  dW_l = da_l^T u_{l-1}, db_l = sum_rows da_l,
//          du_{l-1} = da_l W_l   (dW_m = g^T u_L, db_m = sum_rows g)
//   jvp:   Ru_0 = G_0 xhat_0 + T_0;  Ra_l = [Ru_{l-1} | u_{l-1}] [W_l | V_l]^T + c_l, Rh_l = f'(h_l) Ra_l,
//          Ru_l = g_l rstd (Rh_l - mean(Rh_l) - xhat_l mean(Rh_l xhat_l)) + G_l xhat_l + T_l;  rmu = [Ru_L | u_L] [W_m | V_m]^T + c_m
//
// The GEMMs, the operand splits and the fixed-order reductions are those of trpo_kernels.hip (mlp_core.h): fp32 operands as three bf16
// planes, fp32 accumulation, weight gradients as row-split partial products summed in a fixed order, bias gradients as per-chunk column
// sums in double.  u_{l-1} is never stored: the operand split evaluates it from h_{l-1}, the row statistics and the affine while it
// reads (operand op 3).  What is new here is ONE row kernel per level and pass (ln_row_kernel): a wave owns a row, takes its two
// statistics, the two means of the LayerNorm backward (or forward-mode) formula and writes the level's output, the row staying in
// the CU's cache between the sweeps; the block then sums its 32 rows' contributions to dg_l and dt_l per column, in row order and in
// double, into a partial that mlp_reduce adds over the blocks in block order.  No atomics anywhere: results are bit-identical run to run.
//
// Launches with L hidden blocks: grad 11 (L + 1) and one memset, jvp 7 (L + 1) + 1; L = 3: 44 and 29, 73 per Fisher-vector product.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ln_mlp_plan.h"
#include "mlp_core.h"

namespace mms {

constexpr int kLnRows = 32;                      // rows of one block of the row kernel (4 waves, 8 rows each)

struct LnRowArgs {
    const float* h;                              // the level's saved activation (x at level 0), [M, K], pitch ldh
    const float* in;                             // jvp: Ra_l (NULL at level 0);  grad: du_l
    const float* gamma;                          // g_l [K]
    const float* dgam;                           // jvp: the direction (G_l, T_l)
    const float* dbet;
    float* out;                                  // jvp: Ru_l (may be `in`);  grad: da_l (NULL at level 0; never `in`)
    float* stat;                                 // [M, 2]: mean, rstd
    float* colp;                                 // grad: [blocks][2][ldc], the block's column sums of du xhat and of du
    int64_t M;
    int ldh, ldin, ldo, ldc, K, grad, elu;       // elu: h is an ELU's output (levels >= 1)
    float eps;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(256) ln_row_kernel(LnRowArgs a) {
    __shared__ float sst[kLnRows][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kLnRows;
    const float inv_k = 1.0f / (float)a.K;
    for (int i = wave; i < kLnRows; i += 4) {
        const int64_t m = r0 + i;
        if (m >= a.M) break;                                            // wave-uniform
        const float* hr = a.h + m * a.ldh;
        float s = 0.f;
        for (int k = lane; k < a.K; k += 64) s += hr[k];
        const float mean = wave_sum(s) * inv_k;
        float v = 0.f;
        for (int k = lane; k < a.K; k += 64) {
            const float d = hr[k] - mean;
            v += d * d;
        }
        const float rstd = 1.0f / sqrtf(wave_sum(v) * inv_k + a.eps);
        if (lane == 0) {
            a.stat[2 * m] = mean;
            a.stat[2 * m + 1] = rstd;
            sst[i][0] = mean;
            sst[i][1] = rstd;
        }
        if (!a.out) continue;                                           // grad, level 0: the affine gradients only
        const float* ir = a.in ? a.in + m * a.ldin : nullptr;
        float* orow = a.out + m * a.ldo;
        float m1 = 0.f, m2 = 0.f;
        if (ir) {                                                       // the two row means of t = Rh (jvp) or q = du g (grad)
            float s1 = 0.f, s2 = 0.f;
            for (int k = lane; k < a.K; k += 64) {
                const float hv = hr[k], xh = (hv - mean) * rstd;
                const float t = a.grad ? ir[k] * a.gamma[k] : ((a.elu && hv <= 0.f) ? hv + 1.f : 1.f) * ir[k];
                s1 += t;
                s2 += t * xh;
            }
            m1 = wave_sum(s1) * inv_k;
            m2 = wave_sum(s2) * inv_k;
        }
        for (int k = lane; k < a.K; k += 64) {
            const float hv = hr[k], xh = (hv - mean) * rstd;
            const float fp = (a.elu && hv <= 0.f) ? hv + 1.f : 1.f;
            float o;
            if (a.grad) {
                o = rstd * (ir[k] * a.gamma[k] - m1 - xh * m2) * fp;
            } else {
                o = a.dgam[k] * xh + a.dbet[k];
                if (ir) o += a.gamma[k] * rstd * (fp * ir[k] - m1 - xh * m2);
            }
            orow[k] = o;
        }
    }
    if (!a.grad) return;
    __syncthreads();
    const int64_t left = a.M - r0;
    const int rows = left < kLnRows ? (int)left : kLnRows;
    float* cp = a.colp + (size_t)blockIdx.x * 2 * a.ldc;
    for (int k = threadIdx.x; k < a.K; k += 256) {
        double sg = 0.0, st = 0.0;
        for (int i = 0; i < rows; i++) {
            const float du = a.in[(r0 + i) * a.ldin + k];
            const float xh = (a.h[(r0 + i) * a.ldh + k] - sst[i][0]) * sst[i][1];
            sg += (double)(du * xh);
            st += (double)du;
        }
        cp[k] = (float)sg;
        cp[a.ldc + k] = (float)st;
    }
}

// rmu [M, A] = src [M, A] (pitch lds) . col_scale [A] (NULL: 1)
__global__ void __launch_bounds__(256) ln_out_kernel(const float* __restrict__ src, int lds, const float* __restrict__ col_scale, int64_t M, int A,
                                                      float* __restrict__ rmu) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= M * A) return;
    const int64_t m = id / A;
    const int j = (int)(id - m * A);
    const float v = src[m * lds + j];
    rmu[id] = col_scale ? v * col_scale[j] : v;
}

static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

bool ln_mlp_plan(int blocks, int64_t M, const int32_t* dims, LnMlpPlan* p) {
    if (blocks < 1 || blocks + 1 > kMlpMaxLayers) return false;
    if (!mlp_plan(blocks + 1, M, dims, false, &p->P)) return false;
    const MlpPlan& P = p->P;
    int npmax = 0;
    for (int l = 0; l <= P.L; l++) npmax = P.np[l] > npmax ? P.np[l] : npmax;
    size_t o = P.total;
    auto take = [&](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
    for (int l = 0; l < P.L; l++) p->stat[l] = take((size_t)P.Mp * 2 * 4);
    p->colp2 = take((size_t)((M + kLnRows - 1) / kLnRows) * 2 * npmax * 4);
    p->d0 = take((size_t)P.Mp * npmax * 4);
    p->d1 = take((size_t)P.Mp * npmax * 4);
    p->total = o;
    return true;
}

static hipError_t ln_rows(const LnRowArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(ln_row_kernel, dim3((unsigned)((a.M + kLnRows - 1) / kLnRows)), dim3(256), 0, s, a);
    return hipGetLastError();
}

#define MMS_TRY(call)                                       \
    do {                                                    \
        if (hipError_t e_ = (call); e_ != hipSuccess) return e_; \
    } while (0)

// Levels l = 0..L (the LayerNorms), Linear layers j = 1..L+1 (layer j reads u_{j-1}; j = L+1 is the mean head): P.n[j] is the width of
// layer j's output, which is level j's width for j <= L.
hipError_t ln_mlp_grad(const LnMlpPlan& Q, float eps, const float* x, const float* const* h, const float* const* ln_g, const float* const* ln_t,
                       const float* const* w, const float* g, float* const* dln_g, float* const* dln_t, float* const* dw, float* const* db,
                       uint8_t* ws, hipStream_t s) {
    const MlpPlan& P = Q.P;
    const int J = P.L;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const float* zb = F(P.zb);
    MMS_TRY(hipMemsetAsync(ws + P.zb, 0, P.cb - P.zb, s));
    const int nblk = (int)((P.M + kLnRows - 1) / kLnRows);
    for (int j = J; j >= 1; j--) {
        const int lv = j - 1;                                           // the level below layer j
        const float* hin = lv == 0 ? x : h[lv - 1];
        const OperandArgs od = j == J ? operand(g, P.n[J]) : operand(F((j & 1) ? Q.d1 : Q.d0), P.np[j]);
        // du_lv = d_j W_j
        MMS_TRY(psplit(od, P.M, P.n[j], P.Mp, P.kc[j], 0, ws + P.xp, s));
        MMS_TRY(tsplit(operand(w[j - 1], P.n[lv]), P.n[j], P.n[lv], P.kc[j], P.kc[j], P.np[lv], P.kc[j], 0, ws + P.wp, nullptr, 0, nullptr, 0, s));
        MMS_TRY(gemm(1, P.Mp, P.np[lv], P.kc[j], ws + P.xp, 0, ws + P.wp, 0, zb, F(P.f0), 0, s));
        // level lv: statistics, dg, dt, da_lv
        LnRowArgs r = {};
        r.h = hin; r.ldh = P.n[lv];
        r.in = F(P.f0); r.ldin = P.np[lv];
        r.gamma = ln_g[lv];
        r.out = lv >= 1 ? F((lv & 1) ? Q.d1 : Q.d0) : nullptr; r.ldo = P.np[lv];
        r.stat = F(Q.stat[lv]);
        r.colp = F(Q.colp2); r.ldc = P.np[lv];
        r.M = P.M; r.K = P.n[lv]; r.grad = 1; r.elu = lv >= 1; r.eps = eps;
        MMS_TRY(ln_rows(r, s));
        MMS_TRY(reduce<double>(F(Q.colp2), nblk, (size_t)2 * P.np[lv], P.np[lv], 1, P.n[lv], dln_g[lv], s));
        MMS_TRY(reduce<double>(F(Q.colp2) + P.np[lv], nblk, (size_t)2 * P.np[lv], P.np[lv], 1, P.n[lv], dln_t[lv], s));
        // dW_j = d_j^T u_lv, db_j = sum_rows d_j
        MMS_TRY(tsplit_rows(P, j, P.S[j], 0, od, true, ws, nullptr, 0, true, s));
        MMS_TRY(tsplit_rows(P, lv, P.S[j], 0, operand_ln(hin, P.n[lv], F(Q.stat[lv]), ln_g[lv], ln_t[lv]), false, ws, nullptr, 0, false, s));
        MMS_TRY(weight_grad(P, j, 1, ws, dw[j - 1], db[j - 1], s));
    }
    return hipSuccess;
}

hipError_t ln_mlp_jvp(const LnMlpPlan& Q, float eps, const float* x, const float* const* h, const float* const* ln_g, const float* const* ln_t,
                      const float* const* w, const float* const* vg, const float* const* vt, const float* const* vw, const float* const* vc,
                      const float* col_scale, float* rmu, uint8_t* ws, hipStream_t s) {
    const MlpPlan& P = Q.P;
    const int J = P.L;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    float* cur = F(P.f0);                                               // Ru of the level below, pitch np
    float* nxt = F(P.f1);
    for (int lv = 0; lv <= J; lv++) {
        if (lv >= 1) {                                                  // Ra_lv = [Ru_{lv-1} | u_{lv-1}] [W | V]^T + c  (into nxt)
            const int K = P.n[lv - 1], kc = P.kc[lv - 1];
            const float* hin = lv == 1 ? x : h[lv - 2];
            MMS_TRY(copy2d(vc[lv - 1], 1, P.n[lv], P.n[lv], F(P.cb), 1, P.np[lv], P.np[lv], s));
            MMS_TRY(psplit(operand(cur, P.np[lv - 1]), P.M, K, P.Mp, 2 * kc, 0, ws + P.xp, s));
            MMS_TRY(psplit(operand_ln(hin, K, F(Q.stat[lv - 1]), ln_g[lv - 1], ln_t[lv - 1]), P.M, K, P.Mp, 2 * kc, kc, ws + P.xp, s));
            MMS_TRY(psplit(operand(w[lv - 1], K), P.n[lv], K, P.np[lv], 2 * kc, 0, ws + P.wp, s));
            MMS_TRY(psplit(operand(vw[lv - 1], K), P.n[lv], K, P.np[lv], 2 * kc, kc, ws + P.wp, s));
            MMS_TRY(gemm(1, P.Mp, P.np[lv], 2 * kc, ws + P.xp, 0, ws + P.wp, 0, F(P.cb), nxt, 0, s));
            float* t = cur; cur = nxt; nxt = t;
        }
        if (lv == J) break;                                             // the mean head has no LayerNorm behind it
        LnRowArgs r = {};
        r.h = lv == 0 ? x : h[lv - 1]; r.ldh = P.n[lv];
        r.in = lv == 0 ? nullptr : cur; r.ldin = P.np[lv];
        r.gamma = ln_g[lv]; r.dgam = vg[lv]; r.dbet = vt[lv];
        r.out = cur; r.ldo = P.np[lv];
        r.stat = F(Q.stat[lv]);
        r.M = P.M; r.K = P.n[lv]; r.grad = 0; r.elu = lv >= 1; r.eps = eps;
        MMS_TRY(ln_rows(r, s));
    }
    const int64_t n = P.M * P.n[J];
    hipLaunchKernelGGL(ln_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cur, P.np[J], col_scale, P.M, P.n[J], rmu);
    return hipGetLastError();
}

#undef MMS_TRY

}  // namespace mms
