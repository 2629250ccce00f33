// trpo_kernels.hip -- first- and second-order backward passes of an L-layer ELU MLP with an identity output, for the curvature
// products of TRPO (agents/algorithms/rl/trpo/trpo.py:290, :417-435).
//
// Layers l = 1..L: a_l = h_{l-1} W_l^T + b_l, h_l = ELU(a_l) (l < L), mu = a_L; h_0 = x.  With f'(a) = f''(a) = h + 1 where h <= 0,
// f' = 1 and f'' = 0 where h > 0, everything below reads h_l and never a_l.
//   backward (mlp_grad):      d_L = g, dW_l = d_l^T h_{l-1}, db_l = sum_m d_l, e_{l-1} = d_l W_l, d_{l-1} = e_{l-1} . f'(h_{l-1})
//   R-op (mlp_grad_rop), direction (V_l, c_l), g held fixed (Pearlmutter):
//     Ra_l = Rh_{l-1} W_l^T + h_{l-1} V_l^T + c_l, Rh_l = f'(h_l) . Ra_l, Rh_0 = 0;  R{mu} = Ra_L
//     Rd_L = 0, RdW_l = Rd_l^T h_{l-1} + d_l^T Rh_{l-1}, Rdb_l = sum_m Rd_l,
//     Rd_{l-1} = (Rd_l W_l + d_l V_l) . f'(h_{l-1}) + e_{l-1} . f''(h_{l-1}) . Ra_{l-1}
//
// Every product runs on ONE GEMM core: the split-operand layer of split_kernels.hip (fp32 operands as three bf16 planes, format P32,
// six bf16 MFMA products accumulated in fp32), which computes Y = X W^T.  The three orientations are reduced to that form here:
//   X W^T  (R-forward):            planes of X and of W as they are;
//   D W    (e, Rd: contraction over the layer's outputs): planes of D and of W^T (the transposing split below);
//   D^T X  (weight gradients: contraction over the rows): planes of D^T and of X^T, the rows cut into S parts that run as S groups
//          of one launch (the output has few tiles: 1024 x 1024 is 64 of them), summed afterwards in a fixed order (mlp_reduce):
//          no atomics, so a product is bit-identical from run to run.
// Sums of two products are concatenated along k in plane space (X W^T: one buffer of KC1 + KC2 chunks, one accumulator), or, for the
// weight gradients, run as 2 S groups into the same reduction.  The elementwise factors (. f', the f'' term) are applied by the split
// kernels while they read the fp32 operand, so the GEMM epilogue stays the plain store.  Every dimension is zero-padded to what the
// core takes (rows and output columns multiples of 128, k multiples of 32).  Workspace comes from the caller (mlp_plan sizes it).
// The operand forms and the launchers below are declared in mlp_core.h: ln_mlp_kernels.hip builds its two passes from them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "policy_args.h"
#include "trpo_plan.h"
#include "mlp_core.h"

namespace mms {

hipError_t launch_linear_split(const SplitLinearArgs& a, int groups, hipStream_t s);

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float operand_at(const OperandArgs& o, int64_t m, int k) {
    float v = o.x[m * o.ldx + k];
    if (o.op == 3) return (v - o.st[2 * m]) * o.st[2 * m + 1] * o.ga[k] + o.be[k];
    if (o.op >= 1) {
        const float hv = o.h[m * o.ldh + k];
        const float fp = hv > 0.f ? 1.f : hv + 1.f;
        v = v * fp;
        if (o.op == 2) {
            const float fpp = hv > 0.f ? 0.f : hv + 1.f;
            v = v + o.e[m * o.lde + k] * fpp * o.r[m * o.ldr + k];
        }
    }
    return v;
}

__device__ __forceinline__ void store_planes(uint8_t* dst, const float (&v)[8]) {
    bf16x8 p0, p1, p2;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        float r = v[j];
        p0[j] = (__bf16)r; r -= (float)p0[j];
        p1[j] = (__bf16)r; r -= (float)p1[j];
        p2[j] = (__bf16)r;
    }
    *reinterpret_cast<bf16x8*>(dst) = p0;
    *reinterpret_cast<bf16x8*>(dst + 64) = p1;
    *reinterpret_cast<bf16x8*>(dst + 128) = p2;
}

// ---- A [rows, K] -> P32 planes of A, rows padded to rows_pad, into chunks [coff, coff + KC) of rows of `pitch` chunks -------------
struct PlainSplitArgs {
    OperandArgs o;
    int rows, K, rows_pad, KC, pitch, coff;
    uint8_t* dst;
};

__global__ void __launch_bounds__(256) mlp_split_kernel(PlainSplitArgs a) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int g = (int)(id & 3);
    const int64_t rc = id >> 2;
    const int kc = (int)(rc % a.KC);
    const int64_t row = rc / a.KC;
    if (row >= a.rows_pad) return;
    const int k0 = kc * 32 + g * 8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = (row < a.rows && k0 + j < a.K) ? operand_at(a.o, row, k0 + j) : 0.f;
    store_planes(a.dst + ((size_t)row * a.pitch + a.coff + kc) * kChunk + g * 16, v);
}

// ---- A [rows, cols] -> P32 planes of A^T: `cols` rows (padded to rows_pad) whose k runs over A's rows ------------------------------
// Block = 32 source rows (one chunk mc) x 64 source columns, through LDS.  Chunk mc goes to part p = mc / MCs, local chunk mc % MCs,
// of a buffer of parts [parts][rows_pad][pitch] chunks (coff = first chunk of this operand in a k-concatenation).  Optional: the
// evaluated operand in fp32 (out [rows, cols], pitch ldo) and per-chunk column sums colp[mc][ldc] (a bias gradient's first stage).
struct TransSplitArgs {
    OperandArgs o;
    int rows, cols, MCs, rows_pad, pitch, coff;
    uint8_t* dst;
    float* out;
    int ldo;
    float* colp;
    int ldc;
};

__global__ void __launch_bounds__(256) mlp_tsplit_kernel(TransSplitArgs a) {
    __shared__ float tile[32][65];
    const int t = threadIdx.x, c = t & 63, r0 = t >> 6;
    const int k = blockIdx.x * 64 + c, mc = blockIdx.y;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int r = r0 + 4 * i;
        const int64_t m = (int64_t)mc * 32 + r;
        const bool in = m < a.rows && k < a.cols;
        const float v = in ? operand_at(a.o, m, k) : 0.f;
        tile[r][c] = v;
        if (a.out && in) a.out[m * a.ldo + k] = v;
    }
    __syncthreads();
    if (a.colp && t < 64) {                       // summed in double, rounded once: a serial fp32 sum over the rows is worse than a tree's
        double s = 0.0;
        for (int r = 0; r < 32; r++) s += (double)tile[r][t];
        a.colp[(size_t)mc * a.ldc + blockIdx.x * 64 + t] = (float)s;
    }
    const int n = t >> 2, g = t & 3, row = blockIdx.x * 64 + n;
    const int p = mc / a.MCs, j = mc - p * a.MCs;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = tile[g * 8 + i][n];
    store_planes(a.dst + (((size_t)p * a.rows_pad + row) * a.pitch + a.coff + j) * kChunk + g * 16, v);
}

// out[n, k] = sum over g (in order) of part[g][n, k]  (part rows of ldp floats, `stride` floats apart), accumulated in Acc: float for
// the few row parts of a weight gradient, double for a bias gradient's column sums (one per 32-row chunk: up to 65535 of them)
template <typename Acc>
__global__ void __launch_bounds__(256) mlp_reduce_kernel(const float* __restrict__ part, int groups, size_t stride, int ldp, int N, int K,
                                                          float* __restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)N * K) return;
    const int n = (int)(id / K), k = (int)(id - (int64_t)n * K);
    const float* p = part + (size_t)n * ldp + k;
    Acc s = 0;
    for (int g = 0; g < groups; g++) s += (Acc)p[g * stride];
    out[id] = (float)s;
}

// dst [rd, cd] (pitch ldd) = src [rs, cs] (pitch lds), zero outside
__global__ void __launch_bounds__(256) mlp_copy_kernel(const float* __restrict__ src, int64_t rs, int cs, int lds, float* __restrict__ dst,
                                                        int64_t rd, int cd, int ldd) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= rd * cd) return;
    const int64_t i = id / cd;
    const int j = (int)(id - i * cd);
    dst[i * ldd + j] = (i < rs && j < cs) ? src[i * lds + j] : 0.f;
}

// ---- plan: padded shapes and workspace layout ------------------------------------------------------------------------------------
static inline int r128(int64_t v) { return (int)((v + 127) / 128 * 128); }
static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

bool mlp_plan(int L, int64_t M, const int32_t* dims, bool rop, MlpPlan* p) {
    if (L < 2 || L > kMlpMaxLayers || M <= 0 || M > kMlpMaxRows) return false;
    p->L = L;
    p->M = M;
    p->Mp = r128(M);
    p->MC = (int)(p->Mp / 32);
    if (p->MC > 65535) return false;                  // the transposing split's grid y walks the 32-row chunks (at most 65535)
    int npmax = 0, kcmax = 0;
    for (int l = 0; l <= L; l++) {
        if (dims[l] <= 0 || dims[l] > 65536) return false;
        p->n[l] = dims[l];
        p->np[l] = r128(dims[l]);
        p->kc[l] = (dims[l] + 31) / 32;
        npmax = p->np[l] > npmax ? p->np[l] : npmax;
        kcmax = p->kc[l] > kcmax ? p->kc[l] : kcmax;
    }
    size_t partmax = 0;
    for (int l = 1; l <= L; l++) {
        // rows split into S parts so that the weight gradient's launch has about one 128 x 128 tile per CU (2 S <= the group limit)
        const int64_t tiles = (int64_t)(p->np[l] / 128) * (p->np[l - 1] / 128);
        int S = 1;
        while (S < kMaxGroups / 2 && tiles * S < 256 && p->MC % (2 * S) == 0) S *= 2;
        p->S[l] = S;
        const size_t b = (size_t)2 * S * p->np[l] * p->np[l - 1] * 4;
        partmax = b > partmax ? b : partmax;
    }
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
    p->zb = take((size_t)npmax * 4);
    p->cb = take((size_t)npmax * 4);
    p->ta = take((size_t)2 * npmax * p->MC * kChunk);
    p->tb = take((size_t)2 * npmax * p->MC * kChunk);
    p->part = take(partmax);
    p->colp = take((size_t)p->MC * npmax * 4);
    p->xp = take((size_t)p->Mp * 2 * kcmax * kChunk);
    p->wp = take((size_t)npmax * 2 * kcmax * kChunk);
    p->f0 = take((size_t)p->Mp * npmax * 4);
    p->f1 = take((size_t)p->Mp * npmax * 4);
    for (int l = 0; l <= L; l++) p->ra[l] = (rop && l >= 1) ? take((size_t)p->Mp * p->np[l] * 4) : 0;
    p->total = o;
    return true;
}

hipError_t psplit(const OperandArgs& o, int64_t rows, int K, int64_t rows_pad, int pitch, int coff, uint8_t* dst, hipStream_t s) {
    PlainSplitArgs a = {o, (int)rows, K, (int)rows_pad, (K + 31) / 32, pitch, coff, dst};
    const int64_t threads = rows_pad * a.KC * 4;
    hipLaunchKernelGGL(mlp_split_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// A [rows, cols] -> planes of A^T; MC = chunks over A's rows (all parts), MCs per part
hipError_t tsplit(const OperandArgs& o, int64_t rows, int cols, int MC, int MCs, int rows_pad, int pitch, int coff, uint8_t* dst,
                  float* out, int ldo, float* colp, int ldc, hipStream_t s) {
    TransSplitArgs a = {o, (int)rows, cols, MCs, rows_pad, pitch, coff, dst, out, ldo, colp, ldc};
    hipLaunchKernelGGL(mlp_tsplit_kernel, dim3((unsigned)(rows_pad / 64), (unsigned)MC), dim3(256), 0, s, a);
    return hipGetLastError();
}

// y_g = x_g w_g^T (+ b), g < groups, operands in planes (groups consecutive in memory at the given strides)
hipError_t gemm(int groups, int64_t M, int N, int KC, const uint8_t* x, size_t xs, const uint8_t* w, size_t ws, const float* b, float* y,
                size_t ys, hipStream_t s) {
    SplitLinearArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.x[g] = x + g * xs;
        a.w[g] = w + g * ws;
        a.b[g] = b;
        a.y[g] = y + g * ys;
    }
    a.M = (int)M;
    a.N = N;
    a.KC = KC;
    a.act = 0;
    a.out_mode = 0;
    return launch_linear_split(a, groups, s);
}

hipError_t copy2d(const float* src, int64_t rs, int cs, int lds, float* dst, int64_t rd, int cd, int ldd, hipStream_t s) {
    const int64_t n = rd * cd;
    hipLaunchKernelGGL(mlp_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, rs, cs, lds, dst, rd, cd, ldd);
    return hipGetLastError();
}

template <typename Acc>
hipError_t reduce(const float* part, int groups, size_t stride, int ldp, int N, int K, float* out, hipStream_t s) {
    const int64_t n = (int64_t)N * K;
    hipLaunchKernelGGL(mlp_reduce_kernel<Acc>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, groups, stride, ldp, N, K, out);
    return hipGetLastError();
}

template hipError_t reduce<float>(const float*, int, size_t, int, int, int, float*, hipStream_t);
template hipError_t reduce<double>(const float*, int, size_t, int, int, int, float*, hipStream_t);

#define MMS_TRY(call)                                       \
    do {                                                    \
        if (hipError_t e_ = (call); e_ != hipSuccess) return e_; \
    } while (0)

// dW_l (and db_l) of one layer from the transposed planes already in ta (S parts per product, `prods` products) and tb
hipError_t weight_grad(const MlpPlan& P, int l, int prods, uint8_t* ws, float* dw, float* db, hipStream_t s) {
    const int S = P.S[l], MCs = P.MC / S, G = prods * S;
    const size_t xs = (size_t)P.np[l] * MCs * kChunk, wsz = (size_t)P.np[l - 1] * MCs * kChunk, ys = (size_t)P.np[l] * P.np[l - 1];
    float* part = reinterpret_cast<float*>(ws + P.part);
    MMS_TRY(gemm(G, P.np[l], P.np[l - 1], MCs, ws + P.ta, xs, ws + P.tb, wsz, reinterpret_cast<const float*>(ws + P.zb), part, ys, s));
    MMS_TRY(reduce<float>(part, G, ys, P.np[l - 1], P.n[l], P.n[l - 1], dw, s));
    if (db) MMS_TRY(reduce<double>(reinterpret_cast<const float*>(ws + P.colp), P.MC, (size_t)P.np[l], P.np[l], 1, P.n[l], db, s));
    return hipSuccess;
}

// tsplit into product q's S parts of ta / tb for layer l (contraction over the M rows)
hipError_t tsplit_rows(const MlpPlan& P, int l_rows, int S, int q, const OperandArgs& o, bool into_a, uint8_t* ws, float* out, int ldo,
                       bool colsum, hipStream_t s) {
    const int cols = P.n[l_rows], rows_pad = P.np[l_rows], MCs = P.MC / S;
    uint8_t* dst = ws + (into_a ? P.ta : P.tb) + (size_t)q * S * rows_pad * MCs * kChunk;
    return tsplit(o, P.M, cols, P.MC, MCs, rows_pad, MCs, 0, dst, out, ldo, colsum ? reinterpret_cast<float*>(ws + P.colp) : nullptr, rows_pad, s);
}

hipError_t mlp_grad(const MlpPlan& P, const float* x, const float* const* h, const float* const* w, const float* g, float* const* dw,
                    float* const* db, float* const* d_out, float* const* e_out, uint8_t* ws, hipStream_t s) {
    const int L = P.L;
    MMS_TRY(hipMemsetAsync(ws + P.zb, 0, P.cb - P.zb, s));
    const float* e_cur = nullptr;
    int lde = 0;
    for (int l = L; l >= 1; l--) {
        const float* hin = l == 1 ? x : h[l - 2];
        const OperandArgs od = l == L ? operand(g, P.n[L]) : operand(e_cur, lde, 1, h[l - 1], P.n[l]);
        float* dsave = (l < L && d_out) ? d_out[l - 1] : nullptr;
        MMS_TRY(tsplit_rows(P, l, P.S[l], 0, od, true, ws, dsave, P.n[l], true, s));
        MMS_TRY(tsplit_rows(P, l - 1, P.S[l], 0, operand(hin, P.n[l - 1]), false, ws, nullptr, 0, false, s));
        MMS_TRY(weight_grad(P, l, 1, ws, dw[l - 1], db[l - 1], s));
        if (l > 1) {                                                    // e_{l-1} = d_l W_l
            MMS_TRY(psplit(od, P.M, P.n[l], P.Mp, P.kc[l], 0, ws + P.xp, s));
            MMS_TRY(tsplit(operand(w[l - 1], P.n[l - 1]), P.n[l], P.n[l - 1], P.kc[l], P.kc[l], P.np[l - 1], P.kc[l], 0, ws + P.wp, nullptr, 0,
                           nullptr, 0, s));
            float* ebuf = reinterpret_cast<float*>(ws + ((l & 1) ? P.f1 : P.f0));
            MMS_TRY(gemm(1, P.Mp, P.np[l - 1], P.kc[l], ws + P.xp, 0, ws + P.wp, 0, reinterpret_cast<const float*>(ws + P.zb), ebuf, 0, s));
            if (e_out) MMS_TRY(copy2d(ebuf, P.M, P.n[l - 1], P.np[l - 1], e_out[l - 2], P.M, P.n[l - 1], P.n[l - 1], s));
            e_cur = ebuf;
            lde = P.np[l - 1];
        }
    }
    return hipSuccess;
}

hipError_t mlp_grad_rop(const MlpPlan& P, const float* x, const float* const* h, const float* const* w, const float* const* v, const float* const* c,
                        const float* g, const float* const* d, const float* const* e, float* rmu, float* const* rdw, float* const* rdb, uint8_t* ws,
                        hipStream_t s) {
    const int L = P.L;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const float* zb = F(P.zb);
    MMS_TRY(hipMemsetAsync(ws + P.zb, 0, P.cb - P.zb, s));
    // R-forward: Ra_l = [Rh_{l-1} | h_{l-1}] [W_l | V_l]^T + c_l   (layer 1: x V_1^T + c_1)
    for (int l = 1; l <= L; l++) {
        const int K = P.n[l - 1], kc = P.kc[l - 1];
        MMS_TRY(copy2d(c[l - 1], 1, P.n[l], P.n[l], F(P.cb), 1, P.np[l], P.np[l], s));
        int KCt;
        if (l == 1) {
            MMS_TRY(psplit(operand(x, K), P.M, K, P.Mp, kc, 0, ws + P.xp, s));
            MMS_TRY(psplit(operand(v[0], K), P.n[1], K, P.np[1], kc, 0, ws + P.wp, s));
            KCt = kc;
        } else {
            MMS_TRY(psplit(operand(F(P.ra[l - 1]), P.np[l - 1], 1, h[l - 2], K), P.M, K, P.Mp, 2 * kc, 0, ws + P.xp, s));
            MMS_TRY(psplit(operand(h[l - 2], K), P.M, K, P.Mp, 2 * kc, kc, ws + P.xp, s));
            MMS_TRY(psplit(operand(w[l - 1], K), P.n[l], K, P.np[l], 2 * kc, 0, ws + P.wp, s));
            MMS_TRY(psplit(operand(v[l - 1], K), P.n[l], K, P.np[l], 2 * kc, kc, ws + P.wp, s));
            KCt = 2 * kc;
        }
        MMS_TRY(gemm(1, P.Mp, P.np[l], KCt, ws + P.xp, 0, ws + P.wp, 0, F(P.cb), F(P.ra[l]), 0, s));
    }
    MMS_TRY(copy2d(F(P.ra[L]), P.M, P.n[L], P.np[L], rmu, P.M, P.n[L], P.n[L], s));
    // R-backward
    MMS_TRY(hipMemsetAsync(rdb[L - 1], 0, (size_t)P.n[L] * 4, s));
    float* T = F(P.f0);                                            // (Rd_l W_l + d_l V_l) of the layer below
    for (int l = L; l >= 1; l--) {
        const int S = P.S[l];
        const OperandArgs od = l == L ? operand(g, P.n[L]) : operand(d[l - 1], P.n[l]);
        // Rd_l (l < L; h and e hold L - 1 pointers: index L - 1 is not the caller's to read)
        const OperandArgs ord = l < L ? operand(T, P.np[l], 2, h[l - 1], P.n[l], e[l - 1], P.n[l], F(P.ra[l]), P.np[l]) : operand(nullptr, 0);
        const OperandArgs orh = l >= 2 ? operand(F(P.ra[l - 1]), P.np[l - 1], 1, h[l - 2], P.n[l - 1]) : operand(nullptr, 0);  // Rh_{l-1}
        int prods = 0;
        if (l < L) {                                               // Rd_l^T h_{l-1}
            MMS_TRY(tsplit_rows(P, l, S, prods, ord, true, ws, nullptr, 0, true, s));
            MMS_TRY(tsplit_rows(P, l - 1, S, prods, operand(l == 1 ? x : h[l - 2], P.n[l - 1]), false, ws, nullptr, 0, false, s));
            prods++;
        }
        if (l >= 2) {                                              // d_l^T Rh_{l-1}
            MMS_TRY(tsplit_rows(P, l, S, prods, od, true, ws, nullptr, 0, false, s));
            MMS_TRY(tsplit_rows(P, l - 1, S, prods, orh, false, ws, nullptr, 0, false, s));
            prods++;
        }
        MMS_TRY(weight_grad(P, l, prods, ws, rdw[l - 1], l < L ? rdb[l - 1] : nullptr, s));
        if (l >= 2) {                                              // T_{l-1} = [Rd_l | d_l] [W_l^T | V_l^T]^T  (Rd_L = 0: d_L V_L alone)
            const int kc = P.kc[l], K = P.n[l - 1];
            const int pitch = l < L ? 2 * kc : kc, off = l < L ? kc : 0;
            if (l < L) {
                MMS_TRY(psplit(ord, P.M, P.n[l], P.Mp, pitch, 0, ws + P.xp, s));
                MMS_TRY(tsplit(operand(w[l - 1], K), P.n[l], K, kc, kc, P.np[l - 1], pitch, 0, ws + P.wp, nullptr, 0, nullptr, 0, s));
            }
            MMS_TRY(psplit(od, P.M, P.n[l], P.Mp, pitch, off, ws + P.xp, s));
            MMS_TRY(tsplit(operand(v[l - 1], K), P.n[l], K, kc, kc, P.np[l - 1], pitch, off, ws + P.wp, nullptr, 0, nullptr, 0, s));
            float* Tn = F(T == F(P.f0) ? P.f1 : P.f0);
            MMS_TRY(gemm(1, P.Mp, P.np[l - 1], pitch, ws + P.xp, 0, ws + P.wp, 0, zb, Tn, 0, s));
            T = Tn;
        }
    }
    return hipSuccess;
}

#undef MMS_TRY

}  // namespace mms
