// param_step_kernels.hip -- the parameter step of every learner in two launches (include/mms.h: mms_param_step):
//   param_sqnorm_kernel   one workgroup per chunk of a gradient tensor: the chunk's sum of squares, in double, to partials[chunk]
//   param_step_kernel     one workgroup per chunk of a stepped tensor: adds ALL partials in a fixed order (the same value in every
//                         workgroup: no atomics, no grid-wide wait), forms the clip coefficient, then streams its chunk through
//                         Adam and the polyak average (param_step_lane.h); workgroup 0 stores the norm
// The tensor table travels in the kernel arguments (param_step_args.h).  Memory- and launch-bound: 16-byte accesses where a tensor's
// pointers share their phase within 16 bytes (a scalar head and tail per chunk), scalar accesses otherwise.
// Built WITHOUT the other kernels' fast-math flags and with -ffp-contract=off (csrc/Makefile): IEEE division and square root, no
// fused multiply-add, NaN / inf propagate.
#include <hip/hip_runtime.h>

#include "param_step_args.h"

namespace mms {
namespace {

constexpr int kThreads = 256;

// the sum over the workgroup in a fixed order (the lanes of a wave by halving strides, then the waves in index order), in every thread
__device__ __forceinline__ double block_sum(double x, double* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; w++) s += lds[w];
    return s;
}

// Chunk `chunk` of a tensor of n elements: elements [lo, hi); [va, va + 4 nvec) goes in 16-byte accesses, the nhead elements in
// front of it and those from `tail` on one by one.  head: the elements up to the pointers' 16-byte boundary (0..3; every chunk starts
// at a multiple of 4 elements, so at the tensor's own phase), or kParamChunk where there is no common phase: everything is scalar.
struct Span {
    int64_t lo, hi, va, tail;
    int nvec, nhead, nscalar;
};
__device__ __forceinline__ Span chunk_span(int64_t n, int chunk, int head) {
    Span s;
    s.lo = (int64_t)chunk * kParamChunk;
    s.hi = (n - s.lo < kParamChunk) ? n : s.lo + kParamChunk;
    s.va = (s.hi - s.lo < head) ? s.hi : s.lo + head;
    s.nvec = (int)((s.hi - s.va) >> 2);
    s.tail = s.va + 4 * (int64_t)s.nvec;
    s.nhead = (int)(s.va - s.lo);
    s.nscalar = s.nhead + (int)(s.hi - s.tail);
    return s;
}
__device__ __forceinline__ int64_t scalar_element(const Span& s, int i) { return i < s.nhead ? s.lo + i : s.tail + (i - s.nhead); }
__device__ __forceinline__ unsigned phase(const void* q) { return (unsigned)(reinterpret_cast<uintptr_t>(q) & 15); }
__device__ __forceinline__ int head_of(unsigned ph) { return (int)(((16u - ph) & 15u) >> 2); }

__global__ void __launch_bounds__(kThreads) param_sqnorm_kernel(const ParamArgs a) {
    __shared__ double lds[kThreads / 64];
    const int k = blockIdx.x;
    const int t = param_chunk_tensor(a, false, k);
    const float* g = a.g[t];
    const Span s = chunk_span(a.numel[t], k - a.norm_first[t], head_of(phase(g)));
    double acc = 0.0;
    for (int i = threadIdx.x; i < s.nvec; i += kThreads) {
        const float4 x = *reinterpret_cast<const float4*>(g + s.va + 4 * (int64_t)i);
        acc += (double)x.x * (double)x.x;
        acc += (double)x.y * (double)x.y;
        acc += (double)x.z * (double)x.z;
        acc += (double)x.w * (double)x.w;
    }
    for (int i = threadIdx.x; i < s.nscalar; i += kThreads) {
        const double x = (double)g[scalar_element(s, i)];
        acc += x * x;
    }
    const double sum = block_sum(acc, lds);
    if (threadIdx.x == 0) a.partials[k] = sum;
}

__global__ void __launch_bounds__(kThreads) param_step_kernel(const ParamArgs a) {
    __shared__ double lds[kThreads / 64];
    float coef = 1.f;
    if (a.use_norm) {
        const int parts = a.norm_first[kParamMaxTensors];
        double acc = 0.0;
        for (int i = threadIdx.x; i < parts; i += kThreads) acc += a.partials[i];
        const float total = (float)sqrt(block_sum(acc, lds));
        coef = param_clip_coef(total, a.max_norm);
        if (blockIdx.x == 0 && threadIdx.x == 0 && a.norm_out) *a.norm_out = total;
    }
    const int k = blockIdx.x;
    if (k >= a.step_first[kParamMaxTensors]) return;         // (the one workgroup of a call that only asks for the norm)
    const int t = param_chunk_tensor(a, true, k);
    float* p = a.p[t];
    const float* g = a.g[t];
    float* m = a.m[t];
    float* v = a.v[t];
    float* tg = a.t[t];
    const bool adam = m != nullptr;                          // (the table builder keeps the moments only where param and grad are given)
    const unsigned ph = phase(p);
    bool same = true;
    if (adam) same = same && phase(g) == ph && phase(m) == ph && phase(v) == ph;
    if (tg) same = same && phase(tg) == ph;
    const Span s = chunk_span(a.numel[t], k - a.step_first[t], same ? head_of(ph) : (int)kParamChunk);
    const ParamCoef c = a.c;
    for (int i = threadIdx.x; i < s.nvec; i += kThreads) {
        const int64_t e = s.va + 4 * (int64_t)i;
        float4 P = *reinterpret_cast<const float4*>(p + e);
        if (adam) {
            const float4 G = *reinterpret_cast<const float4*>(g + e);
            float4 M = *reinterpret_cast<const float4*>(m + e);
            float4 V = *reinterpret_cast<const float4*>(v + e);
            param_adam(P.x, G.x, M.x, V.x, coef, c);
            param_adam(P.y, G.y, M.y, V.y, coef, c);
            param_adam(P.z, G.z, M.z, V.z, coef, c);
            param_adam(P.w, G.w, M.w, V.w, coef, c);
            *reinterpret_cast<float4*>(p + e) = P;
            *reinterpret_cast<float4*>(m + e) = M;
            *reinterpret_cast<float4*>(v + e) = V;
        }
        if (tg) {
            float4 T = *reinterpret_cast<const float4*>(tg + e);
            T.x = param_polyak(T.x, P.x, c);
            T.y = param_polyak(T.y, P.y, c);
            T.z = param_polyak(T.z, P.z, c);
            T.w = param_polyak(T.w, P.w, c);
            *reinterpret_cast<float4*>(tg + e) = T;
        }
    }
    for (int i = threadIdx.x; i < s.nscalar; i += kThreads) {
        const int64_t e = scalar_element(s, i);
        float P = p[e];
        if (adam) {
            float M = m[e], V = v[e];
            param_adam(P, g[e], M, V, coef, c);
            p[e] = P;
            m[e] = M;
            v[e] = V;
        }
        if (tg) tg[e] = param_polyak(tg[e], P, c);
    }
}

}  // namespace

// the launches of a checked call (mms_host.h: check_param_step, build_param_args)
hipError_t launch_param_step(const ParamArgs& a, hipStream_t s) {
    const int norm_chunks = a.norm_first[kParamMaxTensors], step_chunks = a.step_first[kParamMaxTensors];
    if (norm_chunks > 0) hipLaunchKernelGGL(param_sqnorm_kernel, dim3((unsigned)norm_chunks), dim3(kThreads), 0, s, a);
    const int grid = step_chunks > 0 ? step_chunks : (a.use_norm && a.norm_out ? 1 : 0);
    if (grid > 0) hipLaunchKernelGGL(param_step_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace mms
