// layer_common.h -- what the three layer-kernel files (policy_kernels.hip, split_kernels.hip, split16_kernels.hip) share: the epilogue's
// activation switch and the launchers' host helpers.  Nothing here allocates or locks: it all sits on the launch path of an eager
// rollout step.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace mms {

// epilogue activation (uniform per launch): 0 identity, 1 ELU (alpha = 1, torch.nn.ELU), 2 ReLU, 3 tanh
__device__ __forceinline__ float act_apply(float v, int act) {
    if (act == 1) return (v > 0.f) ? v : (expf(v) - 1.f);
    if (act == 2) return fmaxf(v, 0.f);
    if (act == 3) {
        // tanh = sign(v) (1 - t) / (1 + t) with t = e^(-2 |v|) in (0, 1]; a few instructions where it is inlined 64 times.  1 - t is exact
        // for t >= 1/2, so near zero the absolute error is what one ulp of t leaves (<= 6e-8) and everywhere else the quotient's
        // relative one; t cannot overflow and the result never exceeds 1.  (As 1 - 2 / (e^(2 v) + 1) the result was rounded twice at
        // magnitude 1 whatever |v|: 1.9e-7 absolute, past the layers' per-element bound 5e-7 (sum |x||w| + |b|) + 1.2e-7 in rows of
        // tiny activations -- tests/test_split16_paths_gpu.py.)
        const float t = __expf(-2.f * fabsf(v));
        return copysignf((1.f - t) / (1.f + t), v);
    }
    return v;
}

// More than 64 KB of dynamic LDS needs an opt-in per kernel and per device; remembered so that it is asked for once.  One
// instantiation, and so one table, per kernel.
template <auto Kernel>
hipError_t allow_large_lds(size_t bytes) {
    static bool done[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !done[dev]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) done[dev] = true;
    }
    return hipSuccess;
}

// the current device's CU count, cached (hipGetDeviceProperties per launch is host time an eager rollout step pays); 256 if unknown
inline int device_cu_count() {
    static int cached[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cached[dev] == 0) {
        int n = 0;
        cached[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    return cached[dev];
}

// The split layers' persistent tiling: 256-row tiles (MT = 4) when they still give every CU a block, else 128-row ones (MT = 2);
// MMS_SPLIT_MT = 2 / 4 forces one (4 only where M allows it).
inline bool split_tiles_256(int64_t M, int N, int groups, int cus) {
    static const int force_mt = getenv("MMS_SPLIT_MT") ? atoi(getenv("MMS_SPLIT_MT")) : 0;
    const int64_t tiles256 = (M % 256 == 0) ? (int64_t)groups * (M / 256) * (N / 128) : 0;
    return force_mt ? (force_mt == 4 && tiles256 > 0) : tiles256 >= cus;
}

}  // namespace mms
