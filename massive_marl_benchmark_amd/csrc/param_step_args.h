// param_step_args.h -- the argument block of the parameter-step kernels (param_step_kernels.hip).  Plain C++, no HIP include: the
// table builder in mms_host.h fills it for both builds, and the CPU build (cpu/mms_cpu.cpp) walks the same chunk table.
#pragma once
#include <stdint.h>

#include "../../include/mms.h"
#include "param_step_lane.h"

namespace mms {

constexpr int kParamMaxTensors = MMS_PARAM_MAX_TENSORS;
constexpr int64_t kParamChunk = MMS_PARAM_CHUNK;       // elements per workgroup: a multiple of 4, so every chunk starts at the tensor's own 16-byte phase

// One call's tensors and chunk tables, passed BY VALUE in the kernel arguments (no host-to-device table copy).  A tensor is cut
// into ceil(numel / kParamChunk) chunks of its own; chunk k of the norm launch belongs to the tensor t with
// norm_first[t] <= k < norm_first[t + 1] (tensors with a grad), chunk k of the step launch likewise through step_first (tensors with
// a param and an Adam step or a target).  The norm launch's chunk index is also the chunk's slot in `partials`.
struct ParamArgs {
    float* p[kParamMaxTensors];
    const float* g[kParamMaxTensors];
    float* m[kParamMaxTensors];              // NULL: no Adam for this tensor (the builder clears it where grad is NULL)
    float* v[kParamMaxTensors];
    float* t[kParamMaxTensors];              // NULL: no polyak
    int64_t numel[kParamMaxTensors];
    int32_t norm_first[kParamMaxTensors + 1];
    int32_t step_first[kParamMaxTensors + 1];
    ParamCoef c;
    float max_norm;
    int32_t tensors;
    int32_t use_norm;                        // a norm was asked for: max_norm > 0 or norm_out given
    double* partials;
    float* norm_out;                         // NULL: not stored
};
static_assert(sizeof(ParamArgs) <= 3584, "ParamArgs travels in the kernel arguments (4 KB limit)");

// the tensor of chunk k of a launch (step: the step launch's table, else the norm launch's), k below the launch's chunk count:
// first[t] <= k < first[t + 1]; tensors without chunks are passed over
MMS_HD int param_chunk_tensor(const ParamArgs& a, bool step, int k) {
    int lo = 0, hi = a.tensors;              // invariant: first[lo] <= k < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const int32_t f = step ? a.step_first[mid] : a.norm_first[mid];
        if (f <= k) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace mms
