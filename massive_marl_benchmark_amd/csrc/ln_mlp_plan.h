// ln_mlp_plan.h -- workspace layout of the LayerNorm-ELU MLP's backward and forward-mode passes (ln_mlp_kernels.hip), shared with the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "trpo_plan.h"

namespace mms {

struct LnMlpPlan {
    MlpPlan P;                           // the L + 1 Linear layers (hidden blocks and the mean head) as trpo_kernels.hip plans them
    // byte offsets behind P.total: row statistics (mean, rstd) [Mp, 2] of every level, the per-block column-sum partials of a level's
    // affine gradients, two fp32 matrices [Mp, npmax] (da_l of two neighbouring levels)
    size_t stat[kMlpMaxLayers + 1], colp2, d0, d1, total;
};

// blocks = L hidden blocks, dims[0..L+1].  False on shapes the plan does not take.
bool ln_mlp_plan(int blocks, int64_t M, const int32_t* dims, LnMlpPlan* p);

hipError_t ln_mlp_grad(const LnMlpPlan& Q, float eps, const float* x, const float* const* h, const float* const* ln_g, const float* const* ln_t,
                       const float* const* w, const float* g, float* const* dln_g, float* const* dln_t, float* const* dw, float* const* db,
                       uint8_t* ws, hipStream_t s);

hipError_t ln_mlp_jvp(const LnMlpPlan& Q, float eps, const float* x, const float* const* h, const float* const* ln_g, const float* const* ln_t,
                      const float* const* w, const float* const* vg, const float* const* vt, const float* const* vw, const float* const* vc,
                      const float* col_scale, float* rmu, uint8_t* ws, hipStream_t s);

}  // namespace mms
