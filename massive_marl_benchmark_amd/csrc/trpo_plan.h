// trpo_plan.h -- padded shapes and workspace layout of the MLP backward / R-op (trpo_kernels.hip), shared with the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mms_host.h"   // kMlpMaxLayers, kMlpMaxRows: the limits the C ABI checks on both builds

namespace mms {

struct MlpPlan {
    int L, MC;                   // layers; 32-row chunks of the padded batch
    int64_t M, Mp;               // rows; rows padded to 128
    int n[kMlpMaxLayers + 1], np[kMlpMaxLayers + 1], kc[kMlpMaxLayers + 1];   // widths, padded to 128, in 32-chunks
    int S[kMlpMaxLayers + 1];    // row parts of layer l's weight-gradient launch
    // byte offsets into the caller's workspace: zero bias, padded bias direction, transposed planes (two products), weight-gradient
    // partials, column-sum partials, plain planes of X and of W (two k-concatenated operands each), two fp32 scratch matrices, Ra_l
    size_t zb, cb, ta, tb, part, colp, xp, wp, f0, f1, ra[kMlpMaxLayers + 1], total;
};

// Fills the plan; false on shapes it does not take (the caller reports).  rop: the R-op's extra buffers (Ra of every layer).
bool mlp_plan(int L, int64_t M, const int32_t* dims, bool rop, MlpPlan* p);

hipError_t mlp_grad(const MlpPlan& P, const float* x, const float* const* h, const float* const* w, const float* g, float* const* dw,
                    float* const* db, float* const* d_out, float* const* e_out, uint8_t* ws, hipStream_t s);

hipError_t mlp_grad_rop(const MlpPlan& P, const float* x, const float* const* h, const float* const* w, const float* const* v, const float* const* c,
                        const float* g, const float* const* d, const float* const* e, float* rmu, float* const* rdw, float* const* rdb, uint8_t* ws,
                        hipStream_t s);

}  // namespace mms
