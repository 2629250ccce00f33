// marl_eval_args.h -- kernel arguments of mms_marl_heads_eval (marl_eval_kernels.hip), shared with the C ABI file
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mms.h"

namespace mms {

struct HeadsEvalArgs {
    const float* h[MMS_MAX_GROUPS];             // [M, H] dense
    const float* gamma[MMS_MAX_GROUPS];         // eps < 0: not read
    const float* beta[MMS_MAX_GROUPS];
    const float* w[MMS_MAX_GROUPS];             // [A, H]
    const float* b[MMS_MAX_GROUPS];
    const float* std[MMS_MAX_GROUPS];           // [A]
    const float* act[MMS_MAX_GROUPS];           // [M, A] at act_pitch
    float* logp[MMS_MAX_GROUPS];                // [M, A] at logp_pitch; NULL: not stored
    const float* old_logp[MMS_MAX_GROUPS];      // [M, A] at old_pitch; read only where factor_out is given
    const float* factor_in[MMS_MAX_GROUPS];     // [M]; NULL: 1
    float* factor_out[MMS_MAX_GROUPS];          // [M]; NULL: no factor
    int A[MMS_MAX_GROUPS];
    int act_pitch[MMS_MAX_GROUPS], logp_pitch[MMS_MAX_GROUPS], old_pitch[MMS_MAX_GROUPS];
    int64_t M;
    int H;
    float eps;
};

hipError_t launch_marl_heads_eval(const HeadsEvalArgs& a, int groups, hipStream_t s);

}  // namespace mms
