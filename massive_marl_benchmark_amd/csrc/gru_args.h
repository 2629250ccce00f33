// gru_args.h -- kernel arguments of mms_gru_group (gru_kernels.hip), shared with the C ABI file
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mms.h"

namespace mms {

struct GruArgs {
    const float* x[MMS_MAX_GROUPS];
    const float* h[MMS_MAX_GROUPS];
    const float* mask[MMS_MAX_GROUPS];      // NULL: hm = h
    const float* w_ih[MMS_MAX_GROUPS];
    const float* w_hh[MMS_MAX_GROUPS];
    const float* b_ih[MMS_MAX_GROUPS];
    const float* b_hh[MMS_MAX_GROUPS];
    float* h_out[MMS_MAX_GROUPS];
    float* y[MMS_MAX_GROUPS];               // NULL: no second destination
    int64_t x_pitch, h_pitch, mask_pitch, h_out_pitch;
    int M, K, H;
};

hipError_t launch_gru_group(const GruArgs& a, int groups, hipStream_t s);

}  // namespace mms
