// gru_gates_args.h -- kernel arguments of mms_gru_gates_group (gru_gates_kernels.hip), shared with the C ABI file
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mms.h"

namespace mms {

struct GruGatesArgs {
    const float* gi[MMS_MAX_GROUPS];        // [M, 3H] at g_pitch: x W_ih^T + b_ih
    const float* gh[MMS_MAX_GROUPS];        // [M, 3H] at g_pitch: h W_hh^T, unmasked, no bias
    const float* h[MMS_MAX_GROUPS];
    const float* mask[MMS_MAX_GROUPS];      // NULL: hm = h
    const float* b_hh[MMS_MAX_GROUPS];
    float* h_out[MMS_MAX_GROUPS];
    float* y[MMS_MAX_GROUPS];               // NULL: no second destination
    int64_t g_pitch, h_pitch, mask_pitch, h_out_pitch;
    int M, H;
};

hipError_t launch_gru_gates_group(const GruGatesArgs& a, int groups, hipStream_t s);

}  // namespace mms
