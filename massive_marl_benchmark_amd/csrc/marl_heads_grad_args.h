// marl_heads_grad_args.h -- kernel arguments of mms_marl_heads_fwd_group and mms_marl_heads_grad_group (marl_heads_grad_kernels.hip),
// shared with the C ABI file
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mms.h"

namespace mms {

struct MarlHeadsFwdArgs {
    const float* f[MMS_MAX_GROUPS];         // [M, H] at f_pitch
    const float* w[MMS_MAX_GROUPS];         // [A_g, H]
    const float* b[MMS_MAX_GROUPS];         // [A_g]
    const float* log_std[MMS_MAX_GROUPS];   // [A_g]; NULL: no std for this group
    float* out[MMS_MAX_GROUPS];             // [M, A_g], dense
    float* std[MMS_MAX_GROUPS];             // [A_g]
    int32_t A[MMS_MAX_GROUPS];
    int64_t f_pitch;
    float x_coef, y_coef;
    int M, H;
};

struct MarlHeadsGradArgs {
    const float* f[MMS_MAX_GROUPS];
    const float* w[MMS_MAX_GROUPS];
    const float* dout[MMS_MAX_GROUPS];      // [M, A_g], dense
    const float* log_std[MMS_MAX_GROUPS];   // NULL: no dlog_std for this group
    const float* dstd[MMS_MAX_GROUPS];      // [A_g]
    float* df[MMS_MAX_GROUPS];              // [M, H] at df_pitch; NULL: not computed
    float* dw[MMS_MAX_GROUPS];              // [A_g, H]; NULL (with db): no sums over rows for this group
    float* db[MMS_MAX_GROUPS];              // [A_g]
    float* dlog_std[MMS_MAX_GROUPS];        // [A_g]
    int64_t part_off[MMS_MAX_GROUPS];       // group g's partials: part + part_off[g], [chunks, A_g (H + 1)] doubles
    int32_t A[MMS_MAX_GROUPS];
    double* part;
    int64_t f_pitch, df_pitch;
    int64_t chunk_rows;
    float x_coef, y_coef;
    int M, H, chunks;
};

int64_t marl_heads_grad_ws_bytes(int groups, int64_t M, int H, const int32_t* A);
hipError_t launch_marl_heads_fwd_group(const MarlHeadsFwdArgs& a, int groups, hipStream_t s);
hipError_t launch_marl_heads_grad_group(const MarlHeadsGradArgs& a, int groups, hipStream_t s);

}  // namespace mms
