// gru_grad_args.h -- kernel arguments of mms_gru_gates_grad_group (gru_grad_kernels.hip), shared with the C ABI file
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mms.h"

namespace mms {

struct GruGradArgs {
    const float* gi[MMS_MAX_GROUPS];        // the forward's inputs (gru_gates_args.h)
    const float* gh[MMS_MAX_GROUPS];
    const float* h[MMS_MAX_GROUPS];
    const float* mask[MMS_MAX_GROUPS];      // NULL: no mask
    const float* b_hh[MMS_MAX_GROUPS];
    const float* dh_out[MMS_MAX_GROUPS];    // d loss / d h'
    const float* dy[MMS_MAX_GROUPS];        // NULL: G = dh_out
    float* dgi[MMS_MAX_GROUPS];
    float* dgh[MMS_MAX_GROUPS];
    float* dh[MMS_MAX_GROUPS];
    float* dbias[MMS_MAX_GROUPS];           // NULL: no column sums for this group
    double* part;                           // [groups, chunks, 4H] column partials (NULL: no group has a dbias)
    int64_t g_pitch, h_pitch, mask_pitch, dh_out_pitch, dy_pitch, dg_pitch, dh_pitch;
    int64_t chunk_rows;
    int M, H, chunks;
};

int64_t gru_grad_ws_bytes(int groups, int64_t M, int H);
hipError_t launch_gru_gates_grad_group(const GruGradArgs& a, int groups, hipStream_t s);

}  // namespace mms
