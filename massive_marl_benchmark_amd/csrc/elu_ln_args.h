// elu_ln_args.h -- kernel arguments of mms_elu_ln_group, mms_elu_ln_planes16_group and mms_elu_ln_grad_group (elu_ln_kernels.hip), shared
// with the C ABI file
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mms.h"

namespace mms {

struct EluLnArgs {
    const float* z[MMS_MAX_GROUPS];         // x W^T without the bias, [M, H] at z_pitch
    const float* bias[MMS_MAX_GROUPS];      // [H]
    const float* gamma[MMS_MAX_GROUPS];
    const float* beta[MMS_MAX_GROUPS];
    float* y[MMS_MAX_GROUPS];               // [M, H] at y_pitch
    float* stat[MMS_MAX_GROUPS];            // [M, 2]: (mean, rstd)
    int64_t z_pitch, y_pitch;
    float eps;
    int M, H;
};

// mms_elu_ln_planes16_group: the same call, which also leaves y_g as H32 planes (planes16_lane.h) with the rows' scales
struct EluLnPlanesArgs {
    EluLnArgs e;
    void* planes[MMS_MAX_GROUPS];           // MMS_H32_BYTES(M, H) bytes
    float* scale[MMS_MAX_GROUPS];           // [M], NULL: not stored
    float* inv[MMS_MAX_GROUPS];             // [M], NULL: not stored
};

struct EluLnGradArgs {
    const float* z[MMS_MAX_GROUPS];         // the forward's inputs
    const float* bias[MMS_MAX_GROUPS];
    const float* gamma[MMS_MAX_GROUPS];
    const float* stat[MMS_MAX_GROUPS];      // the forward's (mean, rstd)
    const float* dy[MMS_MAX_GROUPS];        // [M, H] at dy_pitch
    float* dz[MMS_MAX_GROUPS];              // [M, H] at dz_pitch
    float* dparams[MMS_MAX_GROUPS];         // [3H]: dbias | dgamma | dbeta; NULL: no column sums for this group
    double* part;                           // [groups, chunks, 3H] column partials (NULL: no group has a dparams)
    int64_t z_pitch, dy_pitch, dz_pitch;
    int64_t chunk_rows;
    int M, H, chunks;
};

int64_t elu_ln_grad_ws_bytes(int groups, int64_t M, int H);
hipError_t launch_elu_ln_group(const EluLnArgs& a, int groups, hipStream_t s);
hipError_t launch_elu_ln_planes16_group(const EluLnPlanesArgs& a, int groups, hipStream_t s);
hipError_t launch_elu_ln_grad_group(const EluLnGradArgs& a, int groups, hipStream_t s);

}  // namespace mms
