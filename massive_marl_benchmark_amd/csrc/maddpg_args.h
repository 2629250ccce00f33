// maddpg_args.h -- argument blocks of the MADDPG kernels (maddpg_kernels.hip), shared with the C ABI file (mms_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mms.h"

namespace mms {

// The last layer of `groups` deterministic actors: a_g = act_limit[g] tanh(h_g w_g^T + b_g), optional exploration noise, stored to
// act_out[g] (row pitch act_pitch) and to columns (agent0 + g) A .. of joint_out (row pitch joint_pitch).
struct DetHeadsArgs {
    const float* h[MMS_MAX_GROUPS];
    const float* w[MMS_MAX_GROUPS];
    const float* b[MMS_MAX_GROUPS];
    float* act_out[MMS_MAX_GROUPS];         // NULL: no store
    float act_limit[MMS_MAX_GROUPS];
    float* joint_out;                       // NULL: no store
    int64_t* counters;                      // the head kernel only reads them: the bump is a launch of its own behind it
    uint64_t seed;
    int64_t M, row_offset, act_pitch, joint_pitch;
    int H, A, agent0;
    float sigma;
    // mms_det_heads_act (one network: groups = 1, agent0 = 0) only; the grouped entry leaves both at "none"
    float* tanh_out;                        // NULL: no store; [M,A] dense, tanh(pre) before any noise
    float noise_clip;                       // < 0: none (det_explore); >= 0: det_head_lane.h's det_smooth
};

// The last layer of `groups` critics and the Bellman backup per group (q_kernels.hip's QArgs with one network per group)
struct QGroupArgs {
    const float* h[MMS_MAX_GROUPS];
    const float* w[MMS_MAX_GROUPS];
    const float* b[MMS_MAX_GROUPS];
    float* q_out[MMS_MAX_GROUPS];           // NULL: no store
    const float* reward[MMS_MAX_GROUPS];
    const uint8_t* done[MMS_MAX_GROUPS];
    float* backup[MMS_MAX_GROUPS];          // NULL: no store
    float gamma;
    int64_t M;
    int H, iters;
};

hipError_t launch_det_heads_act(const DetHeadsArgs& a, int groups, hipStream_t s);
hipError_t launch_q_heads_backup_group(const QGroupArgs& a, int groups, hipStream_t s);

}  // namespace mms
