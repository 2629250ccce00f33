// mms_host.h -- the rules of the C ABI (include/mms.h) that do not touch a device, written once for both builds of the engine:
// mms_api.hip (libmms.so) and cpu/mms_cpu.cpp (libmms_cpu.so).  The engine state both keep, the host half of mms_create (config
// check, task dimensions, buffer table, construction-time scene), the entry points that only change that state, and the argument
// check of every operator entry.  Plain C++17, no HIP include.  A check returns the message for mms_last_error, or an empty string;
// what the HIP build refuses the CPU build refuses in the same words (the CPU build is the stand-in for the HIP boundary on
// machines without a GPU).  What stays different between the builds on purpose is listed in DESIGN.md section 1.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/mms.h"
#include "param_step_args.h"

namespace mms {
constexpr int kMlpMaxLayers = 8;
constexpr int64_t kMlpMaxRows = 65535 * 32 / 128 * 128;   // rows: the 32-row chunks of the padded batch index a grid dimension
}  // namespace mms

struct mms_buffer {
    const char* name;
    void* ptr;
    int64_t shape[4];
    int ndim;
    int dtype;
    size_t bytes;
    int64_t row_bytes;   // bytes per env (for indexed set_state)
};

// The engine state both builds keep; each build's mms_engine adds only what is its own.
struct mms_host_state {
    mms_config cfg;
    int actors = 0, dofs = 0, num_actions = 0, obs_dim = 0, prev_dim = 0;
    float* obs_out = nullptr;
    void* obs_planes = nullptr;
    float obs_planes_scale = 1.f;
    const float* actions_in = nullptr;      // mms_bind_actions
    bool head_on = false;                   // mms_bind_policy_head: consumed (and cleared) by the next mms_step
    mms_policy_head head{};
    int write_raw_obs = 1, write_clipped_obs = 1;
    int dr_enabled = 0;
    float* rew_out = nullptr;
    uint8_t* done_out = nullptr;
    std::vector<mms_buffer> bufs;
    std::string err;
};

// the message of a call without a handle: mms_last_error(NULL)
inline std::string g_error;

static inline int fail(mms_host_state* e, const std::string& msg) {
    if (e) e->err = msg; else g_error = msg;
    return 1;
}
// an operator entry's check: 0 to go on, 1 with the message stored
static inline int refused(const std::string& msg) { return msg.empty() ? 0 : fail(nullptr, msg); }
static inline int null_handle(const mms_host_state* h, const char* entry) { return h ? 0 : fail(nullptr, std::string(entry) + ": null handle"); }

static inline size_t dtype_size(int dt) { return dt == MMS_F32 ? 4 : dt == MMS_I64 ? 8 : dt == MMS_I32 ? 4 : 1; }

static inline mms_buffer* find(mms_host_state* e, const char* name) {
    for (auto& b : e->bufs)
        if (!strcmp(b.name, name)) return &b;
    return nullptr;
}

static inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// ---- mms_create, host half ----------------------------------------------------------------------------------------------------

// The config check and the per-task dimensions (into e, with the config).  The device field is the build's own check.
static inline std::string engine_init(mms_host_state* e, const mms_config* cfg, const mms_handle* out) {
    if (!cfg || !out) return "mms_create: null argument";
    if (cfg->abi_version != MMS_ABI_VERSION) return "mms_create: ABI version mismatch";
    if (cfg->num_envs <= 0 || cfg->num_agents <= 0) return "mms_create: num_envs and num_agents must be positive";
    const int A = cfg->num_agents;
    if (cfg->task == MMS_TASK_TEN_ANT) { e->actors = A + 1; e->dofs = 8 * A; e->num_actions = 8 * A; e->obs_dim = 38 * A + 8; e->prev_dim = 4 * A + 2; }
    else if (cfg->task == MMS_TASK_ONE_ANT) { e->actors = 2; e->dofs = 8; e->num_actions = 8; e->obs_dim = 60; e->prev_dim = 6; }
    else if (cfg->task == MMS_TASK_MULTI_ANT_CIRCLE) { e->actors = A + 1; e->dofs = 8 * A; e->num_actions = 8 * A; e->obs_dim = 38 * A; e->prev_dim = 2 * A; }
    else if (cfg->task == MMS_TASK_MULTI_INGENUITY) { e->actors = A; e->dofs = 4 * A; e->num_actions = 6 * A; e->obs_dim = 13 * A; e->prev_dim = 3 * A; }
    else return "mms_create: unknown task";
    if (cfg->task == MMS_TASK_MULTI_INGENUITY && A != 4) return "mms_create: MultiIngenuity has 4 helicopters per env";
    if (cfg->task == MMS_TASK_ONE_ANT && A != 1) return "mms_create: OneAnt has one ant per env";
    if (cfg->task == MMS_TASK_MULTI_ANT_CIRCLE && A != 2) return "mms_create: MultiAntCircle has two ants per env";
    // one env is one workgroup of at most 512 lanes: 4 per ant, rounded up to 8, and 8 for the box
    if (cfg->task != MMS_TASK_MULTI_INGENUITY && ((4 * A + 7) & ~7) + 8 > 512) return "mms_create: at most 126 ants per env";
    e->cfg = *cfg;
    return {};
}

// The named buffers of an engine (name, dtype, shape, sizes; ptr NULL): each build allocates them zero-filled where its step reads them.
static inline std::vector<mms_buffer> buffer_table(const mms_host_state& e) {
    const int64_t N = e.cfg.num_envs, A = e.cfg.num_agents;
    const struct { const char* name; int dtype; int64_t rows, cols; } table[] = {       // cols 0: one dimension
        {"actions", MMS_F32, N, e.num_actions},
        {"obs", MMS_F32, N, e.obs_dim},
        {"obs_clipped", MMS_F32, N, e.obs_dim},
        {"rew", MMS_F32, N, 0},
        {"reset", MMS_I64, N, 0},
        {"progress", MMS_I64, N, 0},
        {"reset_count", MMS_I64, N, 0},
        {"root_states", MMS_F32, N * e.actors, 13},
        {"initial_root_states", MMS_F32, N * e.actors, 13},
        {"dof_state", MMS_F32, N * e.dofs, 2},
        {"env_origin", MMS_F32, N, 3},
        {"prev", MMS_F32, N, e.prev_dim},
        {"reset_noise", MMS_F32, N, 16},
        {"foot_sensors", MMS_F32, N * A, 24},
        {"dr_params", MMS_F32, N * A, MMS_DR_FLOATS},
    };
    std::vector<mms_buffer> out;
    for (const auto& t : table) {
        mms_buffer b{};
        b.name = t.name;
        b.dtype = t.dtype;
        b.ndim = t.cols ? 2 : 1;
        b.shape[0] = t.rows;
        b.shape[1] = t.cols;
        b.bytes = (size_t)t.rows * (size_t)(t.cols ? t.cols : 1) * dtype_size(t.dtype);
        b.row_bytes = (int64_t)(b.bytes / (size_t)N);
        out.push_back(b);
    }
    return out;
}

// The construction-time scene (what create_sim .. prepare_sim leave in the reference, agents/tasks/ten_ant.py:205-633) into the
// caller's zero-filled host arrays, shaped as the buffers of the same names.  root_states starts as a copy of initial_root_states.
static inline void fill_scene(const mms_host_state& e, float* initial_root_states, float* env_origin, float* prev, int64_t* reset, float* dr_params) {
    const mms_config* cfg = &e.cfg;
    const int N = cfg->num_envs, A = cfg->num_agents;
    int64_t npr = (int64_t)sqrt((double)cfg->total_envs);
    if (npr < 1) npr = 1;
    for (int i = 0; i < N; i++) {
        int64_t gi = cfg->env_offset + i;
        float* o = env_origin + 3 * (size_t)i;
        o[0] = (float)(gi % npr) * 2.f * cfg->env_spacing;                       // env grid: SURVEY.md B.2 convention
        o[1] = (float)(gi / npr) * 2.f * cfg->env_spacing;
        float* r = initial_root_states + (size_t)i * e.actors * 13;
        for (int k = 0; k < e.actors; k++) r[13 * k + 6] = 1.f;
        if (cfg->task != MMS_TASK_MULTI_INGENUITY) {
            for (int k = 0; k < A; k++) {                                        // ten_ant.py:339-358 / one_ant.py:234
                float off = (A == 1) ? 0.f : (1.5f + 3.f * (float)(k / 2)) * ((k % 2 == 0) ? -1.f : 1.f);
                r[13 * k + 0] = cfg->ant_start_x; r[13 * k + 1] = off; r[13 * k + 2] = cfg->ant_start_z;
                if (cfg->task == MMS_TASK_MULTI_ANT_CIRCLE) {                       // multi_ant_circle.py:216-219: (3, 0, 1) and (-3, 0, 1)
                    r[13 * k + 0] = (k % 2 == 0) ? cfg->ant_start_x : -cfg->ant_start_x; r[13 * k + 1] = 0.f;
                }
            }
            for (int j = 0; j < 3; j++) r[13 * A + j] = cfg->box_start[j];       // ten_ant.py:494-495
        } else {
            static const float hy[4] = {2.f, -2.f, 6.f, -6.f};                   // multi_ingenuity.py:157-164
            for (int k = 0; k < A; k++) { r[13 * k + 0] = 0.f; r[13 * k + 1] = hy[k % 4]; r[13 * k + 2] = 1.f; }
        }
        // caches start as the construction-time poses: what reset_idx reads from the not-yet-refreshed tensors on the
        // first step (ten_ant.py:870-882, one_ant.py:410-411), in the global frame
        float* pv = prev + (size_t)i * e.prev_dim;
        if (cfg->task == MMS_TASK_TEN_ANT) {
            const float* b = r + 13 * A;
            float bx = b[0] + o[0], by = b[1] + o[1];
            float ang = atanf((2.f * b[6] * b[5]) / (1.f - 2.f * b[5] * b[5]));   // ten_ant.py:935-947
            float sv = sinf(ang), cv = -cosf(ang);
            for (int k = 0; k < A; k++) {
                pv[2 * k] = r[13 * k] + o[0]; pv[2 * k + 1] = r[13 * k + 1] + o[1];
                float off = 1.5f + 3.0f * (float)(k / 2);
                pv[2 * A + 2 * k] = (k % 2 == 0) ? bx + off * sv : bx - off * sv;
                pv[2 * A + 2 * k + 1] = (k % 2 == 0) ? by + off * cv : by - off * cv;
            }
            pv[4 * A] = bx; pv[4 * A + 1] = by;
        } else if (cfg->task == MMS_TASK_ONE_ANT) {
            pv[0] = r[0] + o[0]; pv[1] = r[1] + o[1]; pv[2] = r[13] + o[0]; pv[3] = r[14] + o[1];
            pv[4] = -4.f / cfg->dt; pv[5] = -4.f / cfg->dt;                       // one_ant.py:143-144
        } else if (cfg->task == MMS_TASK_MULTI_ANT_CIRCLE) {
            for (int k = 0; k < A; k++) { pv[2 * k] = r[13 * k] + o[0]; pv[2 * k + 1] = r[13 * k + 1] + o[1]; }   // multi_ant_circle.py:367-368
        }
        reset[i] = 1;                                                            // base_task.py:62-63
    }
    for (size_t k = 0; k < (size_t)N * A; k++)                                   // nominal: scales 1, limit offsets 0
        for (int j = 0; j < 17; j++) dr_params[k * MMS_DR_FLOATS + j] = 1.f;
}

// ---- the entry points that only read or change host state -----------------------------------------------------------------------

static inline int host_get_tensor(mms_host_state* h, const char* name, mms_tensor* out) {
    if (!h || !name || !out) return fail(h, "mms_get_tensor: null argument");
    mms_buffer* b = find(h, name);
    if (!b) return fail(h, std::string("mms_get_tensor: unknown buffer '") + name + "'");
    memset(out, 0, sizeof(*out));
    out->ptr = b->ptr;
    for (int i = 0; i < b->ndim; i++) out->shape[i] = b->shape[i];
    out->ndim = b->ndim;
    out->dtype = b->dtype;
    out->device = h->cfg.device;
    return 0;
}

// the checks of mms_set_state (all ids are checked before anything is written); *buffer is the destination
static inline int host_set_state_check(mms_host_state* h, const char* name, const void* src, const int64_t* env_ids, int64_t n, mms_buffer** buffer) {
    if (!h || !name || !src) return fail(h, "mms_set_state: null argument");
    mms_buffer* b = find(h, name);
    if (!b) return fail(h, std::string("mms_set_state: unknown buffer '") + name + "'");
    *buffer = b;
    if (!env_ids) return 0;
    if (b->row_bytes <= 0) return fail(h, "mms_set_state: buffer is not per-env");
    if (n < 0) return fail(h, "mms_set_state: negative row count");
    for (int64_t i = 0; i < n; i++)
        if (env_ids[i] < 0 || env_ids[i] >= h->cfg.num_envs) return fail(h, "mms_set_state: env id out of range");
    return 0;
}

static inline int host_bind_obs_out(mms_host_state* h, void* dst) {
    if (null_handle(h, "mms_bind_obs_out")) return 1;
    h->obs_out = (float*)dst;
    return 0;
}

static inline int host_bind_obs_planes16(mms_host_state* h, void* planes, float scale) {
    if (null_handle(h, "mms_bind_obs_planes16")) return 1;
    if (!planes) { h->obs_planes = nullptr; return 0; }
    if (h->cfg.task == MMS_TASK_MULTI_INGENUITY) return fail(h, "mms_bind_obs_planes16: not for the helicopter task (its policies' layers are 256 wide: exact-fp32 kernel)");
    int e = 0;
    if (!(scale > 0.f) || frexpf(scale, &e) != 0.5f) return fail(h, "mms_bind_obs_planes16: the scale must be a power of two");
    if (!(h->cfg.clip_obs * scale <= 16384.f)) return fail(h, "mms_bind_obs_planes16: clip_observations x scale must not exceed 2^14 (fp16 planes)");
    if ((addr(planes) & 15) != 0) return fail(h, "mms_bind_obs_planes16: the planes must be 16-byte aligned");
    h->obs_planes = planes;
    h->obs_planes_scale = scale;
    return 0;
}

static inline int host_bind_actions(mms_host_state* h, const float* src) {
    if (null_handle(h, "mms_bind_actions")) return 1;
    if (src && (addr(src) & 7) != 0) return fail(h, "mms_bind_actions: the action tensor must be 8-byte aligned");
    h->actions_in = src;
    return 0;
}

// step_takes_head: the build's own answer to "this engine's step takes a head" (asked only with a handle and a head)
static inline int host_bind_policy_head(mms_host_state* h, const mms_policy_head* head, bool step_takes_head) {
    if (null_handle(h, "mms_bind_policy_head")) return 1;
    if (!head) { h->head_on = false; return 0; }
    if (h->dr_enabled || !step_takes_head)
        return fail(h, "mms_bind_policy_head: not available for this engine (needs the 16-envs-per-workgroup TenAnt layout: 10 ants, num_envs a multiple "
                       "of 16 and >= 16 per CU, no physical DR) -- launch mms_ppo_heads_act instead");
    if (!head->hidden || !head->weight || !head->bias || !head->vhidden || !head->vweight || !head->vbias || !head->log_std || !head->counters)
        return fail(h, "mms_bind_policy_head: null pointer (hidden, weight, bias, vhidden, vweight, vbias, log_std, counters are required)");
    if (head->A != 8 * h->cfg.num_agents || head->H <= 0 || head->H % 512 != 0 || head->VH <= 0 || head->VH % 4 != 0)
        return fail(h, "mms_bind_policy_head: A must be 8 x num_agents, H a multiple of 512, VH a multiple of 4");
    if (((addr(head->hidden) | addr(head->weight) | addr(head->vhidden) | addr(head->vweight) | addr(head->weight_tiles)) & 15) != 0)
        return fail(h, "mms_bind_policy_head: hidden, weight, weight_tiles, vhidden, vweight must be 16-byte aligned");
    h->head = *head;
    h->head_on = true;
    return 0;
}

static inline int host_set_dr(mms_host_state* h, int32_t enable) {
    if (null_handle(h, "mms_set_dr")) return 1;
    if (enable && h->cfg.task == MMS_TASK_MULTI_INGENUITY) return fail(h, "mms_set_dr: the helicopter task has no randomised physical parameters");
    // the other half of mms_bind_policy_head's "no physical DR": the fused head's step kernel has no DR form, so DR cannot come on between
    // a bind and the step that consumes it (nothing changes: the head stays bound, DR stays off)
    if (enable && h->head_on)
        return fail(h, "mms_set_dr: a policy head is bound (mms_bind_policy_head) and its step has no physical DR -- step first, or unbind with "
                       "mms_bind_policy_head(h, NULL)");
    h->dr_enabled = enable != 0;
    return 0;
}

static inline int host_set_obs_outputs(mms_host_state* h, int32_t raw, int32_t clipped) {
    if (null_handle(h, "mms_set_obs_outputs")) return 1;
    h->write_raw_obs = raw != 0;
    h->write_clipped_obs = clipped != 0;
    return 0;
}

static inline int host_bind_rollout_out(mms_host_state* h, float* rew_out, uint8_t* done_out) {
    if (null_handle(h, "mms_bind_rollout_out")) return 1;
    h->rew_out = rew_out;
    h->done_out = done_out;
    return 0;
}

// ---- the operator entries' argument checks (after the build's device-argument check) -----------------------------------------------
// x_pitch arguments are the effective pitch (the caller has replaced 0 by K).

static inline std::string check_groups(const char* entry, int32_t groups) {
    if (groups >= 1 && groups <= MMS_MAX_GROUPS) return {};
    return std::string(entry) + ": groups must be 1.." + std::to_string(MMS_MAX_GROUPS);
}

static inline bool all_set(int n, const float* const* p) {
    if (!p) return false;
    for (int i = 0; i < n; i++)
        if (!p[i]) return false;
    return true;
}

static inline std::string check_gae_ppo_normalized(const float* rewards, const uint8_t* dones, const float* values, const float* last_values,
                                                   const float* returns, const float* advantages, const double* stats, int32_t T, int64_t N) {
    if (!rewards || !dones || !values || !last_values || !returns || !advantages || !stats || T < 1 || N < 1)
        return "mms_gae_ppo_normalized: bad arguments (null pointer, T < 1 or N < 1)";
    return {};
}

static inline std::string check_gae_ppo(const float* rewards, const uint8_t* dones, const float* values, const float* last_values,
                                        const float* returns, const float* advantages, const double* stats, int32_t T, int64_t N) {
    if (!rewards || !dones || !values || !last_values || !returns || !advantages || !stats || T < 1 || N < 1)
        return "mms_gae_ppo: bad arguments (null pointer, T < 1 or N < 1)";
    return {};
}

static inline std::string check_adv_normalize(const float* advantages, const double* stats, int64_t count) {
    if (!advantages || !stats || count < 1) return "mms_adv_normalize: bad arguments (null pointer or count < 1)";
    return {};
}

// mms_gae_marl (A = 1) and mms_gae_marl_agents
static inline std::string check_gae_marl(const char* entry, const float* rewards, const float* value_preds, const float* masks, const float* returns,
                                         int32_t T, int64_t N, int32_t A, int32_t use_norm, const float* norm_mean, const float* norm_var) {
    if (!rewards || !value_preds || !masks || !returns || T < 1 || N < 1 || A < 1)
        return std::string(entry) + ": bad arguments (null pointer, T < 1, N < 1 or A < 1)";
    if (use_norm && (!norm_mean || !norm_var)) return std::string(entry) + ": use_norm needs norm_mean and norm_var";
    return {};
}

// (n = 0, an empty batch, is accepted: nothing is launched over)
static inline std::string check_marl_views(const float* obs_clipped, const float* obs_all, int64_t n, int32_t agents, int32_t per_agent, int32_t shared) {
    if (n < 0 || agents < 1 || per_agent < 1 || shared < 0 || (n > 0 && (!obs_clipped || !obs_all)))
        return "mms_marl_views: bad arguments (null pointer, n < 0, agents < 1, per_agent < 1 or shared < 0)";
    return {};
}

static inline std::string check_ppo_act(const float* mean, const float* log_std, const int64_t* counters, int64_t N, int32_t A) {
    if (!mean || !log_std || !counters || N < 0 || A <= 0 || A > 128) return "mms_ppo_act: bad arguments (A must be in 1..128)";
    return {};
}

static inline std::string check_ppo_heads_act(const float* hidden, const float* weight, const float* bias, int32_t H, const float* vhidden,
                                              const float* vweight, const float* vbias, int32_t VH, const float* log_std, const int64_t* counters,
                                              int64_t N, int32_t A) {
    if (!hidden || !weight || !bias || !log_std || !counters || N < 0 || A <= 0 || A > 128 || H <= 0 || (H % 64) != 0)
        return "mms_ppo_heads_act: bad arguments (A must be in 1..128, H a positive multiple of 64)";
    if (vhidden && (!vweight || !vbias || VH <= 0 || (VH % 4) != 0))
        return "mms_ppo_heads_act: the value head needs weight, bias and a hidden width that is a multiple of 4";
    if ((addr(hidden) | addr(weight) | addr(vhidden) | addr(vweight)) & 15)
        return "mms_ppo_heads_act: hidden, weight, vhidden and vweight must be 16-byte aligned";
    return {};
}

static inline std::string check_sac_heads_act(const float* hidden, int32_t H, const float* mu_weight, const float* mu_bias, const float* ls_weight,
                                              const float* ls_bias, int32_t deterministic, const int64_t* counters, int64_t N, int32_t A) {
    if (!hidden || !mu_weight || !mu_bias || !ls_weight || !ls_bias || (!deterministic && !counters) || N < 0 || A <= 0 || A > 128 || H <= 0 ||
        (H % 64) != 0)
        return "mms_sac_heads_act: bad arguments (A must be in 1..128, H a positive multiple of 64, counters required unless deterministic)";
    if ((addr(hidden) | addr(mu_weight) | addr(ls_weight)) & 15) return "mms_sac_heads_act: hidden and both weight matrices must be 16-byte aligned";
    return {};
}

// mms_sac_heads_grad: the shapes, then (workspace NULL is the size query: nothing else is read; N == 0: nothing to do, nothing else
// is read) the operands and the workspace against `need`, the bytes this build's plan asks for (the CPU build's: 0).
static inline std::string check_sac_heads_grad(int64_t N, int32_t A, const float* u, const float* mu, const float* log_std, const float* grad_action,
                                               const float* grad_logp, const float* dy, const void* workspace, const int64_t* ws_bytes,
                                               int64_t need) {
    if (!ws_bytes) return "mms_sac_heads_grad: ws_bytes required";
    if (N < 0 || N > 0x7fffffff) return "mms_sac_heads_grad: N must be in 0..2147483647";
    if (A < 1 || A > 128) return "mms_sac_heads_grad: A must be in 1..128";
    if (!workspace || N == 0) return {};
    if (!u || !mu || !log_std || !dy) return "mms_sac_heads_grad: null pointer (u, mu, log_std and dy are required)";
    if (!grad_action && !grad_logp) return "mms_sac_heads_grad: no incoming gradient (grad_action and grad_logp both NULL)";
    if (*ws_bytes < need) return "mms_sac_heads_grad: workspace too small (" + std::to_string(*ws_bytes) + " bytes, needs " + std::to_string(need) + ")";
    if (addr(workspace) & 255) return "mms_sac_heads_grad: workspace must be 256-byte aligned";
    return {};
}

// all checks before any work; G is 2 when the second network is given
static inline std::string check_q_heads_backup(int64_t M, int32_t H, const float* h0, const float* w0, const float* b0, const float* q0_out,
                                               const float* h1, const float* w1, const float* b1, const float* q1_out, const float* reward,
                                               const uint8_t* done, const float* backup) {
    if (!h0 || !w0 || !b0 || M < 0 || H <= 0 || (H % 64) != 0 || H > MMS_Q_MAX_H)
        return "mms_q_heads_backup: bad arguments (h0, w0, b0 required, M >= 0, H a positive multiple of 64 up to " + std::to_string(MMS_Q_MAX_H) + ")";
    if ((h1 || w1 || b1 || q1_out) && !(h1 && w1 && b1)) return "mms_q_heads_backup: the second network needs h1, w1 and b1 (or all four NULL: one network)";
    if ((addr(h0) | addr(w0) | addr(h1) | addr(w1)) & 15) return "mms_q_heads_backup: hidden activations and weights must be 16-byte aligned";
    if (!q0_out && !q1_out && !backup) return "mms_q_heads_backup: no destination (q0_out, q1_out, backup all NULL)";
    if (backup && (!reward || !done)) return "mms_q_heads_backup: the backup needs reward and done";
    return {};
}

// mms_q_heads_loss: everything before any work (workspace NULL is the size query: nothing else is read)
static inline std::string check_q_heads_loss(int64_t M, int32_t H, const float* h0, const float* w0, const float* b0, const float* h1, const float* w1,
                                             const float* b1, int32_t mode, const float* target, const float* loss, const float* q1_out,
                                             const float* dh0, const float* dh1, const float* dw0, const float* db0, const float* dw1, const float* db1,
                                             const void* workspace, const int64_t* ws_bytes, int64_t need) {
    if (!ws_bytes) return "mms_q_heads_loss: ws_bytes required";
    if (M < 1 || M > 0x7fffffff) return "mms_q_heads_loss: M must be in 1..2147483647 (a mean of no rows has no value)";
    if (H <= 0 || (H % 64) != 0 || H > MMS_Q_LOSS_MAX_H)
        return "mms_q_heads_loss: H must be a positive multiple of 64 up to " + std::to_string(MMS_Q_LOSS_MAX_H);
    if (mode != 0 && mode != 1) return "mms_q_heads_loss: mode must be 0 (MSE) or 1 (policy)";
    if (!workspace) return {};
    if (!h0 || !w0 || !b0 || !loss) return "mms_q_heads_loss: null pointer (h0, w0, b0 and loss are required)";
    if ((h1 || w1 || b1) && !(h1 && w1 && b1)) return "mms_q_heads_loss: the second network needs h1, w1 and b1 (or all NULL: one network)";
    if (!h1 && (q1_out || dh1 || dw1 || db1)) return "mms_q_heads_loss: an output of the second network without h1, w1 and b1";
    if (mode == 0 && !target) return "mms_q_heads_loss: mode 0 needs target";
    if (mode == 1 && target) return "mms_q_heads_loss: mode 1 takes no target";
    if ((!dw0) != (!db0) || (!dw1) != (!db1)) return "mms_q_heads_loss: dw_g and db_g are given together or both NULL";
    if ((addr(h0) | addr(w0) | addr(h1) | addr(w1) | addr(dh0) | addr(dh1)) & 15)
        return "mms_q_heads_loss: hidden activations, weights and dh must be 16-byte aligned";
    if (*ws_bytes < need) return "mms_q_heads_loss: workspace too small (" + std::to_string(*ws_bytes) + " bytes, needs " + std::to_string(need) + ")";
    if (addr(workspace) & 255) return "mms_q_heads_loss: workspace must be 256-byte aligned";
    return {};
}

static inline std::string check_det_heads_act_group(int32_t groups, int64_t M, int32_t H, int32_t A, int32_t agent0, const float* const* h,
                                                    const float* const* w, const float* const* b, const float* act_limit, float sigma,
                                                    const int64_t* counters, float* const* act_out, int64_t act_pitch, const float* joint_out,
                                                    int64_t joint_pitch) {
    std::string bad = check_groups("mms_det_heads_act_group", groups);
    if (!bad.empty()) return bad;
    if (!h || !w || !b || !act_limit || M < 0 || A <= 0 || A > 128 || H <= 0 || (H % 64) != 0 || agent0 < 0 || !(sigma >= 0.f))
        return "mms_det_heads_act_group: bad arguments (A must be in 1..128, H a positive multiple of 64, M >= 0, agent0 >= 0, sigma >= 0)";
    if (sigma > 0.f && !counters) return "mms_det_heads_act_group: sigma > 0 needs counters";
    bool any_act = false;
    for (int g = 0; g < groups; g++) {
        if (!h[g] || !w[g] || !b[g]) return "mms_det_heads_act_group: null pointer in a group";
        if ((addr(h[g]) | addr(w[g])) & 15) return "mms_det_heads_act_group: hidden activations and weights must be 16-byte aligned";
        const bool act = act_out && act_out[g];
        any_act = any_act || act;
        if (!act && !joint_out) return "mms_det_heads_act_group: no destination (act_out[g] and joint_out both NULL)";
    }
    if (any_act && act_pitch < A) return "mms_det_heads_act_group: act_pitch below A";
    if (joint_out && joint_pitch < ((int64_t)agent0 + groups) * A) return "mms_det_heads_act_group: joint_pitch below (agent0 + groups) * A";
    return {};
}

// mms_det_heads_act: the grouped entry's limits for one network, two optional destinations
static inline std::string check_det_heads_act(int64_t M, int32_t H, int32_t A, const float* h, const float* w, const float* b, float act_limit,
                                              float sigma, float noise_clip, const int64_t* counters, const float* act_out, int64_t act_pitch,
                                              const float* tanh_out) {
    if (!h || !w || !b || M < 0 || A <= 0 || A > 128 || H <= 0 || (H % 64) != 0 || !(sigma >= 0.f) || noise_clip != noise_clip || act_limit != act_limit)
        return "mms_det_heads_act: bad arguments (h, w, b required, A must be in 1..128, H a positive multiple of 64, M >= 0, sigma >= 0, no NaN)";
    if (sigma > 0.f && !counters) return "mms_det_heads_act: sigma > 0 needs counters";
    if ((addr(h) | addr(w)) & 15) return "mms_det_heads_act: hidden activations and weights must be 16-byte aligned";
    if (!act_out && !tanh_out) return "mms_det_heads_act: no destination (act_out and tanh_out both NULL)";
    if (act_out && act_pitch < A) return "mms_det_heads_act: act_pitch below A";
    return {};
}

// the noise clip as the kernels take it: the value where it is finite and >= 0, -1 ("none") for a negative one and +inf
static inline float det_noise_clip(float noise_clip) { return (noise_clip >= 0.f && noise_clip <= 3.4028234e38f) ? noise_clip : -1.f; }

// mms_det_heads_grad: mms_sac_heads_grad's order -- the shapes, then (workspace NULL is the size query: nothing else is read; N == 0:
// nothing to do, nothing else is read) the operands and the workspace against `need`, the bytes this build's plan asks for (CPU build: 0)
static inline std::string check_det_heads_grad(int64_t N, int32_t A, const float* t, const float* g, int64_t grad_pitch, const float* dy,
                                               const void* workspace, const int64_t* ws_bytes, int64_t need) {
    if (!ws_bytes) return "mms_det_heads_grad: ws_bytes required";
    if (N < 0 || N > 0x7fffffff) return "mms_det_heads_grad: N must be in 0..2147483647";
    if (A < 1 || A > 128) return "mms_det_heads_grad: A must be in 1..128";
    if (!workspace || N == 0) return {};
    if (!t || !g || !dy) return "mms_det_heads_grad: null pointer (t, g and dy are required)";
    if (grad_pitch < A) return "mms_det_heads_grad: grad_pitch below A";
    if (*ws_bytes < need) return "mms_det_heads_grad: workspace too small (" + std::to_string(*ws_bytes) + " bytes, needs " + std::to_string(need) + ")";
    if (addr(workspace) & 255) return "mms_det_heads_grad: workspace must be 256-byte aligned";
    return {};
}

static inline std::string check_q_heads_backup_group(int32_t groups, int64_t M, int32_t H, const float* const* h, const float* const* w,
                                                     const float* const* b, float* const* q_out, const float* const* reward,
                                                     const uint8_t* const* done, float* const* backup) {
    std::string bad = check_groups("mms_q_heads_backup_group", groups);
    if (!bad.empty()) return bad;
    if (!h || !w || !b || M < 0 || H <= 0 || (H % 64) != 0 || H > MMS_Q_MAX_H)
        return "mms_q_heads_backup_group: bad arguments (h, w, b required, M >= 0, H a positive multiple of 64 up to " + std::to_string(MMS_Q_MAX_H) + ")";
    bool any = false;
    for (int g = 0; g < groups; g++) {
        if (!h[g] || !w[g] || !b[g]) return "mms_q_heads_backup_group: null pointer in a group";
        if ((addr(h[g]) | addr(w[g])) & 15) return "mms_q_heads_backup_group: hidden activations and weights must be 16-byte aligned";
        if (backup && backup[g] && (!reward || !done || !reward[g] || !done[g])) return "mms_q_heads_backup_group: the backup needs reward and done";
        any = any || (q_out && q_out[g]) || (backup && backup[g]);
    }
    if (!any) return "mms_q_heads_backup_group: no destination (every q_out[g] and backup[g] NULL)";
    return {};
}

// mms_ppo_loss: the shapes, then (workspace NULL is the size query: nothing else is read) the operands and the workspace against
// `need`, the bytes this build's plan asks for (the CPU build's: 0).
static inline std::string check_ppo_loss(int64_t M, int32_t A, const float* mu, const float* log_std, const float* value, const float* actions,
                                         const float* old_logp, const float* adv, const float* returns, const float* target_values,
                                         const float* old_mu, const float* old_sigma, const float* out, const float* dmu, const float* dlog_std,
                                         const float* dvalue, const void* workspace, const int64_t* ws_bytes, int64_t need) {
    if (!ws_bytes) return "mms_ppo_loss: ws_bytes required";
    if (M < 1 || M > 0x7fffffff) return "mms_ppo_loss: M must be in 1..2147483647";
    if (A < 1 || A > MMS_PPO_LOSS_MAX_A) return "mms_ppo_loss: A must be in 1.." + std::to_string(MMS_PPO_LOSS_MAX_A);
    if (!workspace) return {};
    if (!mu || !log_std || !value || !actions || !old_logp || !adv || !returns || !target_values || !old_mu || !old_sigma || !out)
        return "mms_ppo_loss: null pointer (mu, log_std, value, actions, old_logp, adv, returns, target_values, old_mu, old_sigma and out are required)";
    if ((dmu || dlog_std || dvalue) && !(dmu && dlog_std && dvalue)) return "mms_ppo_loss: dmu, dlog_std and dvalue go together (all three, or all NULL: the terms only)";
    if (*ws_bytes < need) return "mms_ppo_loss: workspace too small (" + std::to_string(*ws_bytes) + " bytes, needs " + std::to_string(need) + ")";
    if (addr(workspace) & 255) return "mms_ppo_loss: workspace must be 256-byte aligned";
    return {};
}

// mms_trpo_heads: check_ppo_loss's order; what is required follows from the outputs asked for (include/mms.h lists it).
static inline std::string check_trpo_heads(int64_t M, int32_t A, const float* mu, const float* log_std, const float* rmu, const float* actions,
                                           const float* adv, const float* old_mu, const float* old_sigma, const float* old_logp, const float* out,
                                           const float* logp, const float* gsur, const float* gkl, const float* gn, const void* workspace,
                                           const int64_t* ws_bytes, int64_t need) {
    if (!ws_bytes) return "mms_trpo_heads: ws_bytes required";
    if (M < 1 || M > 0x7fffffff) return "mms_trpo_heads: M must be in 1..2147483647";
    if (A < 1 || A > MMS_PPO_LOSS_MAX_A) return "mms_trpo_heads: A must be in 1.." + std::to_string(MMS_PPO_LOSS_MAX_A);
    if (!workspace) return {};
    if (!out && !logp && !gsur && !gkl && !gn) return "mms_trpo_heads: no output (out, logp, gsur, gkl and gn all NULL)";
    if (!log_std) return "mms_trpo_heads: null pointer (log_std is required)";
    if (gn && !rmu) return "mms_trpo_heads: gn needs rmu";
    if ((out || logp || gsur || gkl) && !mu) return "mms_trpo_heads: null pointer (out, logp, gsur and gkl need mu)";
    if ((out || logp || gsur) && !actions) return "mms_trpo_heads: null pointer (out, logp and gsur need actions)";
    if ((out || gsur) && (!old_logp || !adv)) return "mms_trpo_heads: null pointer (out and gsur need old_logp and adv)";
    if ((out || gkl) && !old_mu) return "mms_trpo_heads: null pointer (out and gkl need old_mu)";
    if (out && !old_sigma) return "mms_trpo_heads: null pointer (out needs old_sigma)";
    if (*ws_bytes < need) return "mms_trpo_heads: workspace too small (" + std::to_string(*ws_bytes) + " bytes, needs " + std::to_string(need) + ")";
    if (addr(workspace) & 255) return "mms_trpo_heads: workspace must be 256-byte aligned";
    return {};
}

// mms_marl_ppo_loss: as check_ppo_loss, with the stored fields' pitches and what each flag requires.
static inline std::string check_marl_ppo_loss(int64_t M, int32_t A, const float* mu, const float* std, const float* value, const mms_marl_loss_fields* f,
                                              int32_t policy_masks, int32_t value_masks, int32_t use_norm, const float* norm_mean,
                                              const float* norm_var, const float* out, const float* dmu, const float* dstd, const float* dvalue,
                                              const void* workspace, const int64_t* ws_bytes, int64_t need) {
    if (!ws_bytes) return "mms_marl_ppo_loss: ws_bytes required";
    if (M < 1 || M > 0x7fffffff) return "mms_marl_ppo_loss: M must be in 1..2147483647";
    if (A < 1 || A > MMS_MARL_LOSS_MAX_A) return "mms_marl_ppo_loss: A must be in 1.." + std::to_string(MMS_MARL_LOSS_MAX_A);
    if (!workspace) return {};
    if (!mu || !std || !value || !f || !out || !f->actions.base || !f->old_logp.base || !f->adv.base || !f->value_preds.base || !f->returns.base)
        return "mms_marl_ppo_loss: null pointer (mu, std, value, fields, its actions, old_logp, adv, value_preds and returns, and out are required)";
    if ((policy_masks || value_masks) && !f->active_masks.base) return "mms_marl_ppo_loss: a mask flag is on but active_masks is NULL";
    if (use_norm && (!norm_mean || !norm_var)) return "mms_marl_ppo_loss: use_norm needs norm_mean and norm_var";
    if (f->actions.pitch < A || f->old_logp.pitch < A) return "mms_marl_ppo_loss: the pitch of actions and old_logp must be at least A";
    if (f->adv.pitch < 1 || f->value_preds.pitch < 1 || f->returns.pitch < 1 || (f->active_masks.base && f->active_masks.pitch < 1) ||
        (f->factor.base && f->factor.pitch < 1))
        return "mms_marl_ppo_loss: the pitch of adv, value_preds, returns, active_masks and factor must be at least 1";
    if ((dmu || dstd || dvalue) && !(dmu && dstd && dvalue)) return "mms_marl_ppo_loss: dmu, dstd and dvalue go together (all three, or all NULL: the terms only)";
    if (*ws_bytes < need) return "mms_marl_ppo_loss: workspace too small (" + std::to_string(*ws_bytes) + " bytes, needs " + std::to_string(need) + ")";
    if (addr(workspace) & 255) return "mms_marl_ppo_loss: workspace must be 256-byte aligned";
    return {};
}

// mms_marl_ppo_loss_group: the shared shapes and the table, then check_marl_ppo_loss per group (the first refusal names its group).
static inline std::string check_marl_ppo_loss_group(int32_t groups, int64_t M, int32_t A, const mms_marl_loss_group* table, int32_t policy_masks,
                                                    int32_t value_masks, int32_t use_norm, const void* workspace, const int64_t* ws_bytes, int64_t need) {
    const std::string name = "mms_marl_ppo_loss_group";
    if (!ws_bytes) return name + ": ws_bytes required";
    std::string bad = check_groups(name.c_str(), groups);
    if (!bad.empty()) return bad;
    if (M < 1 || M > 0x7fffffff) return name + ": M must be in 1..2147483647";
    if (A < 1 || A > MMS_MARL_LOSS_MAX_A) return name + ": A must be in 1.." + std::to_string(MMS_MARL_LOSS_MAX_A);
    if (!workspace) return {};
    if (!table) return name + ": table is NULL";
    for (int g = 0; g < groups; g++) {
        const mms_marl_loss_group& t = table[g];
        bad = check_marl_ppo_loss(M, A, t.mu, t.std, t.value, &t.fields, policy_masks, value_masks, use_norm, t.norm_mean, t.norm_var, t.out, t.dmu, t.dstd,
                                  t.dvalue, workspace, ws_bytes, need);
        if (!bad.empty()) return name + ": group " + std::to_string(g) + ": " + bad;
    }
    return {};
}

static inline std::string check_linear2_act(int64_t M, int32_t N, int32_t K, const float* x0, const float* w0, const float* b0, const float* y0,
                                            const float* x1, const float* w1, const float* b1, const float* y1, int32_t act) {
    if (!x0 || !w0 || !b0 || !y0 || M < 0 || M > 0x7fffffff || N <= 0 || K <= 0 || (K % 4) != 0 || act < 0 || act > 3)
        return "mms_linear2_act: bad arguments (K must be a positive multiple of 4, act 0..3)";
    if ((x1 || w1 || b1 || y1) && !(x1 && w1 && b1 && y1)) return "mms_linear2_act: the second problem needs all four pointers";
    return {};
}

static inline std::string check_split_planes(int64_t rows, int32_t K, int32_t x_pitch, const float* x, const void* planes) {
    if (!x || !planes || rows < 0 || K <= 0 || x_pitch < K || (x_pitch % 4) != 0 || (addr(x) & 15) != 0 || (addr(planes) & 15) != 0)
        return "mms_split_planes: bad arguments (x and planes 16-byte aligned, x_pitch >= K and a multiple of 4)";
    return {};
}

static inline std::string check_split_planes_group(int32_t groups, int64_t rows, int32_t K, int32_t x_pitch, const float* const* x, void* const* planes) {
    std::string bad = check_groups("mms_split_planes_group", groups);
    if (!bad.empty()) return bad;
    if (!x || !planes || rows < 0 || K <= 0 || x_pitch < K) return "mms_split_planes_group: bad arguments (x_pitch >= K)";
    for (int g = 0; g < groups; g++)
        if (!x[g] || !planes[g] || (addr(planes[g]) & 15) != 0 || (addr(x[g]) & 3) != 0)
            return "mms_split_planes_group: null or misaligned pointer in a group (planes 16-byte aligned)";
    return {};
}

// mms_linear_group_act_split (x_inv, w_inv, y_scale unused: scaled = false) and mms_linear_group_act_split16 (scaled = true)
static inline std::string check_split_layer(bool scaled, int32_t groups, int64_t M, int32_t N, int32_t K, const void* const* x, const void* const* w,
                                            const float* const* b, void* const* y, const float* const* x_inv, const float* const* w_inv,
                                            const float* const* y_scale, int32_t act, int32_t out_mode, const float* const* ln_s,
                                            const float* const* ln_stat_in, float* const* ln_part_out, const float* const* head_w,
                                            float* const* head_part, const int32_t* head_dims) {
    const char* fn = scaled ? "mms_linear_group_act_split16" : "mms_linear_group_act_split";
    std::string bad = check_groups(fn, groups);
    if (!bad.empty()) return bad;
    if (!x || !w || !b || (scaled && (!x_inv || !w_inv)) || M < 0 || M > 0x7fffffff || (M % 128) != 0 || N <= 0 || (N % 128) != 0 || K <= 0 || act < 0 ||
        act > 3 || out_mode < 0 || out_mode > 2 || (out_mode != 2 && !y) || (scaled && out_mode == 1 && !y_scale))
        return std::string(fn) + ": bad arguments (M and N multiples of 128, act 0..3, out_mode 0..2" + (scaled ? ", x_inv, w_inv, y_scale with out_mode 1)" : ")");
    const bool ln = ln_s || ln_stat_in || ln_part_out;
    if (ln && (!ln_s || !ln_stat_in || !ln_part_out || act != 1 || out_mode == 0))
        return std::string(fn) + ": the LayerNorm folds come together (ln_s, ln_stat_in, ln_part_out), with act = ELU and out_mode 1 or 2";
    if (out_mode == 2 && (!ln || !head_w || !head_part || !head_dims)) return std::string(fn) + ": out_mode 2 needs the LayerNorm folds, head_w, head_part and head_dims";
    for (int g = 0; g < groups; g++) {
        if (!x[g] || !w[g] || !b[g] || (scaled && (!x_inv[g] || !w_inv[g])) || (out_mode != 2 && !y[g]) || (scaled && out_mode == 1 && !y_scale[g]) ||
            (ln && (!ln_s[g] || !ln_stat_in[g] || !ln_part_out[g])) || (out_mode == 2 && (!head_w[g] || !head_part[g])))
            return std::string(fn) + ": null pointer in a group";
        uintptr_t bits = addr(x[g]) | addr(w[g]) | addr(b[g]);                   // 16 bytes; the (mean, rstd) pairs and slot partials 8
        if (scaled) bits |= addr(w_inv[g]);
        if (out_mode != 2) bits |= addr(y[g]);
        if (ln) bits |= addr(ln_s[g]) | (addr(ln_stat_in[g]) << 1) | (addr(ln_part_out[g]) << 1);
        if ((bits & 15) != 0) return std::string(fn) + ": operands must be 16-byte aligned";
        if (out_mode == 2 && (head_dims[g] < 1 || head_dims[g] > 16)) return "split layer, out_mode 2: 1 <= head_dims[g] <= 16";
    }
    return {};
}

static inline std::string check_split_planes16_group(int32_t groups, int64_t rows, int32_t K, int32_t x_pitch, const float* const* x, void* const* planes,
                                                     float* const* scale, float* const* inv, int32_t nchains, int32_t L, const float* const* chain,
                                                     float* const* chain_scale, float* const* chain_inv, float* const* stat) {
    std::string bad = check_groups("mms_split_planes16_group", groups);
    if (!bad.empty()) return bad;
    if (!x || !planes || !scale || !inv || rows < 0 || K <= 0 || x_pitch < K || nchains < 0 || L < 0 || (nchains > 0 && (L < 1 || !chain || !chain_scale || !chain_inv)))
        return "mms_split_planes16_group: bad arguments (x_pitch >= K; nchains > 0 needs L >= 1, chain, chain_scale, chain_inv)";
    for (int g = 0; g < groups; g++) {
        if (!x[g] || !planes[g] || (addr(planes[g]) & 15) != 0 || (addr(x[g]) & 3) != 0 || (nchains > 0 && (!chain[g] || !chain_scale[g] || !chain_inv[g])))
            return "mms_split_planes16_group: null or misaligned pointer in a group (planes 16-byte aligned)";
        if (stat && (!stat[g] || (addr(stat[g]) & 7) != 0)) return "mms_split_planes16_group: null or misaligned stat pointer in a group";
    }
    return {};
}

// (pitch0 / pitch1 as the entry resolved them: 0 has become the source's own K)
static inline std::string check_split_planes16_cat(int64_t rows, int32_t K0, int32_t pitch0, const float* x0, int32_t K1, int32_t pitch1, const float* x1,
                                                   const void* planes, int32_t nchains, int32_t L, const float* chain, const float* chain_scale,
                                                   const float* chain_inv) {
    if (rows < 0 || K0 < 1 || K1 < 1 || (int64_t)K0 + K1 > 0x7fffffe0 || pitch0 < K0 || pitch1 < K1 || nchains < 0 || L < 0 ||
        (nchains > 0 && (L < 1 || !chain || !chain_scale || !chain_inv)))
        return "mms_split_planes16_cat: bad arguments (rows >= 0; K0, K1 >= 1; pitch0 >= K0, pitch1 >= K1; nchains > 0 needs L >= 1, chain, chain_scale, chain_inv)";
    if (!x0 || !x1 || !planes || (addr(planes) & 15) != 0 || ((addr(x0) | addr(x1)) & 3) != 0)
        return "mms_split_planes16_cat: null or misaligned pointer (x0, x1 4-byte aligned, planes 16-byte aligned)";
    return {};
}

static inline std::string check_weight_planes16_group(int32_t groups, const int64_t* N, const int32_t* K, const float* const* w, void* const* planes,
                                                      float* const* scale, float* const* inv) {
    std::string bad = check_groups("mms_weight_planes16_group", groups);
    if (!bad.empty()) return bad;
    if (!N || !K || !w || !planes || !scale || !inv) return "mms_weight_planes16_group: bad arguments (null array)";
    for (int g = 0; g < groups; g++) {
        if (N[g] < 0 || K[g] <= 0) return "mms_weight_planes16_group: bad shape in a group (N >= 0, K > 0)";
        if (!w[g] || !planes[g] || !scale[g] || !inv[g] || (addr(planes[g]) & 15) != 0 || (addr(w[g]) & 3) != 0 || (addr(inv[g]) & 15) != 0)
            return "mms_weight_planes16_group: null or misaligned pointer in a group (planes and inv 16-byte aligned)";
    }
    return {};
}

static inline std::string check_chain_refresh16(int32_t nchains, int32_t L, const float* const* l1, const int32_t* n, const float* chain, float bound0,
                                                int64_t rows, const float* chain_scale, const float* chain_inv) {
    if (nchains < 1 || L < 1 || (int64_t)nchains * L > MMS_MAX_GROUPS || !l1 || !n || !chain || rows < 0 || (rows > 0 && (!chain_scale || !chain_inv || !(bound0 >= 0.f))))
        return "mms_chain_refresh16: bad arguments (nchains, L >= 1, nchains * L <= " + std::to_string(MMS_MAX_GROUPS) + "; rows > 0 needs chain_scale, chain_inv, bound0 >= 0)";
    for (int e = 0; e < nchains * L; e++)
        if (!l1[e] || n[e] < 0) return "mms_chain_refresh16: null pointer or negative count in an entry";
    return {};
}

static inline std::string check_fold_planes16_group(int32_t groups, const int64_t* N, const int32_t* K, const float* const* w, void* const* planes,
                                                    float* const* inv) {
    std::string bad = check_groups("mms_fold_planes16_group", groups);
    if (!bad.empty()) return bad;
    if (!N || !K || !w) return "mms_fold_planes16_group: bad arguments (null array)";
    for (int g = 0; g < groups; g++) {
        if (N[g] < 0 || K[g] <= 0) return "mms_fold_planes16_group: bad shape in a group (N >= 0, K > 0)";
        if (!w[g] || (planes && planes[g] && (!inv || !inv[g])) || (planes && (addr(planes[g]) & 15) != 0))
            return "mms_fold_planes16_group: null or misaligned pointer in a group (planes 16-byte aligned and with inv)";
    }
    return {};
}

static inline std::string check_fold_scales16_group(int32_t groups, const float* const* rb, const int32_t* n, int64_t M) {
    std::string bad = check_groups("mms_fold_scales16_group", groups);
    if (!bad.empty()) return bad;
    if (!rb || !n || M < 0) return "mms_fold_scales16_group: bad arguments";
    for (int g = 0; g < groups; g++)
        if (!rb[g] || n[g] < 0) return "mms_fold_scales16_group: null pointer or negative count in a group";
    return {};
}

static inline std::string check_layer_clock_probe(const uint64_t* out, int32_t slots) {
    if (out && slots < 1) return "mms_layer_clock_probe: slots must be >= 1 with an output buffer";
    if (out && (addr(out) & 7) != 0) return "mms_layer_clock_probe: the buffer must be 8-byte aligned";
    return {};
}

static inline std::string check_row_stats_chan_group(int32_t groups, int64_t M, int32_t slots, const float* const* part, float* const* stat) {
    std::string bad = check_groups("mms_row_stats_chan_group", groups);
    if (!bad.empty()) return bad;
    if (!part || !stat || M < 0 || slots < 1) return "mms_row_stats_chan_group: bad arguments";
    for (int g = 0; g < groups; g++)
        if (!part[g] || !stat[g]) return "mms_row_stats_chan_group: null pointer in a group";
    return {};
}

static inline std::string check_marl_heads_finish(int32_t groups, int64_t M, int32_t slots, const float* const* part, const float* const* head_part,
                                                  const float* const* hs, const float* const* hc, const int32_t* A, float* const* out,
                                                  const int32_t* out_pitch) {
    std::string bad = check_groups("mms_marl_heads_finish", groups);
    if (!bad.empty()) return bad;
    if (!part || !head_part || !hs || !hc || !A || !out || M < 0 || slots < 1) return "mms_marl_heads_finish: bad arguments";
    for (int g = 0; g < groups; g++) {
        if (!part[g] || !head_part[g] || !hs[g] || !hc[g] || !out[g] || A[g] < 1 || A[g] > 16)
            return "mms_marl_heads_finish: null pointer or output width outside 1..16 in a group";
        if ((addr(head_part[g]) & 15) != 0 || (addr(part[g]) & 7) != 0)
            return "mms_marl_heads_finish: head_part must be 16-byte aligned and part 8-byte aligned (read as float4 / float2)";
        if (out_pitch && out_pitch[g] < A[g]) return "mms_marl_heads_finish: out_pitch below the output width";
    }
    return {};
}

static inline std::string check_linear_group_act(int32_t groups, int64_t M, int32_t N, int32_t K, const float* const* x, const float* const* w,
                                                 const float* const* b, float* const* y, int32_t act, const float* const* ln_s,
                                                 const float* const* ln_stat_in, float* const* ln_part_out) {
    std::string bad = check_groups("mms_linear_group_act", groups);
    if (!bad.empty()) return bad;
    if (!x || !w || !b || !y || M < 0 || M > 0x7fffffff || N <= 0 || K <= 0 || (K % 4) != 0 || act < 0 || (act & ~16) > 3)
        return "mms_linear_group_act: bad arguments (K must be a positive multiple of 4, act 0..3, optionally + 16)";
    if ((ln_stat_in != nullptr) != (ln_s != nullptr)) return "mms_linear_group_act: ln_stat_in and ln_s come together";
    if ((ln_stat_in || ln_part_out) && ((act & ~16) != 1 || M % 128 != 0 || N % 128 != 0 || K < 8))
        return "mms_linear_group_act: the LayerNorm folds need act = ELU, M and N multiples of 128";
    for (int g = 0; g < groups; g++)
        if (!x[g] || !w[g] || !b[g] || !y[g] || (ln_s && (!ln_s[g] || !ln_stat_in[g])) || (ln_part_out && !ln_part_out[g]))
            return "mms_linear_group_act: null pointer in a group";
    return {};
}

static inline std::string check_row_stats_group(int32_t groups, int64_t M, int32_t slots, int32_t width, const float* const* part, float* const* stat) {
    std::string bad = check_groups("mms_row_stats_group", groups);
    if (!bad.empty()) return bad;
    if (!part || !stat || M < 0 || slots < 1 || width < 1) return "mms_row_stats_group: bad arguments";
    for (int g = 0; g < groups; g++)
        if (!part[g] || !stat[g]) return "mms_row_stats_group: null pointer in a group";
    return {};
}

static inline std::string check_row_moments_group(int32_t groups, int64_t M, int32_t K, int32_t x_pitch, const float* const* x, float* const* stat) {
    std::string bad = check_groups("mms_row_moments_group", groups);
    if (!bad.empty()) return bad;
    if (!x || !stat || M < 0 || K <= 0 || K > 4096 || x_pitch < K) return "mms_row_moments_group: bad arguments (1 <= K <= 4096)";
    for (int g = 0; g < groups; g++)
        if (!x[g] || !stat[g]) return "mms_row_moments_group: null pointer in a group";
    return {};
}

static inline std::string check_layernorm_group(int32_t groups, int64_t M, int32_t K, int32_t Kp, int32_t x_pitch, const float* const* x,
                                                const float* const* gamma, const float* const* beta, float* const* y) {
    std::string bad = check_groups("mms_layernorm_group", groups);
    if (!bad.empty()) return bad;
    if (!x || !gamma || !beta || !y || M < 0 || K <= 0 || K > 4096 || Kp < K || x_pitch < K)
        return "mms_layernorm_group: bad arguments (1 <= K <= 4096, Kp >= K, x_pitch >= K or 0)";
    for (int g = 0; g < groups; g++) {
        if (!x[g] || !gamma[g] || !beta[g] || !y[g]) return "mms_layernorm_group: null pointer in a group";
        if ((Kp != K || x_pitch != K) && x[g] == y[g]) return "mms_layernorm_group: in place needs Kp == x_pitch == K";
    }
    return {};
}

static inline std::string check_marl_heads_act(int32_t groups, int64_t M, int32_t H, const float* const* h, const float* const* gamma,
                                               const float* const* beta, const float* const* w, const float* const* b, const int32_t* A,
                                               float* const* out, const int32_t* out_pitch, float eps) {
    std::string bad = check_groups("mms_marl_heads_act", groups);
    if (!bad.empty()) return bad;
    const bool ln = eps >= 0.f;                          // eps < 0: the plain output layer -- gamma / beta are not read (NULL allowed)
    if (!h || (ln && (!gamma || !beta)) || !w || !b || !A || !out || M < 0 || H <= 0 || H > 1024) return "mms_marl_heads_act: bad arguments (1 <= H <= 1024)";
    for (int g = 0; g < groups; g++) {
        if (!h[g] || (ln && (!gamma[g] || !beta[g])) || !w[g] || !b[g] || !out[g] || A[g] < 1 || A[g] > 16)
            return "mms_marl_heads_act: null pointer in a group, or outputs outside 1..16";
        if (out_pitch && out_pitch[g] < A[g]) return "mms_marl_heads_act: out_pitch below the number of outputs";
    }
    return {};
}

// mms_marl_heads_eval: mms_marl_heads_act's front, the actions given.  Pitches: NULL = A[g].
static inline std::string check_marl_heads_eval(int32_t groups, int64_t M, int32_t H, const float* const* h, const float* const* gamma,
                                                const float* const* beta, const float* const* w, const float* const* b, const int32_t* A,
                                                const float* const* std, const float* const* act, const int32_t* act_pitch, float* const* logp,
                                                const int32_t* logp_pitch, const float* const* old_logp, const int32_t* old_pitch,
                                                const float* const* factor_in, float* const* factor_out, float eps) {
    std::string bad = check_groups("mms_marl_heads_eval", groups);
    if (!bad.empty()) return bad;
    const bool ln = eps >= 0.f;                          // eps < 0: the plain output layer -- gamma / beta are not read (NULL allowed)
    if (!h || (ln && (!gamma || !beta)) || !w || !b || !A || !std || !act || M < 0 || M > 0x7fffffff || H <= 0 || H > 1024)
        return "mms_marl_heads_eval: bad arguments (h, w, b, A, std and act are required; 1 <= H <= 1024)";
    for (int g = 0; g < groups; g++) {
        if (!h[g] || (ln && (!gamma[g] || !beta[g])) || !w[g] || !b[g] || !std[g] || !act[g] || A[g] < 1 || A[g] > 16)
            return "mms_marl_heads_eval: null pointer in a group, or action dimensions outside 1..16";
        if ((act_pitch && act_pitch[g] < A[g]) || (logp_pitch && logp_pitch[g] < A[g]) || (old_pitch && old_pitch[g] < A[g]))
            return "mms_marl_heads_eval: a row pitch below the number of action dimensions";
        if (factor_out && factor_out[g] && !(old_logp && old_logp[g])) return "mms_marl_heads_eval: factor_out needs old_logp";
        if (logp && logp[g] && (logp[g] == act[g] || (old_logp && logp[g] == old_logp[g])))
            return "mms_marl_heads_eval: logp must not be act or old_logp";
    }
    (void)factor_in;
    return {};
}

// mms_gru_group.  A workgroup writes its rows of h_out / y while others still read those rows of x and h: no destination may be one of
// the sources (compared as pointers over all groups: the layers of one [M, recurrent_N, H] slot interleave legitimately).
static inline std::string check_gru_group(int32_t groups, int64_t M, int32_t K, int32_t H, const float* const* x, int64_t x_pitch, const float* const* h,
                                          int64_t h_pitch, const float* const* mask, int64_t mask_pitch, const float* const* w_ih, const float* const* w_hh,
                                          const float* const* b_ih, const float* const* b_hh, float* const* h_out, int64_t h_out_pitch, float* const* y) {
    std::string bad = check_groups("mms_gru_group", groups);
    if (!bad.empty()) return bad;
    if (!x || !h || !w_ih || !w_hh || !b_ih || !b_hh || !h_out) return "mms_gru_group: null pointer (x, h, w_ih, w_hh, b_ih, b_hh and h_out are required)";
    if (M < 0 || M > 0x7fffffff || K < 4 || (K % 4) != 0 || H < 4 || (H % 4) != 0 || H > 1024)
        return "mms_gru_group: bad shapes (0 <= M <= 2147483647, K and H positive multiples of 4, H <= 1024)";
    if (x_pitch < K || h_pitch < H || h_out_pitch < H || (x_pitch % 4) != 0 || (h_pitch % 4) != 0 || (h_out_pitch % 4) != 0 || (mask && mask_pitch < 1))
        return "mms_gru_group: bad pitches (x_pitch >= K, h_pitch >= H, h_out_pitch >= H, each a multiple of 4; mask_pitch >= 1)";
    for (int g = 0; g < groups; g++) {
        if (!x[g] || !h[g] || !w_ih[g] || !w_hh[g] || !b_ih[g] || !b_hh[g] || !h_out[g] || (mask && !mask[g])) return "mms_gru_group: null pointer in a group";
        if (((addr(x[g]) | addr(h[g]) | addr(w_ih[g]) | addr(w_hh[g]) | addr(h_out[g]) | (y ? addr(y[g]) : 0)) & 15) != 0 ||
            ((addr(b_ih[g]) | addr(b_hh[g]) | (mask ? addr(mask[g]) : 0)) & 3) != 0)
            return "mms_gru_group: misaligned pointer in a group (x, h, w_ih, w_hh, h_out, y 16-byte aligned)";
    }
    for (int g = 0; g < groups; g++)
        for (int q = 0; q < groups; q++) {
            if (h_out[g] == h[q] || h_out[g] == x[q]) return "mms_gru_group: h_out must not be h or x (other workgroups still read those rows)";
            if (y && y[g] && (y[g] == h[q] || y[g] == x[q] || y[g] == h_out[q])) return "mms_gru_group: y must not be h, x or h_out";
            if (q != g && (h_out[g] == h_out[q] || (y && y[g] && y[g] == y[q]))) return "mms_gru_group: two groups share a destination";
        }
    return {};
}

// mms_gru_gates_group: the refusal rules of mms_gru_group with the pre-activation blocks gi / gh in x's place (and b_hh read 16 bytes
// at a time)
static inline std::string check_gru_gates_group(int32_t groups, int64_t M, int32_t H, const float* const* gi, const float* const* gh, int64_t g_pitch,
                                                const float* const* h, int64_t h_pitch, const float* const* mask, int64_t mask_pitch,
                                                const float* const* b_hh, float* const* h_out, int64_t h_out_pitch, float* const* y) {
    std::string bad = check_groups("mms_gru_gates_group", groups);
    if (!bad.empty()) return bad;
    if (!gi || !gh || !h || !b_hh || !h_out) return "mms_gru_gates_group: null pointer (gi, gh, h, b_hh and h_out are required)";
    if (M < 0 || M > 0x7fffffff || H < 4 || (H % 4) != 0 || H > 1024)
        return "mms_gru_gates_group: bad shapes (0 <= M <= 2147483647, H a positive multiple of 4, H <= 1024)";
    if (g_pitch < 3 * (int64_t)H || h_pitch < H || h_out_pitch < H || (g_pitch % 4) != 0 || (h_pitch % 4) != 0 || (h_out_pitch % 4) != 0 || (mask && mask_pitch < 1))
        return "mms_gru_gates_group: bad pitches (g_pitch >= 3 H, h_pitch >= H, h_out_pitch >= H, each a multiple of 4; mask_pitch >= 1)";
    for (int g = 0; g < groups; g++) {
        if (!gi[g] || !gh[g] || !h[g] || !b_hh[g] || !h_out[g] || (mask && !mask[g])) return "mms_gru_gates_group: null pointer in a group";
        if (((addr(gi[g]) | addr(gh[g]) | addr(h[g]) | addr(b_hh[g]) | addr(h_out[g]) | (y ? addr(y[g]) : 0)) & 15) != 0 || ((mask ? addr(mask[g]) : 0) & 3) != 0)
            return "mms_gru_gates_group: misaligned pointer in a group (gi, gh, h, b_hh, h_out, y 16-byte aligned)";
    }
    for (int g = 0; g < groups; g++)
        for (int q = 0; q < groups; q++) {
            if (h_out[g] == h[q] || h_out[g] == gi[q] || h_out[g] == gh[q]) return "mms_gru_gates_group: h_out must not be h, gi or gh";
            if (y && y[g] && (y[g] == h[q] || y[g] == gi[q] || y[g] == gh[q] || y[g] == h_out[q])) return "mms_gru_gates_group: y must not be h, gi, gh or h_out";
            if (q != g && (h_out[g] == h_out[q] || (y && y[g] && y[g] == y[q]))) return "mms_gru_gates_group: two groups share a destination";
        }
    return {};
}

// mms_gru_gates_grad_group: ws_bytes and the shapes first (workspace NULL is the size query: nothing else is read), then the forward's
// rules for the forward's inputs, the same pitch and alignment rules for the gradients, and every destination against every source and
// every other destination over all groups.  `need`: the build's workspace size (the CPU build: 0).
static inline std::string check_gru_gates_grad_group(int32_t groups, int64_t M, int32_t H, const float* const* gi, const float* const* gh, int64_t g_pitch,
                                                     const float* const* h, int64_t h_pitch, const float* const* mask, int64_t mask_pitch,
                                                     const float* const* b_hh, const float* const* dh_out, int64_t dh_out_pitch, const float* const* dy,
                                                     int64_t dy_pitch, float* const* dgi, float* const* dgh, int64_t dg_pitch, float* const* dh,
                                                     int64_t dh_pitch, float* const* dbias, const void* workspace, const int64_t* ws_bytes, int64_t need) {
    const char* who = "mms_gru_gates_grad_group";
    std::string bad = check_groups(who, groups);
    if (!bad.empty()) return bad;
    if (!ws_bytes) return std::string(who) + ": ws_bytes required";
    if (M < 0 || M > 0x7fffffff || H < 4 || (H % 4) != 0 || H > 1024)
        return std::string(who) + ": bad shapes (0 <= M <= 2147483647, H a positive multiple of 4, H <= 1024)";
    if (!workspace) return {};
    if (!gi || !gh || !h || !b_hh || !dh_out || !dgi || !dgh || !dh)
        return std::string(who) + ": null pointer (gi, gh, h, b_hh, dh_out, dgi, dgh and dh are required)";
    if (g_pitch < 3 * (int64_t)H || dg_pitch < 3 * (int64_t)H || h_pitch < H || dh_out_pitch < H || dh_pitch < H || (dy && dy_pitch < H) || (g_pitch % 4) != 0 ||
        (dg_pitch % 4) != 0 || (h_pitch % 4) != 0 || (dh_out_pitch % 4) != 0 || (dh_pitch % 4) != 0 || (dy && (dy_pitch % 4) != 0) || (mask && mask_pitch < 1))
        return std::string(who) + ": bad pitches (g_pitch, dg_pitch >= 3 H; h_pitch, dh_out_pitch, dy_pitch, dh_pitch >= H; each a multiple of 4; mask_pitch >= 1)";
    if (*ws_bytes < need) return std::string(who) + ": workspace too small (" + std::to_string(*ws_bytes) + " bytes, needs " + std::to_string(need) + ")";
    if (addr(workspace) & 255) return std::string(who) + ": workspace must be 256-byte aligned";
    for (int g = 0; g < groups; g++) {
        if (!gi[g] || !gh[g] || !h[g] || !b_hh[g] || !dh_out[g] || !dgi[g] || !dgh[g] || !dh[g] || (mask && !mask[g])) return std::string(who) + ": null pointer in a group";
        if (((addr(gi[g]) | addr(gh[g]) | addr(h[g]) | addr(b_hh[g]) | addr(dh_out[g]) | (dy ? addr(dy[g]) : 0) | addr(dgi[g]) | addr(dgh[g]) | addr(dh[g])) & 15) != 0 ||
            (((mask ? addr(mask[g]) : 0) | (dbias ? addr(dbias[g]) : 0)) & 3) != 0)
            return std::string(who) + ": misaligned pointer in a group (gi, gh, h, b_hh, dh_out, dy, dgi, dgh, dh 16-byte aligned)";
    }
    for (int g = 0; g < groups; g++) {
        const float* dst[4] = {dgi[g], dgh[g], dh[g], dbias ? dbias[g] : nullptr};
        for (int k = 0; k < 4; k++) {
            if (!dst[k]) continue;
            for (int l = k + 1; l < 4; l++)
                if (dst[k] == dst[l]) return std::string(who) + ": two destinations share an address";
            for (int q = 0; q < groups; q++) {
                const float* src[7] = {gi[q], gh[q], h[q], mask ? mask[q] : nullptr, b_hh[q], dh_out[q], dy ? dy[q] : nullptr};
                for (int l = 0; l < 7; l++)
                    if (dst[k] == src[l]) return std::string(who) + ": a destination (dgi, dgh, dh, dbias) must not be a source (gi, gh, h, mask, b_hh, dh_out, dy)";
                if (q == g) continue;
                const float* other[4] = {dgi[q], dgh[q], dh[q], dbias ? dbias[q] : nullptr};
                for (int l = 0; l < 4; l++)
                    if (dst[k] == other[l]) return std::string(who) + ": two groups share a destination";
            }
        }
    }
    return {};
}

// the shapes of mms_elu_ln_group and mms_elu_ln_grad_group
static inline bool elu_ln_shapes(int32_t groups, int64_t M, int32_t H) {
    return groups >= 1 && groups <= MMS_MAX_GROUPS && M >= 0 && M <= 0x7fffffff && H >= 4 && (H % 4) == 0 && H <= 1024;
}

// mms_elu_ln_group: shapes, pitches, then per group the pointers, their alignment and every destination against every source and every
// other destination over all groups
static inline std::string check_elu_ln_group(int32_t groups, int64_t M, int32_t H, float eps, const float* const* z, int64_t z_pitch, const float* const* bias,
                                             const float* const* gamma, const float* const* beta, float* const* y, int64_t y_pitch, float* const* stat,
                                             const char* who = "mms_elu_ln_group") {
    std::string bad = check_groups(who, groups);
    if (!bad.empty()) return bad;
    if (!elu_ln_shapes(groups, M, H)) return std::string(who) + ": bad shapes (0 <= M <= 2147483647, H a positive multiple of 4, H <= 1024)";
    if (!(eps >= 0.f)) return std::string(who) + ": eps must be >= 0";
    if (!z || !bias || !gamma || !beta || !y || !stat) return std::string(who) + ": null pointer (z, bias, gamma, beta, y and stat are required)";
    if (z_pitch < H || y_pitch < H || (z_pitch % 4) != 0 || (y_pitch % 4) != 0) return std::string(who) + ": bad pitches (z_pitch, y_pitch >= H, each a multiple of 4)";
    for (int g = 0; g < groups; g++) {
        if (!z[g] || !bias[g] || !gamma[g] || !beta[g] || !y[g] || !stat[g]) return std::string(who) + ": null pointer in a group";
        if (((addr(z[g]) | addr(bias[g]) | addr(gamma[g]) | addr(beta[g]) | addr(y[g])) & 15) != 0 || (addr(stat[g]) & 7) != 0)
            return std::string(who) + ": misaligned pointer in a group (z, bias, gamma, beta, y 16-byte aligned, stat 8)";
    }
    for (int g = 0; g < groups; g++) {
        if (y[g] == stat[g]) return std::string(who) + ": two destinations share an address";
        for (int q = 0; q < groups; q++) {
            const float* src[4] = {z[q], bias[q], gamma[q], beta[q]};
            for (int l = 0; l < 4; l++)
                if (y[g] == src[l] || stat[g] == src[l]) return std::string(who) + ": a destination (y, stat) must not be a source (z, bias, gamma, beta)";
            if (q != g && (y[g] == y[q] || y[g] == stat[q] || stat[g] == stat[q])) return std::string(who) + ": two groups share a destination";
        }
    }
    return {};
}

// mms_elu_ln_planes16_group: mms_elu_ln_group's rules under its own name, then the three further destinations (scale_g and inv_g are
// optional) against every source and every other destination over all groups
static inline std::string check_elu_ln_planes16_group(int32_t groups, int64_t M, int32_t H, float eps, const float* const* z, int64_t z_pitch,
                                                      const float* const* bias, const float* const* gamma, const float* const* beta, float* const* y,
                                                      int64_t y_pitch, float* const* stat, void* const* planes, float* const* scale, float* const* inv) {
    const char* who = "mms_elu_ln_planes16_group";
    std::string bad = check_elu_ln_group(groups, M, H, eps, z, z_pitch, bias, gamma, beta, y, y_pitch, stat, who);
    if (!bad.empty()) return bad;
    if (!planes || !scale || !inv) return std::string(who) + ": null pointer (the planes, scale and inv arrays are required; scale and inv entries may be NULL)";
    for (int g = 0; g < groups; g++) {
        if (!planes[g]) return std::string(who) + ": null planes pointer in a group";
        if ((addr(planes[g]) & 15) != 0 || ((addr(scale[g]) | addr(inv[g])) & 3) != 0)
            return std::string(who) + ": misaligned pointer in a group (planes 16-byte aligned, scale and inv 4)";
    }
    for (int g = 0; g < groups; g++) {
        const void* dst[3] = {planes[g], scale[g], inv[g]};
        for (int k = 0; k < 3; k++) {
            if (!dst[k]) continue;
            for (int l = k + 1; l < 3; l++)
                if (dst[k] == dst[l]) return std::string(who) + ": two destinations share an address";
            for (int q = 0; q < groups; q++) {
                const void* src[4] = {z[q], bias[q], gamma[q], beta[q]};
                for (int l = 0; l < 4; l++)
                    if (dst[k] == src[l]) return std::string(who) + ": a destination (planes, scale, inv) must not be a source (z, bias, gamma, beta)";
                if (dst[k] == y[q] || dst[k] == stat[q]) return std::string(who) + ": two destinations share an address (planes, scale, inv against y, stat)";
                if (q == g) continue;
                const void* other[3] = {planes[q], scale[q], inv[q]};
                for (int l = 0; l < 3; l++)
                    if (dst[k] == other[l]) return std::string(who) + ": two groups share a destination";
            }
        }
    }
    return {};
}

// mms_elu_ln_grad_group: ws_bytes and the shapes first (workspace NULL is the size query: nothing else is read), then as above.
// `need`: the build's workspace size (the CPU build: 0).
static inline std::string check_elu_ln_grad_group(int32_t groups, int64_t M, int32_t H, const float* const* z, int64_t z_pitch, const float* const* bias,
                                                  const float* const* gamma, const float* const* stat, const float* const* dy, int64_t dy_pitch,
                                                  float* const* dz, int64_t dz_pitch, float* const* dparams, const void* workspace, const int64_t* ws_bytes,
                                                  int64_t need) {
    const char* who = "mms_elu_ln_grad_group";
    std::string bad = check_groups(who, groups);
    if (!bad.empty()) return bad;
    if (!ws_bytes) return std::string(who) + ": ws_bytes required";
    if (!elu_ln_shapes(groups, M, H)) return std::string(who) + ": bad shapes (0 <= M <= 2147483647, H a positive multiple of 4, H <= 1024)";
    if (!workspace) return {};
    if (!z || !bias || !gamma || !stat || !dy || !dz) return std::string(who) + ": null pointer (z, bias, gamma, stat, dy and dz are required)";
    if (z_pitch < H || dy_pitch < H || dz_pitch < H || (z_pitch % 4) != 0 || (dy_pitch % 4) != 0 || (dz_pitch % 4) != 0)
        return std::string(who) + ": bad pitches (z_pitch, dy_pitch, dz_pitch >= H, each a multiple of 4)";
    if (*ws_bytes < need) return std::string(who) + ": workspace too small (" + std::to_string(*ws_bytes) + " bytes, needs " + std::to_string(need) + ")";
    if (addr(workspace) & 255) return std::string(who) + ": workspace must be 256-byte aligned";
    for (int g = 0; g < groups; g++) {
        if (!z[g] || !bias[g] || !gamma[g] || !stat[g] || !dy[g] || !dz[g]) return std::string(who) + ": null pointer in a group";
        if (((addr(z[g]) | addr(bias[g]) | addr(gamma[g]) | addr(dy[g]) | addr(dz[g])) & 15) != 0 || (addr(stat[g]) & 7) != 0 ||
            ((dparams ? addr(dparams[g]) : 0) & 3) != 0)
            return std::string(who) + ": misaligned pointer in a group (z, bias, gamma, dy, dz 16-byte aligned, stat 8, dparams 4)";
    }
    for (int g = 0; g < groups; g++) {
        const float* dst[2] = {dz[g], dparams ? dparams[g] : nullptr};
        if (dst[0] == dst[1]) return std::string(who) + ": two destinations share an address";
        for (int k = 0; k < 2; k++) {
            if (!dst[k]) continue;
            for (int q = 0; q < groups; q++) {
                const float* src[5] = {z[q], bias[q], gamma[q], stat[q], dy[q]};
                for (int l = 0; l < 5; l++)
                    if (dst[k] == src[l]) return std::string(who) + ": a destination (dz, dparams) must not be a source (z, bias, gamma, stat, dy)";
                if (q == g) continue;
                if (dst[k] == dz[q] || (dparams && dst[k] == dparams[q])) return std::string(who) + ": two groups share a destination";
            }
        }
    }
    return {};
}

// the shapes of mms_marl_heads_fwd_group and mms_marl_heads_grad_group (A: HOST array)
static inline std::string check_marl_heads_shapes(const char* who, int32_t groups, int64_t M, int32_t H, const int32_t* A) {
    std::string bad = check_groups(who, groups);
    if (!bad.empty()) return bad;
    if (M < 0 || M > 0x7fffffff || H < 4 || (H % 4) != 0 || H > 1024)
        return std::string(who) + ": bad shapes (0 <= M <= 2147483647, H a positive multiple of 4, H <= 1024)";
    if (!A) return std::string(who) + ": null pointer (A is required)";
    for (int g = 0; g < groups; g++)
        if (A[g] < 1 || A[g] > 16) return std::string(who) + ": A[g] must be 1..16, got " + std::to_string(A[g]);
    return {};
}

// mms_marl_heads_fwd_group: shapes, the pitch, then per group the pointers, their alignment and every destination against every source
// and every other destination over all groups
static inline std::string check_marl_heads_fwd_group(int32_t groups, int64_t M, int32_t H, const float* const* f, int64_t f_pitch, const float* const* w,
                                                     const float* const* b, const int32_t* A, const float* const* log_std, float x_coef,
                                                     float* const* out, float* const* std_out) {
    const char* who = "mms_marl_heads_fwd_group";
    std::string bad = check_marl_heads_shapes(who, groups, M, H, A);
    if (!bad.empty()) return bad;
    if (!f || !w || !b || !out) return std::string(who) + ": null pointer (f, w, b and out are required)";
    if (f_pitch < H || (f_pitch % 4) != 0) return std::string(who) + ": bad pitch (f_pitch >= H, a multiple of 4)";
    if (log_std && (!std_out || !(x_coef != 0.f))) return std::string(who) + ": log_std needs std and a non-zero x_coef";
    for (int g = 0; g < groups; g++) {
        if (!f[g] || !w[g] || !b[g] || !out[g] || (log_std && log_std[g] && !std_out[g])) return std::string(who) + ": null pointer in a group";
        if (((addr(f[g]) | addr(w[g])) & 15) != 0 || ((addr(b[g]) | addr(out[g]) | (log_std ? addr(log_std[g]) | addr(std_out[g]) : 0)) & 3) != 0)
            return std::string(who) + ": misaligned pointer in a group (f, w 16-byte aligned, b, log_std, out, std 4)";
    }
    for (int g = 0; g < groups; g++) {
        const float* dst[2] = {out[g], log_std && log_std[g] ? std_out[g] : nullptr};
        if (dst[0] == dst[1]) return std::string(who) + ": two destinations share an address";
        for (int k = 0; k < 2; k++) {
            if (!dst[k]) continue;
            for (int q = 0; q < groups; q++) {
                const float* src[4] = {f[q], w[q], b[q], log_std ? log_std[q] : nullptr};
                for (int l = 0; l < 4; l++)
                    if (dst[k] == src[l]) return std::string(who) + ": a destination (out, std) must not be a source (f, w, b, log_std)";
                if (q == g) continue;
                if (dst[k] == out[q] || (log_std && log_std[q] && dst[k] == std_out[q])) return std::string(who) + ": two groups share a destination";
            }
        }
    }
    return {};
}

// mms_marl_heads_grad_group: ws_bytes and the shapes first (workspace NULL is the size query: nothing but A is read), then as above.
// `need`: the build's workspace size (the CPU build: 0).
static inline std::string check_marl_heads_grad_group(int32_t groups, int64_t M, int32_t H, const float* const* f, int64_t f_pitch, const float* const* w,
                                                      const int32_t* A, const float* const* dout, const float* const* log_std, const float* const* dstd,
                                                      float x_coef, float* const* df, int64_t df_pitch, float* const* dw, float* const* db,
                                                      float* const* dlog_std, const void* workspace, const int64_t* ws_bytes, int64_t need) {
    const char* who = "mms_marl_heads_grad_group";
    std::string bad = check_marl_heads_shapes(who, groups, M, H, A);
    if (!bad.empty()) return bad;
    if (!ws_bytes) return std::string(who) + ": ws_bytes required";
    if (!workspace) return {};
    if (!f || !w || !dout) return std::string(who) + ": null pointer (f, w and dout are required)";
    if ((dw == nullptr) != (db == nullptr)) return std::string(who) + ": dw and db are given together or not at all";
    if (f_pitch < H || (f_pitch % 4) != 0 || (df && (df_pitch < H || (df_pitch % 4) != 0)))
        return std::string(who) + ": bad pitches (f_pitch, df_pitch >= H, each a multiple of 4)";
    if (dlog_std && (!log_std || !dstd || !(x_coef != 0.f))) return std::string(who) + ": dlog_std needs log_std, dstd and a non-zero x_coef";
    if (*ws_bytes < need) return std::string(who) + ": workspace too small (" + std::to_string(*ws_bytes) + " bytes, needs " + std::to_string(need) + ")";
    if (addr(workspace) & 255) return std::string(who) + ": workspace must be 256-byte aligned";
    const auto at = [](float* const* t, int g) -> float* { return t ? t[g] : nullptr; };
    for (int g = 0; g < groups; g++) {
        if (!f[g] || !w[g] || !dout[g]) return std::string(who) + ": null pointer in a group";
        if ((at(dw, g) == nullptr) != (at(db, g) == nullptr)) return std::string(who) + ": dw_g and db_g are given together or not at all";
        if (at(dlog_std, g) && (!log_std[g] || !dstd[g])) return std::string(who) + ": dlog_std_g needs log_std_g and dstd_g";
        if (((addr(f[g]) | addr(w[g]) | addr(at(df, g))) & 15) != 0 ||
            ((addr(dout[g]) | addr(at(dw, g)) | addr(at(db, g)) | addr(at(dlog_std, g)) | (log_std ? addr(log_std[g]) : 0) | (dstd ? addr(dstd[g]) : 0)) & 3) != 0)
            return std::string(who) + ": misaligned pointer in a group (f, w, df 16-byte aligned, the others 4)";
    }
    for (int g = 0; g < groups; g++) {
        const float* dst[4] = {at(df, g), at(dw, g), at(db, g), at(dlog_std, g)};
        for (int k = 0; k < 4; k++) {
            if (!dst[k]) continue;
            for (int l = k + 1; l < 4; l++)
                if (dst[k] == dst[l]) return std::string(who) + ": two destinations share an address";
            for (int q = 0; q < groups; q++) {
                const float* src[5] = {f[q], w[q], dout[q], log_std ? log_std[q] : nullptr, dstd ? dstd[q] : nullptr};
                for (int l = 0; l < 5; l++)
                    if (dst[k] == src[l]) return std::string(who) + ": a destination (df, dw, db, dlog_std) must not be a source (f, w, dout, log_std, dstd)";
                if (q == g) continue;
                const float* other[4] = {at(df, q), at(dw, q), at(db, q), at(dlog_std, q)};
                for (int l = 0; l < 4; l++)
                    if (dst[k] == other[l]) return std::string(who) + ": two groups share a destination";
            }
        }
    }
    return {};
}

// mms_mlp_grad and mms_mlp_grad_rop: the shapes, then (workspace NULL is the size query: nothing else is read) the operands.  The
// workspace's size and alignment are the HIP build's own; the CPU build needs none.
static inline std::string check_mlp_shapes(const char* entry, int32_t layers, int64_t M, const int32_t* dims, const int64_t* ws_bytes) {
    bool ok = dims && ws_bytes && layers >= 2 && layers <= mms::kMlpMaxLayers && M >= 1 && M <= mms::kMlpMaxRows;
    for (int l = 0; ok && l <= layers; l++) ok = dims[l] >= 1 && dims[l] <= 65536;
    if (ok) return {};
    return std::string(entry) + ": bad arguments (2 <= layers <= " + std::to_string(mms::kMlpMaxLayers) + ", 1 <= M <= " + std::to_string(mms::kMlpMaxRows) +
           ", dims[0..layers] in 1..65536, ws_bytes required)";
}

static inline std::string check_mlp_grad(int32_t layers, int64_t M, const int32_t* dims, const float* x, const float* const* h, const float* const* w,
                                         const float* g, float* const* dw, float* const* db, float* const* d_out, float* const* e_out,
                                         const void* workspace, const int64_t* ws_bytes) {
    std::string bad = check_mlp_shapes("mms_mlp_grad", layers, M, dims, ws_bytes);
    if (!bad.empty() || !workspace) return bad;
    if (!x || !g || !all_set(layers - 1, h) || !all_set(layers, w) || !all_set(layers, dw) || !all_set(layers, db) ||
        (d_out && !all_set(layers - 1, d_out)) || (e_out && !all_set(layers - 1, e_out)))
        return "mms_mlp_grad: null pointer (x, g, h[layers-1], w / dw / db[layers]; d_out / e_out all or none)";
    return {};
}

static inline std::string check_mlp_grad_rop(int32_t layers, int64_t M, const int32_t* dims, const float* x, const float* const* h, const float* const* w,
                                             const float* const* v, const float* const* c, const float* g, const float* const* d,
                                             const float* const* e, const float* rmu, float* const* rdw, float* const* rdb, const void* workspace,
                                             const int64_t* ws_bytes) {
    std::string bad = check_mlp_shapes("mms_mlp_grad_rop", layers, M, dims, ws_bytes);
    if (!bad.empty() || !workspace) return bad;
    if (!x || !g || !rmu || !all_set(layers - 1, h) || !all_set(layers, w) || !all_set(layers, v) || !all_set(layers, c) || !all_set(layers - 1, d) ||
        !all_set(layers - 1, e) || !all_set(layers, rdw) || !all_set(layers, rdb))
        return "mms_mlp_grad_rop: null pointer (x, g, rmu, h / d / e[layers-1], w / v / c / rdw / rdb[layers])";
    return {};
}

// mms_ln_mlp_grad and mms_ln_mlp_jvp: the shapes, then (workspace NULL is the size query: nothing else is read) the operands, then the
// workspace against `need`, which is each build's own.
static inline std::string check_ln_mlp_shapes(const char* entry, int32_t blocks, int64_t M, const int32_t* dims, const int64_t* ws_bytes) {
    bool ok = dims && ws_bytes && blocks >= 1 && blocks <= MMS_LN_MLP_MAX_BLOCKS && M >= 1 && M <= mms::kMlpMaxRows;
    for (int l = 0; ok && l <= blocks; l++) ok = dims[l] >= 1 && dims[l] <= MMS_LN_MLP_MAX_WIDTH;
    ok = ok && dims[blocks + 1] >= 1 && dims[blocks + 1] <= MMS_LN_MLP_MAX_A;
    if (ok) return {};
    return std::string(entry) + ": bad arguments (1 <= blocks <= " + std::to_string(MMS_LN_MLP_MAX_BLOCKS) + ", 1 <= M <= " + std::to_string(mms::kMlpMaxRows) +
           ", dims[0..blocks] in 1.." + std::to_string(MMS_LN_MLP_MAX_WIDTH) + ", dims[blocks+1] in 1.." + std::to_string(MMS_LN_MLP_MAX_A) +
           ", ws_bytes required)";
}

static inline std::string check_ln_mlp_workspace(const char* entry, const void* workspace, const int64_t* ws_bytes, int64_t need) {
    if (*ws_bytes < need) return std::string(entry) + ": workspace too small (" + std::to_string(*ws_bytes) + " bytes, needs " + std::to_string(need) + ")";
    if (addr(workspace) & 255) return std::string(entry) + ": workspace must be 256-byte aligned";
    return {};
}

// the CPU build's workspace: the row statistics (mean, rstd) of every level, in double
static inline int64_t ln_mlp_cpu_ws_bytes(int32_t blocks, int64_t M) { return (((int64_t)(blocks + 1) * M * 2 * 8) + 255) / 256 * 256; }

static inline std::string check_ln_mlp_grad(int32_t blocks, int64_t M, const int32_t* dims, float eps, const float* x, const float* const* h,
                                            const float* const* ln_g, const float* const* ln_t, const float* const* w, const float* g,
                                            float* const* dln_g, float* const* dln_t, float* const* dw, float* const* db, const void* workspace,
                                            const int64_t* ws_bytes, int64_t need) {
    std::string bad = check_ln_mlp_shapes("mms_ln_mlp_grad", blocks, M, dims, ws_bytes);
    if (!bad.empty() || !workspace) return bad;
    if (!(eps >= 0.f)) return "mms_ln_mlp_grad: eps must not be negative";
    if (!x || !g || !all_set(blocks, h) || !all_set(blocks + 1, ln_g) || !all_set(blocks + 1, ln_t) || !all_set(blocks + 1, w) ||
        !all_set(blocks + 1, dln_g) || !all_set(blocks + 1, dln_t) || !all_set(blocks + 1, dw) || !all_set(blocks + 1, db))
        return "mms_ln_mlp_grad: null pointer (x, g, h[blocks], ln_g / ln_t / w / dln_g / dln_t / dw / db[blocks+1])";
    return check_ln_mlp_workspace("mms_ln_mlp_grad", workspace, ws_bytes, need);
}

static inline std::string check_ln_mlp_jvp(int32_t blocks, int64_t M, const int32_t* dims, float eps, const float* x, const float* const* h,
                                           const float* const* ln_g, const float* const* ln_t, const float* const* w, const float* const* vg,
                                           const float* const* vt, const float* const* vw, const float* const* vc, const float* rmu,
                                           const void* workspace, const int64_t* ws_bytes, int64_t need) {
    std::string bad = check_ln_mlp_shapes("mms_ln_mlp_jvp", blocks, M, dims, ws_bytes);
    if (!bad.empty() || !workspace) return bad;
    if (!(eps >= 0.f)) return "mms_ln_mlp_jvp: eps must not be negative";
    if (!x || !rmu || !all_set(blocks, h) || !all_set(blocks + 1, ln_g) || !all_set(blocks + 1, ln_t) || !all_set(blocks + 1, w) ||
        !all_set(blocks + 1, vg) || !all_set(blocks + 1, vt) || !all_set(blocks + 1, vw) || !all_set(blocks + 1, vc))
        return "mms_ln_mlp_jvp: null pointer (x, rmu, h[blocks], ln_g / ln_t / w / vg / vt / vw / vc[blocks+1])";
    return check_ln_mlp_workspace("mms_ln_mlp_jvp", workspace, ws_bytes, need);
}

// ---- mms_param_step ---------------------------------------------------------------------------------------------------------------

static inline int64_t param_chunks(int64_t numel) { return (numel + mms::kParamChunk - 1) / mms::kParamChunk; }

// mms_param_step_partials: the doubles of the `partials` workspace (0 for bad arguments; at least 1 otherwise)
static inline int64_t param_step_partials(int32_t tensors, const int64_t* numel) {
    if (tensors < 0 || tensors > MMS_PARAM_MAX_TENSORS || (tensors > 0 && !numel)) return 0;
    int64_t n = 0;
    for (int t = 0; t < tensors; t++) {
        if (numel[t] < 0) return 0;
        n += param_chunks(numel[t]);
    }
    return n > 0 ? n : 1;
}

// all checks before any work
static inline std::string check_param_step(int32_t tensors, const int64_t* numel, float* const* param, const float* const* grad, float* const* exp_avg,
                                           float* const* exp_avg_sq, float* const* target, double lr, double beta1, double beta2, double eps,
                                           double weight_decay, int64_t step, double max_norm, double polyak, int32_t flags, const double* partials,
                                           const float* norm_out) {
    if (tensors < 0 || tensors > MMS_PARAM_MAX_TENSORS) return "mms_param_step: tensors must be 0.." + std::to_string(MMS_PARAM_MAX_TENSORS);
    if (step < 1) return "mms_param_step: step must be >= 1 (the step number after this call)";
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return "mms_param_step: beta1 and beta2 must lie in [0, 1)";
    if (!(lr >= 0.0 && lr <= DBL_MAX) || !(eps >= 0.0 && eps <= DBL_MAX) || !(weight_decay >= 0.0 && weight_decay <= DBL_MAX))
        return "mms_param_step: lr, eps and weight_decay must be finite and not negative";
    if (flags != 0) return "mms_param_step: flags is reserved and must be 0";
    if (tensors > 0 && !numel) return "mms_param_step: numel required";
    int64_t chunks = 0;
    bool any_target = false;
    for (int t = 0; t < tensors; t++) {
        const float* p = param ? param[t] : nullptr;
        const float* g = grad ? grad[t] : nullptr;
        const float* m = exp_avg ? exp_avg[t] : nullptr;
        const float* v = exp_avg_sq ? exp_avg_sq[t] : nullptr;
        const float* tg = target ? target[t] : nullptr;
        if (numel[t] < 0) return "mms_param_step: negative numel";
        chunks += param_chunks(numel[t]);
        if (chunks > 0x7fffffff) return "mms_param_step: more than 2^31 - 1 chunks";
        if ((m != nullptr) != (v != nullptr)) return "mms_param_step: exp_avg and exp_avg_sq go together (both, or both NULL)";
        if (p && g && !m) return "mms_param_step: a tensor with param and grad needs its moments (exp_avg, exp_avg_sq)";
        if (tg && !p) return "mms_param_step: a target needs its param";
        if ((addr(p) | addr(g) | addr(m) | addr(v) | addr(tg)) & 3) return "mms_param_step: pointers must be 4-byte aligned";
        any_target = any_target || tg;
    }
    if (any_target && !(polyak == polyak)) return "mms_param_step: polyak is NaN";
    if (max_norm > 0.0 || norm_out) {
        if (!partials) return "mms_param_step: a norm (max_norm > 0 or norm_out) needs the partials workspace";
        if (addr(partials) & 7) return "mms_param_step: partials must be 8-byte aligned";
    }
    if (addr(norm_out) & 3) return "mms_param_step: norm_out must be 4-byte aligned";
    return {};
}

// The argument block of a checked call: the pointers (NULL arrays resolved, moments cleared where there is no Adam step), the two
// chunk tables and the scalars.  norm_first / step_first [tensors] are the launches' chunk counts.
static inline mms::ParamArgs build_param_args(int32_t tensors, const int64_t* numel, float* const* param, const float* const* grad, float* const* exp_avg,
                                              float* const* exp_avg_sq, float* const* target, double lr, double beta1, double beta2, double eps,
                                              double weight_decay, int64_t step, double max_norm, double polyak, double* partials, float* norm_out) {
    mms::ParamArgs a = {};
    a.tensors = tensors;
    a.use_norm = (max_norm > 0.0 || norm_out) ? 1 : 0;
    int32_t nf = 0, sf = 0;
    for (int t = 0; t < tensors; t++) {
        a.p[t] = param ? param[t] : nullptr;
        a.g[t] = grad ? grad[t] : nullptr;
        const bool adam = a.p[t] && a.g[t];
        a.m[t] = adam ? exp_avg[t] : nullptr;
        a.v[t] = adam ? exp_avg_sq[t] : nullptr;
        a.t[t] = target ? target[t] : nullptr;
        a.numel[t] = numel[t];
        a.norm_first[t] = nf;
        a.step_first[t] = sf;
        const int32_t chunks = (int32_t)param_chunks(numel[t]);
        if (a.use_norm && a.g[t]) nf += chunks;
        if (a.p[t] && (adam || a.t[t])) sf += chunks;
    }
    for (int t = tensors; t <= mms::kParamMaxTensors; t++) { a.norm_first[t] = nf; a.step_first[t] = sf; }
    a.c = mms::param_coef(lr, beta1, beta2, eps, weight_decay, step, polyak);
    a.max_norm = (float)max_norm;
    a.partials = partials;
    a.norm_out = norm_out;
    return a;
}
