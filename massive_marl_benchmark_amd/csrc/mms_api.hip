// mms_api.hip -- the C ABI of include/mms.h: engine lifetime, named device buffers, launches.
// Host side only allocates, fills the construction-time scene (what create_sim .. prepare_sim do in the
// reference, agents/tasks/ten_ant.py:205-633) and enqueues kernels on the caller's stream.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include "mms_host.h"
#include "policy_args.h"
#include "step_args.h"
#include "trpo_plan.h"
#include "ln_mlp_plan.h"
#include "maddpg_args.h"
#include "gru_args.h"
#include "gru_gates_args.h"
#include "gru_grad_args.h"
#include "elu_ln_args.h"
#include "marl_heads_grad_args.h"
#include "marl_eval_args.h"

namespace mms {
hipError_t launch_step(const StepArgs& a, int task, hipStream_t stream);
bool step_layout_takes_head(int task, int num_envs, int num_agents, int packing);
hipError_t launch_gae_ppo(const float*, const uint8_t*, const float*, const float*, float*, float*, double*, int, int64_t, float, float, hipStream_t);
hipError_t launch_adv_normalize(float*, const double*, int64_t, hipStream_t);
hipError_t launch_gae_ppo_normalized(const float*, const uint8_t*, const float*, const float*, float*, float*, double*, int, int64_t, float, float, hipStream_t);
hipError_t launch_gae_marl(const float*, const float*, const float*, float*, int, int64_t, float, float, int, const float*, const float*, hipStream_t);
hipError_t launch_marl_views(const float*, float*, int64_t, int, int, int, hipStream_t);
hipError_t launch_gae_marl_agents(const float*, const float*, const float*, float*, int, int64_t, int, float, float, int, const float*, const float*, hipStream_t);
hipError_t launch_ppo_act(const float*, const float*, const float*, uint64_t, int64_t*, int64_t, int, float*, float*, float*, float*, float*, float*, int64_t, int, hipStream_t);
hipError_t launch_ppo_head_act(const float*, const float*, const float*, int, const float*, const float*, const float*, const float*, int, const float*, uint64_t,
                               int64_t*, int64_t, int, float*, float*, float*, float*, float*, float*, int64_t, int, hipStream_t);
hipError_t launch_sac_head_act(const float*, int, const float*, const float*, const float*, const float*, float, float, int, uint64_t, int64_t*, int64_t,
                               float*, float*, float*, float*, float*, float*, int64_t, int, hipStream_t);
hipError_t launch_q_heads_backup(int, int64_t, int, const float* const*, const float* const*, const float* const*, float* const*, const float*,
                                 const uint8_t*, const float*, float, float, float*, hipStream_t);
int64_t ppo_loss_ws_bytes(int64_t, int);
hipError_t launch_ppo_loss(int64_t, int, const float*, const float*, const float*, const int64_t*, const float*, const float*, const float*, const float*,
                           const float*, const float*, const float*, float, float, float, int, float*, float*, float*, float*, void*, hipStream_t);
int64_t trpo_heads_ws_bytes(int64_t, int);
hipError_t launch_trpo_heads(int64_t, int, const float*, const float*, const float*, const int64_t*, const float*, const float*, const float*, const float*,
                             const float*, int, float*, float*, float*, float*, float*, void*, hipStream_t);
int64_t marl_loss_ws_bytes(int64_t, int);
hipError_t launch_marl_ppo_loss(int64_t, int, const float*, const float*, const float*, const int64_t*, const mms_marl_loss_fields&, float, float, float,
                                float, int, int, int, int, int, const float*, const float*, float*, float*, float*, float*, float*, void*, hipStream_t);
int64_t marl_loss_group_ws_bytes(int, int64_t, int);
hipError_t launch_marl_ppo_loss_group(int, int64_t, int, const mms_marl_loss_group*, float, float, float, float, int, int, int, int, int, void*, hipStream_t);
hipError_t launch_param_step(const ParamArgs&, hipStream_t);
int64_t sac_grad_ws_bytes(int64_t, int);
hipError_t launch_sac_heads_grad(int64_t, int, float, float, const float*, const float*, const float*, const float*, const float*, float*, float*, void*,
                                 hipStream_t);
int64_t det_grad_ws_bytes(int64_t, int);
hipError_t launch_det_heads_grad(int64_t, int, float, const float*, const float*, int64_t, float*, float*, void*, hipStream_t);
int64_t q_loss_ws_bytes(int64_t, int, int);
hipError_t launch_q_heads_loss(int, int64_t, int, const float* const*, const float* const*, const float* const*, int, const float*, const float*, float,
                               float, float*, float* const*, float* const*, float* const*, float* const*, void*, hipStream_t);
struct MlpPlan;
}  // namespace mms

struct mms_engine : mms_host_state {
    mms_config* d_cfg = nullptr;
    void* scratch = nullptr;                // staging of mms_set_state(env_ids)
    size_t scratch_bytes = 0;
    int packing = 1;
};

// Every entry point that touches the GPU runs on ITS device (the engine's, or the `device` argument) and leaves the caller's
// current device as it found it: two engines in one process, or a torch current device other than the engine's, must not make a
// launch pick another device's stream or caches, and torch allocations after a call must not move GPU.
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) { err = hipSetDevice(device); changed = (err == hipSuccess); }
    }
    ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
};

#define MMS_HIP(e, call)                                                                              \
    do {                                                                                              \
        hipError_t err_ = (call);                                                                     \
        if (err_ != hipSuccess) return fail(e, std::string(#call) + ": " + hipGetErrorString(err_));  \
    } while (0)

// rows of a per-env buffer scattered to their env slots in one launch (mms_set_state with env ids): block = row, 4-byte words
__global__ void __launch_bounds__(256) scatter_rows_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, const int64_t* __restrict__ ids,
                                                           int64_t row_words) {
    const int64_t i = blockIdx.x;
    uint32_t* d = dst + ids[i] * row_words;
    const uint32_t* s = src + i * row_words;
    for (int64_t k = threadIdx.x; k < row_words; k += 256) d[k] = s[k];
}

static std::string config_device_error(int device) {
    if (device < 0) return "mms_create: this is the HIP build of the engine (no CPU fallback); device must be a HIP ordinal >= 0 -- device -1 is served by libmms_cpu.so, an explicit opt-in";
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return "mms_create: no HIP device available (no CPU fallback)";
    if (device >= ndev) return "mms_create: device ordinal out of range";
    return {};
}

extern "C" {

__attribute__((visibility("default"))) int mms_abi_version(void) { return MMS_ABI_VERSION; }

__attribute__((visibility("default"))) const char* mms_last_error(mms_handle h) { return h ? h->err.c_str() : g_error.c_str(); }

__attribute__((visibility("default"))) int mms_create(const mms_config* cfg, mms_handle* out) {
    mms_engine* e = new mms_engine();
    std::string bad = engine_init(e, cfg, out);
    if (bad.empty()) bad = config_device_error(cfg->device);
    if (!bad.empty()) { delete e; return fail(nullptr, bad); }
    DeviceGuard guard(cfg->device);
    hipError_t he = guard.err;
    if (const char* pk = getenv("MMS_PACKING")) e->packing = atoi(pk);   // A/B switch for profiling
    e->bufs = buffer_table(*e);
    for (auto& b : e->bufs) {
        const size_t alloc = b.bytes ? b.bytes : 16;
        if (he == hipSuccess) he = hipMalloc(&b.ptr, alloc);
        if (he == hipSuccess) he = hipMemset(b.ptr, 0, alloc);
    }
    // construction-time scene (host), uploaded once
    const size_t N = (size_t)cfg->num_envs, A = (size_t)cfg->num_agents;
    std::vector<float> init(N * e->actors * 13, 0.f), origin(N * 3, 0.f), prev(N * e->prev_dim, 0.f), dr(N * A * MMS_DR_FLOATS, 0.f);
    std::vector<int64_t> reset(N, 0);
    fill_scene(*e, init.data(), origin.data(), prev.data(), reset.data(), dr.data());
    auto up = [&](const char* name, const void* src, size_t bytes) {
        if (he == hipSuccess) he = hipMemcpy(find(e, name)->ptr, src, bytes, hipMemcpyHostToDevice);
    };
    up("initial_root_states", init.data(), init.size() * 4);
    up("root_states", init.data(), init.size() * 4);
    up("env_origin", origin.data(), origin.size() * 4);
    up("prev", prev.data(), prev.size() * 4);
    up("reset", reset.data(), reset.size() * 8);
    up("dr_params", dr.data(), dr.size() * 4);
    if (he == hipSuccess) he = hipMalloc((void**)&e->d_cfg, sizeof(mms_config));
    if (he == hipSuccess) he = hipMemcpy(e->d_cfg, &e->cfg, sizeof(mms_config), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he != hipSuccess) { g_error = std::string("mms_create: ") + hipGetErrorString(he); mms_destroy(e); return 1; }
    *out = e;
    return 0;
}

__attribute__((visibility("default"))) int mms_destroy(mms_handle h) {
    if (!h) return 0;
    DeviceGuard guard(h->cfg.device);                  // teardown: nothing useful to do with an error here
    (void)hipDeviceSynchronize();
    for (auto& b : h->bufs)
        if (b.ptr) (void)hipFree(b.ptr);
    if (h->d_cfg) (void)hipFree(h->d_cfg);
    if (h->scratch) (void)hipFree(h->scratch);
    delete h;
    return 0;
}

__attribute__((visibility("default"))) int mms_get_tensor(mms_handle h, const char* name, mms_tensor* out) { return host_get_tensor(h, name, out); }

static mms::StepArgs step_args(mms_handle h, int physics) {
    mms::StepArgs a{};
    a.cfg = h->d_cfg;
    a.actions = h->actions_in ? h->actions_in : (const float*)find(h, "actions")->ptr;
    a.obs = h->write_raw_obs ? (float*)find(h, "obs")->ptr : nullptr;
    a.obs_clipped = h->write_clipped_obs ? (float*)find(h, "obs_clipped")->ptr : nullptr;
    a.obs_out = h->obs_out;
    a.obs_planes = h->obs_planes; a.obs_planes_scale = h->obs_planes_scale;
    a.rew_out = h->rew_out;
    a.done_out = h->done_out;
    a.rew = (float*)find(h, "rew")->ptr;
    a.reset = (int64_t*)find(h, "reset")->ptr;
    a.progress = (int64_t*)find(h, "progress")->ptr;
    a.root_states = (float*)find(h, "root_states")->ptr;
    a.initial_root_states = (const float*)find(h, "initial_root_states")->ptr;
    a.dof_state = (float*)find(h, "dof_state")->ptr;
    a.env_origin = (const float*)find(h, "env_origin")->ptr;
    a.prev = (float*)find(h, "prev")->ptr;
    a.reset_noise = (const float*)find(h, "reset_noise")->ptr;
    a.foot_sensors = (float*)find(h, "foot_sensors")->ptr;
    a.reset_count = (int64_t*)find(h, "reset_count")->ptr;
    a.dr = h->dr_enabled ? (const float*)find(h, "dr_params")->ptr : nullptr;
    a.do_physics = physics;
    a.num_envs = h->cfg.num_envs;
    a.num_agents = h->cfg.num_agents;
    a.obs_dim = h->obs_dim;
    a.prev_dim = h->prev_dim;
    a.packing = h->packing;
    a.head_on = (physics && h->head_on) ? 1 : 0;
    if (a.head_on) a.head = h->head;
    return a;
}

static int do_step(mms_handle h, void* stream, int physics) {
    if (null_handle(h, "mms_step")) return 1;
    DeviceGuard guard(h->cfg.device);
    MMS_HIP(h, guard.err);
    mms::StepArgs a = step_args(h, physics);
    if (physics) h->head_on = false;                                  // the binding is for one step (the slot pointers move every step)
    MMS_HIP(h, mms::launch_step(a, h->cfg.task, (hipStream_t)stream));
    return 0;
}
__attribute__((visibility("default"))) int mms_step(mms_handle h, void* hip_stream) { return do_step(h, hip_stream, 1); }
__attribute__((visibility("default"))) int mms_post_step(mms_handle h, void* hip_stream) { return do_step(h, hip_stream, 0); }

__attribute__((visibility("default"))) int mms_reset_all(mms_handle h, void* hip_stream) {
    if (null_handle(h, "mms_reset_all")) return 1;
    DeviceGuard guard(h->cfg.device);
    MMS_HIP(h, guard.err);
    std::vector<int64_t> ones((size_t)h->cfg.num_envs, 1);
    MMS_HIP(h, hipMemcpyAsync(find(h, "reset")->ptr, ones.data(), ones.size() * 8, hipMemcpyHostToDevice, (hipStream_t)hip_stream));
    MMS_HIP(h, hipStreamSynchronize((hipStream_t)hip_stream));   // `ones` is a temporary
    return 0;
}

__attribute__((visibility("default"))) int mms_set_state(mms_handle h, const char* name, const void* src, int src_is_host, const int64_t* env_ids, int64_t n, void* hip_stream) {
    mms_buffer* b = nullptr;
    if (host_set_state_check(h, name, src, env_ids, n, &b)) return 1;
    DeviceGuard guard(h->cfg.device);
    MMS_HIP(h, guard.err);
    hipStream_t s = (hipStream_t)hip_stream;
    hipMemcpyKind kind = src_is_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (!env_ids) {
        MMS_HIP(h, hipMemcpyAsync(b->ptr, src, b->bytes, kind, s));
    } else {
        if (n <= 16 || (b->row_bytes & 3) != 0) {
            for (int64_t i = 0; i < n; i++)
                MMS_HIP(h, hipMemcpyAsync((char*)b->ptr + env_ids[i] * b->row_bytes, (const char*)src + i * b->row_bytes, (size_t)b->row_bytes, kind, s));
        } else {
            // the indexed setter of the reference (gym.set_*_tensor_indexed, ten_ant.py:867-875) takes thousands of ids: one scatter
            // launch instead of one copy per env.  Staging (ids, and the rows when they come from the host) lives in engine scratch.
            const size_t id_bytes = (size_t)n * 8, row_total = (size_t)n * (size_t)b->row_bytes;
            const size_t need = id_bytes + (src_is_host ? row_total : 0);
            if (need > h->scratch_bytes) {
                if (h->scratch) MMS_HIP(h, hipFree(h->scratch));
                h->scratch = nullptr; h->scratch_bytes = 0;
                MMS_HIP(h, hipMalloc(&h->scratch, need));
                h->scratch_bytes = need;
            }
            MMS_HIP(h, hipMemcpyAsync(h->scratch, env_ids, id_bytes, hipMemcpyHostToDevice, s));
            const void* rows = src;
            if (src_is_host) {
                MMS_HIP(h, hipMemcpyAsync((char*)h->scratch + id_bytes, src, row_total, hipMemcpyHostToDevice, s));
                rows = (char*)h->scratch + id_bytes;
            }
            hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)n), dim3(256), 0, s, (uint32_t*)b->ptr, (const uint32_t*)rows,
                               (const int64_t*)h->scratch, b->row_bytes / 4);
            MMS_HIP(h, hipGetLastError());
            MMS_HIP(h, hipStreamSynchronize(s));                 // env_ids is the caller's host array; the scratch is reused by the next call
        }
    }
    if (src_is_host) MMS_HIP(h, hipStreamSynchronize(s));
    return 0;
}

__attribute__((visibility("default"))) int mms_bind_obs_out(mms_handle h, void* dst) { return host_bind_obs_out(h, dst); }
__attribute__((visibility("default"))) int mms_bind_obs_planes16(mms_handle h, void* planes, float scale) { return host_bind_obs_planes16(h, planes, scale); }
__attribute__((visibility("default"))) int mms_bind_actions(mms_handle h, const float* src) { return host_bind_actions(h, src); }
__attribute__((visibility("default"))) int mms_set_dr(mms_handle h, int32_t enable) { return host_set_dr(h, enable); }
__attribute__((visibility("default"))) int mms_set_obs_outputs(mms_handle h, int32_t raw, int32_t clipped) { return host_set_obs_outputs(h, raw, clipped); }
__attribute__((visibility("default"))) int mms_bind_rollout_out(mms_handle h, float* rew_out, uint8_t* done_out) { return host_bind_rollout_out(h, rew_out, done_out); }

__attribute__((visibility("default"))) int mms_bind_policy_head(mms_handle h, const mms_policy_head* head) {
    bool takes = false;
    if (h && head) {                                                  // the layout depends on the device's CU count
        DeviceGuard guard(h->cfg.device);
        MMS_HIP(h, guard.err);
        takes = mms::step_layout_takes_head(h->cfg.task, h->cfg.num_envs, h->cfg.num_agents, h->packing);
    }
    return host_bind_policy_head(h, head, takes);
}

#define MMS_DEV(device)                                                                                \
    if ((device) < 0) { g_error = "no CPU path in this library: device must be a HIP ordinal (the CPU build is libmms_cpu.so)"; return 1; } \
    DeviceGuard guard_(device);                                                                        \
    if (guard_.err != hipSuccess) { g_error = std::string("hipSetDevice: ") + hipGetErrorString(guard_.err); return 1; }
#define MMS_FREE(call)                                                                                 \
    do {                                                                                               \
        hipError_t err_ = (call);                                                                      \
        if (err_ != hipSuccess) { g_error = std::string(#call) + ": " + hipGetErrorString(err_); return 1; } \
    } while (0)

__attribute__((visibility("default"))) int mms_marl_views(int device, const float* obs_clipped, float* obs_all, int64_t n, int32_t agents, int32_t per_agent, int32_t shared, void* s) {
    MMS_DEV(device)
    if (refused(check_marl_views(obs_clipped, obs_all, n, agents, per_agent, shared))) return 1;
    MMS_FREE(mms::launch_marl_views(obs_clipped, obs_all, n, agents, per_agent, shared, (hipStream_t)s));
    return 0;
}
__attribute__((visibility("default"))) int mms_gae_ppo(int device, const float* rewards, const uint8_t* dones, const float* values, const float* last_values, float* returns,
                float* advantages, double* stats, int32_t T, int64_t N, float gamma, float lam, void* s) {
    MMS_DEV(device)
    if (refused(check_gae_ppo(rewards, dones, values, last_values, returns, advantages, stats, T, N))) return 1;
    MMS_FREE(mms::launch_gae_ppo(rewards, dones, values, last_values, returns, advantages, stats, T, N, gamma, lam, (hipStream_t)s));
    return 0;
}
__attribute__((visibility("default"))) int mms_gae_ppo_normalized(int device, const float* rewards, const uint8_t* dones, const float* values, const float* last_values,
                                                                  float* returns, float* advantages, double* stats, int32_t T, int64_t N, float gamma, float lam, void* s) {
    MMS_DEV(device)
    if (refused(check_gae_ppo_normalized(rewards, dones, values, last_values, returns, advantages, stats, T, N))) return 1;
    MMS_FREE(mms::launch_gae_ppo_normalized(rewards, dones, values, last_values, returns, advantages, stats, T, N, gamma, lam, (hipStream_t)s));
    return 0;
}
__attribute__((visibility("default"))) int mms_adv_normalize(int device, float* advantages, const double* stats, int64_t count, void* s) {
    MMS_DEV(device)
    if (refused(check_adv_normalize(advantages, stats, count))) return 1;
    MMS_FREE(mms::launch_adv_normalize(advantages, stats, count, (hipStream_t)s));
    return 0;
}
__attribute__((visibility("default"))) int mms_gae_marl(int device, const float* rewards, const float* value_preds, const float* masks, float* returns, int32_t T, int64_t N,
                 float gamma, float lam, int32_t use_norm, const float* norm_mean, const float* norm_var, void* s) {
    MMS_DEV(device)
    if (refused(check_gae_marl("mms_gae_marl", rewards, value_preds, masks, returns, T, N, 1, use_norm, norm_mean, norm_var))) return 1;
    MMS_FREE(mms::launch_gae_marl(rewards, value_preds, masks, returns, T, N, gamma, lam, use_norm, norm_mean, norm_var, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_gae_marl_agents(int device, const float* rewards, const float* value_preds, const float* masks,
                                                               float* returns, int32_t T, int64_t N, int32_t A, float gamma, float lam,
                                                               int32_t use_norm, const float* norm_mean, const float* norm_var, void* s) {
    MMS_DEV(device)
    if (refused(check_gae_marl("mms_gae_marl_agents", rewards, value_preds, masks, returns, T, N, A, use_norm, norm_mean, norm_var))) return 1;
    MMS_FREE(mms::launch_gae_marl_agents(rewards, value_preds, masks, returns, T, N, A, gamma, lam, use_norm, norm_mean, norm_var, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_ppo_act(int device, const float* mean, const float* value, const float* log_std, uint64_t seed,
                                                       int64_t* counters, int64_t row_offset, int32_t reference_scale, float* actions_out,
                                                       float* act_slot, float* logp_slot, float* value_slot, float* mu_slot, float* sigma_slot,
                                                       int64_t N, int32_t A, void* s) {
    MMS_DEV(device)
    if (refused(check_ppo_act(mean, log_std, counters, N, A))) return 1;
    MMS_FREE(mms::launch_ppo_act(mean, value, log_std, seed, counters, row_offset, reference_scale, actions_out, act_slot, logp_slot, value_slot,
                                 mu_slot, sigma_slot, N, A, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_ppo_heads_act(int device, const float* hidden, const float* weight, const float* bias, int32_t H,
                                                             const float* value, const float* vhidden, const float* vweight, const float* vbias,
                                                             int32_t VH, const float* log_std, uint64_t seed, int64_t* counters,
                                                             int64_t row_offset, int32_t reference_scale, float* actions_out, float* act_slot,
                                                             float* logp_slot, float* value_slot, float* mu_slot, float* sigma_slot, int64_t N,
                                                             int32_t A, void* s) {
    MMS_DEV(device)
    if (refused(check_ppo_heads_act(hidden, weight, bias, H, vhidden, vweight, vbias, VH, log_std, counters, N, A))) return 1;
    MMS_FREE(mms::launch_ppo_head_act(hidden, weight, bias, H, value, vhidden, vweight, vbias, VH, log_std, seed, counters, row_offset, reference_scale,
                                      actions_out, act_slot, logp_slot, value_slot, mu_slot, sigma_slot, N, A, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_sac_heads_act(int device, const float* hidden, int32_t H, const float* mu_weight,
                                                             const float* mu_bias, const float* ls_weight, const float* ls_bias, float act_limit,
                                                             float epsilon, int32_t deterministic, uint64_t seed, int64_t* counters,
                                                             int64_t row_offset, float* actions_out, float* act_slot, float* logp_slot,
                                                             float* u_slot, float* mu_slot, float* log_std_slot, int64_t N, int32_t A, void* s) {
    MMS_DEV(device)
    if (refused(check_sac_heads_act(hidden, H, mu_weight, mu_bias, ls_weight, ls_bias, deterministic, counters, N, A))) return 1;
    MMS_FREE(mms::launch_sac_head_act(hidden, H, mu_weight, mu_bias, ls_weight, ls_bias, act_limit, epsilon, deterministic, seed, counters, row_offset,
                                      actions_out, act_slot, logp_slot, u_slot, mu_slot, log_std_slot, N, A, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_sac_heads_grad(int device, int64_t N, int32_t A, float act_limit, float epsilon, const float* u,
                                                              const float* mu, const float* log_std, const float* grad_action,
                                                              const float* grad_logp, float* dy, float* dbias, void* workspace, int64_t* ws_bytes,
                                                              void* s) {
    MMS_DEV(device)
    const bool shapes = N >= 0 && N <= 0x7fffffff && A >= 1 && A <= 128;
    const int64_t need = shapes ? mms::sac_grad_ws_bytes(N, A) : 0;
    if (refused(check_sac_heads_grad(N, A, u, mu, log_std, grad_action, grad_logp, dy, workspace, ws_bytes, need))) return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    if (N == 0) return 0;
    MMS_FREE(mms::launch_sac_heads_grad(N, A, act_limit, epsilon, u, mu, log_std, grad_action, grad_logp, dy, dbias, workspace, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_q_heads_backup(int device, int64_t M, int32_t H, const float* h0, const float* w0, const float* b0,
                                                              float* q0_out, const float* h1, const float* w1, const float* b1, float* q1_out,
                                                              const float* reward, const uint8_t* done, const float* logp, float gamma,
                                                              float alpha, float* backup, void* s) {
    MMS_DEV(device)
    if (refused(check_q_heads_backup(M, H, h0, w0, b0, q0_out, h1, w1, b1, q1_out, reward, done, backup))) return 1;
    const float* h[2] = {h0, h1};
    const float* w[2] = {w0, w1};
    const float* b[2] = {b0, b1};
    float* q[2] = {q0_out, q1_out};
    MMS_FREE(mms::launch_q_heads_backup(h1 ? 2 : 1, M, H, h, w, b, q, reward, done, backup ? logp : nullptr, gamma, alpha, backup, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_q_heads_loss(int device, int64_t M, int32_t H, const float* h0, const float* w0, const float* b0,
                                                            const float* h1, const float* w1, const float* b1, int32_t mode, const float* target,
                                                            const float* logp, float alpha, float scale, float* loss, float* q0_out,
                                                            float* q1_out, float* dh0, float* dh1, float* dw0, float* db0, float* dw1, float* db1,
                                                            void* workspace, int64_t* ws_bytes, void* s) {
    MMS_DEV(device)
    const int G = h1 ? 2 : 1;
    const bool shapes = M >= 1 && M <= 0x7fffffff && H > 0 && H % 64 == 0 && H <= MMS_Q_LOSS_MAX_H;
    const int64_t need = shapes ? mms::q_loss_ws_bytes(M, H, G) : 0;
    if (refused(check_q_heads_loss(M, H, h0, w0, b0, h1, w1, b1, mode, target, loss, q1_out, dh0, dh1, dw0, db0, dw1, db1, workspace, ws_bytes, need)))
        return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    const float* h[2] = {h0, h1};
    const float* w[2] = {w0, w1};
    const float* b[2] = {b0, b1};
    float* q[2] = {q0_out, q1_out};
    float* dh[2] = {dh0, dh1};
    float* dw[2] = {dw0, dw1};
    float* db[2] = {db0, db1};
    MMS_FREE(mms::launch_q_heads_loss(G, M, H, h, w, b, mode, target, logp, alpha, scale, loss, q, dh, dw, db, workspace, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_det_heads_act_group(int device, int32_t groups, int64_t M, int32_t H, int32_t A, int32_t agent0,
                                                                   const float* const* h, const float* const* w, const float* const* b,
                                                                   const float* act_limit, float sigma, uint64_t seed, int64_t* counters,
                                                                   int64_t row_offset, float* const* act_out, int64_t act_pitch, float* joint_out,
                                                                   int64_t joint_pitch, void* s) {
    MMS_DEV(device)
    if (refused(check_det_heads_act_group(groups, M, H, A, agent0, h, w, b, act_limit, sigma, counters, act_out, act_pitch, joint_out, joint_pitch))) return 1;
    mms::DetHeadsArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.h[g] = h[g]; a.w[g] = w[g]; a.b[g] = b[g]; a.act_out[g] = act_out ? act_out[g] : nullptr; a.act_limit[g] = act_limit[g];
    }
    a.joint_out = joint_out; a.counters = counters; a.seed = seed; a.M = M; a.row_offset = row_offset; a.act_pitch = act_pitch;
    a.joint_pitch = joint_pitch; a.H = H; a.A = A; a.agent0 = agent0; a.sigma = sigma; a.noise_clip = -1.f;
    MMS_FREE(mms::launch_det_heads_act(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_det_heads_act(int device, int64_t M, int32_t H, int32_t A, const float* h, const float* w,
                                                             const float* b, float act_limit, float sigma, float noise_clip, uint64_t seed,
                                                             int64_t* counters, int64_t row_offset, float* act_out, int64_t act_pitch,
                                                             float* tanh_out, void* s) {
    MMS_DEV(device)
    if (refused(check_det_heads_act(M, H, A, h, w, b, act_limit, sigma, noise_clip, counters, act_out, act_pitch, tanh_out))) return 1;
    mms::DetHeadsArgs a = {};              // the grouped kernel with one group: the same block body, the same bits
    a.h[0] = h; a.w[0] = w; a.b[0] = b; a.act_out[0] = act_out; a.act_limit[0] = act_limit;
    a.counters = counters; a.seed = seed; a.M = M; a.row_offset = row_offset; a.act_pitch = act_pitch; a.H = H; a.A = A; a.sigma = sigma;
    a.tanh_out = tanh_out; a.noise_clip = det_noise_clip(noise_clip);
    MMS_FREE(mms::launch_det_heads_act(a, 1, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_det_heads_grad(int device, int64_t N, int32_t A, float act_limit, const float* t, const float* g,
                                                              int64_t grad_pitch, float* dy, float* dbias, void* workspace, int64_t* ws_bytes,
                                                              void* s) {
    MMS_DEV(device)
    const bool shapes = N >= 0 && N <= 0x7fffffff && A >= 1 && A <= 128;
    const int64_t need = shapes ? mms::det_grad_ws_bytes(N, A) : 0;
    if (refused(check_det_heads_grad(N, A, t, g, grad_pitch, dy, workspace, ws_bytes, need))) return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    if (N == 0) return 0;
    MMS_FREE(mms::launch_det_heads_grad(N, A, act_limit, t, g, grad_pitch, dy, dbias, workspace, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_q_heads_backup_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* h,
                                                                    const float* const* w, const float* const* b, float* const* q_out,
                                                                    const float* const* reward, const uint8_t* const* done, float gamma,
                                                                    float* const* backup, void* s) {
    MMS_DEV(device)
    if (refused(check_q_heads_backup_group(groups, M, H, h, w, b, q_out, reward, done, backup))) return 1;
    mms::QGroupArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.h[g] = h[g]; a.w[g] = w[g]; a.b[g] = b[g];
        a.q_out[g] = q_out ? q_out[g] : nullptr;
        a.backup[g] = backup ? backup[g] : nullptr;
        a.reward[g] = a.backup[g] ? reward[g] : nullptr;
        a.done[g] = a.backup[g] ? done[g] : nullptr;
    }
    a.gamma = gamma; a.M = M; a.H = H;
    MMS_FREE(mms::launch_q_heads_backup_group(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int64_t mms_param_step_partials(int32_t tensors, const int64_t* numel) { return param_step_partials(tensors, numel); }

__attribute__((visibility("default"))) int mms_param_step(int device, int32_t tensors, const int64_t* numel, float* const* param, const float* const* grad,
                                                          float* const* exp_avg, float* const* exp_avg_sq, float* const* target, double lr, double beta1,
                                                          double beta2, double eps, double weight_decay, int64_t step, double max_norm, double polyak,
                                                          int32_t flags, double* partials, float* norm_out, void* s) {
    MMS_DEV(device)
    if (refused(check_param_step(tensors, numel, param, grad, exp_avg, exp_avg_sq, target, lr, beta1, beta2, eps, weight_decay, step, max_norm, polyak, flags,
                                 partials, norm_out)))
        return 1;
    if (tensors == 0) return 0;
    const mms::ParamArgs a = build_param_args(tensors, numel, param, grad, exp_avg, exp_avg_sq, target, lr, beta1, beta2, eps, weight_decay, step, max_norm,
                                              polyak, partials, norm_out);
    MMS_FREE(mms::launch_param_step(a, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_linear2_act(int device, int64_t M, int32_t N, int32_t K, const float* x0, const float* w0, const float* b0,
                                                           float* y0, const float* x1, const float* w1, const float* b1, float* y1, int32_t act,
                                                           void* s) {
    MMS_DEV(device)
    if (refused(check_linear2_act(M, N, K, x0, w0, b0, y0, x1, w1, b1, y1, act))) return 1;
    const bool two = x1 != nullptr;
    mms::LinearArgs a = {};
    a.x[0] = x0; a.x[1] = x1; a.w[0] = w0; a.w[1] = w1; a.b[0] = b0; a.b[1] = b1; a.y[0] = y0; a.y[1] = y1;
    a.M = (int)M; a.N = N; a.K = K; a.act = act;
    MMS_FREE(mms::launch_linear_act(a, two ? 2 : 1, (hipStream_t)s));
    return 0;
}

// ---- split-operand layers (split_kernels.hip) ---------------------------------------------------------------------------------
__attribute__((visibility("default"))) int mms_split_planes(int device, int64_t rows, int32_t K, int32_t x_pitch, const float* x, void* planes, void* s) {
    MMS_DEV(device)
    if (x_pitch == 0) x_pitch = K;
    if (refused(check_split_planes(rows, K, x_pitch, x, planes))) return 1;
    MMS_FREE(mms::launch_split_planes(x, planes, rows, K, x_pitch, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_split_planes_group(int device, int32_t groups, int64_t rows, int32_t K, int32_t x_pitch,
                                                                  const float* const* x, void* const* planes, void* s) {
    MMS_DEV(device)
    if (x_pitch == 0) x_pitch = K;
    if (refused(check_split_planes_group(groups, rows, K, x_pitch, x, planes))) return 1;
    mms::SplitPlanesArgs a = {};
    for (int g = 0; g < groups; g++) { a.x[g] = x[g]; a.planes[g] = planes[g]; }
    a.rows = rows; a.K = K; a.x_pitch = x_pitch;
    MMS_FREE(mms::launch_split_planes_group(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_linear_group_act_split(int device, int32_t groups, int64_t M, int32_t N, int32_t K, const void* const* x,
                                                                      const void* const* w, const float* const* b, void* const* y, int32_t act,
                                                                      int32_t out_mode, const float* const* ln_s, const float* const* ln_stat_in,
                                                                      float* const* ln_part_out, const float* const* head_w, float* const* head_part,
                                                                      const int32_t* head_dims, void* s) {
    MMS_DEV(device)
    if (refused(check_split_layer(false, groups, M, N, K, x, w, b, y, nullptr, nullptr, nullptr, act, out_mode, ln_s, ln_stat_in, ln_part_out, head_w, head_part, head_dims))) return 1;
    const bool ln = ln_s != nullptr;
    mms::SplitLinearArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.x[g] = x[g]; a.w[g] = w[g]; a.b[g] = b[g]; a.y[g] = out_mode != 2 ? y[g] : nullptr;
        if (ln) { a.s[g] = ln_s[g]; a.stat_in[g] = ln_stat_in[g]; a.part_out[g] = ln_part_out[g]; }
        if (out_mode == 2) { a.head_w[g] = head_w[g]; a.head_part[g] = head_part[g]; a.hdims[g] = head_dims[g]; }
    }
    a.M = (int)M; a.N = N; a.KC = (K + 31) / 32; a.act = act; a.out_mode = out_mode;
    MMS_FREE(mms::launch_linear_split(a, groups, (hipStream_t)s));
    return 0;
}

// ---- the same with two scaled fp16 planes per operand (split16_kernels.hip) -----------------------------------------------------
__attribute__((visibility("default"))) int mms_split_planes16_group(int device, int32_t groups, int64_t rows, int32_t K, int32_t x_pitch,
                                                                    const float* const* x, void* const* planes, float* const* scale, float* const* inv,
                                                                    int32_t nchains, int32_t L, const float* const* chain, float* const* chain_scale,
                                                                    float* const* chain_inv, float* const* stat, float eps, void* s) {
    MMS_DEV(device)
    if (x_pitch == 0) x_pitch = K;
    if (refused(check_split_planes16_group(groups, rows, K, x_pitch, x, planes, scale, inv, nchains, L, chain, chain_scale, chain_inv, stat))) return 1;
    mms::Split16PlanesArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.x[g] = x[g]; a.planes[g] = planes[g]; a.scale[g] = scale[g]; a.inv[g] = inv[g];
        if (nchains > 0) { a.chain[g] = chain[g]; a.chain_scale[g] = chain_scale[g]; a.chain_inv[g] = chain_inv[g]; }
        if (stat) a.stat[g] = stat[g];
    }
    a.rows = rows; a.K = K; a.x_pitch = x_pitch; a.nchains = nchains; a.L = nchains > 0 ? L : 0; a.eps = eps;
    MMS_FREE(mms::launch_split16_planes_group(a, groups, (hipStream_t)s));
    return 0;
}

// ... of one matrix whose rows are [x0 row | x1 row], read where the two halves lie (a critic's cat(obs, act))
__attribute__((visibility("default"))) int mms_split_planes16_cat(int device, int64_t rows, int32_t K0, int32_t pitch0, const float* x0, int32_t K1,
                                                                  int32_t pitch1, const float* x1, void* planes, float* scale, float* inv,
                                                                  int32_t nchains, int32_t L, const float* chain, float* chain_scale, float* chain_inv,
                                                                  void* s) {
    MMS_DEV(device)
    if (pitch0 == 0) pitch0 = K0;
    if (pitch1 == 0) pitch1 = K1;
    if (refused(check_split_planes16_cat(rows, K0, pitch0, x0, K1, pitch1, x1, planes, nchains, L, chain, chain_scale, chain_inv))) return 1;
    mms::Split16CatArgs a = {};
    a.x0 = x0; a.x1 = x1; a.planes = planes; a.scale = scale; a.inv = inv;
    if (nchains > 0) { a.chain = chain; a.chain_scale = chain_scale; a.chain_inv = chain_inv; }
    a.rows = rows; a.K0 = K0; a.pitch0 = pitch0; a.K1 = K1; a.pitch1 = pitch1; a.nchains = nchains; a.L = nchains > 0 ? L : 0;
    MMS_FREE(mms::launch_split16_planes_cat(a, (hipStream_t)s));
    return 0;
}

// The weights' side of the split16 layers, refreshed on the device after every parameter update: planes, row scales and row 1-norms of
// `groups` weight matrices of ANY shapes in one launch ...
__attribute__((visibility("default"))) int mms_weight_planes16_group(int device, int32_t groups, const int64_t* N, const int32_t* K, const float* const* w,
                                                                     void* const* planes, float* const* scale, float* const* inv,
                                                                     float* const* l1, void* s) {
    MMS_DEV(device)
    if (refused(check_weight_planes16_group(groups, N, K, w, planes, scale, inv))) return 1;
    mms::Split16PlanesArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.x[g] = w[g]; a.planes[g] = planes[g]; a.scale[g] = scale[g]; a.inv[g] = inv[g];
        a.l1[g] = l1 ? l1[g] : nullptr;
        a.rows_g[g] = N[g]; a.K_g[g] = K[g];
    }
    a.per_group = 1;
    MMS_FREE(mms::launch_split16_planes_group(a, groups, (hipStream_t)s));
    return 0;
}

// ... and the bound chain (+ the scales of a constant-bound input) from them, one launch.
__attribute__((visibility("default"))) int mms_chain_refresh16(int device, int32_t nchains, int32_t L, const float* const* l1, const float* const* bias,
                                                               const int32_t* n, float* chain, float bound0, int64_t rows, float* chain_scale,
                                                               float* chain_inv, void* s) {
    MMS_DEV(device)
    if (refused(check_chain_refresh16(nchains, L, l1, n, chain, bound0, rows, chain_scale, chain_inv))) return 1;
    mms::ChainRefreshArgs a = {};
    for (int e = 0; e < nchains * L; e++) { a.l1[e] = l1[e]; a.bias[e] = bias ? bias[e] : nullptr; a.n[e] = n[e]; }
    a.chain = chain; a.nchains = nchains; a.L = L; a.bound0 = bound0; a.rows = rows; a.chain_scale = chain_scale; a.chain_inv = chain_inv;
    MMS_FREE(mms::launch_chain_refresh16(a, (hipStream_t)s));
    return 0;
}

// ---- the folded-LayerNorm layers' weight side, refreshed on the device (fold16_kernels.hip) ------------------------------------
__attribute__((visibility("default"))) int mms_fold_planes16_group(int device, int32_t groups, const int64_t* N, const int32_t* K, const float* const* w,
                                                                   const float* const* gamma, const float* const* beta, const float* const* bias,
                                                                   void* const* planes, float* const* inv, float* const* s_out, float* const* c_out,
                                                                   float* const* rb, float* const* wt, void* s) {
    MMS_DEV(device)
    if (refused(check_fold_planes16_group(groups, N, K, w, planes, inv))) return 1;
    mms::FoldPlanesArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.w[g] = w[g];
        a.gamma[g] = gamma ? gamma[g] : nullptr; a.beta[g] = beta ? beta[g] : nullptr; a.bias[g] = bias ? bias[g] : nullptr;
        a.planes[g] = planes ? planes[g] : nullptr; a.inv[g] = inv ? inv[g] : nullptr;
        a.s[g] = s_out ? s_out[g] : nullptr; a.c[g] = c_out ? c_out[g] : nullptr; a.rb[g] = rb ? rb[g] : nullptr; a.wt[g] = wt ? wt[g] : nullptr;
        a.rows_g[g] = N[g]; a.K_g[g] = K[g];
    }
    MMS_FREE(mms::launch_fold_planes16(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_fold_scales16_group(int device, int32_t groups, const float* const* rb, const int32_t* n, int64_t M,
                                                                   float* const* scale1, float* const* ysc, float* const* yinv, void* s) {
    MMS_DEV(device)
    if (refused(check_fold_scales16_group(groups, rb, n, M))) return 1;
    mms::FoldScalesArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.rb[g] = rb[g]; a.n[g] = n[g];
        a.scale1[g] = scale1 ? scale1[g] : nullptr; a.ysc[g] = ysc ? ysc[g] : nullptr; a.yinv[g] = yinv ? yinv[g] : nullptr;
    }
    a.M = M;
    MMS_FREE(mms::launch_fold_scales16(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_linear_group_act_split16(int device, int32_t groups, int64_t M, int32_t N, int32_t K, const void* const* x,
                                                                        const void* const* w, const float* const* b, void* const* y,
                                                                        const float* const* x_inv, const float* const* w_inv, const float* const* y_scale,
                                                                        int32_t act, int32_t out_mode, const float* const* ln_s,
                                                                        const float* const* ln_stat_in, float* const* ln_part_out,
                                                                        const float* const* head_w, float* const* head_part, const int32_t* head_dims, void* s) {
    MMS_DEV(device)
    if (refused(check_split_layer(true, groups, M, N, K, x, w, b, y, x_inv, w_inv, y_scale, act, out_mode, ln_s, ln_stat_in, ln_part_out, head_w, head_part, head_dims))) return 1;
    const bool ln = ln_s != nullptr;
    mms::Split16LinearArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.x[g] = x[g]; a.w[g] = w[g]; a.b[g] = b[g]; a.y[g] = out_mode != 2 ? y[g] : nullptr;
        a.xinv[g] = x_inv[g]; a.winv[g] = w_inv[g]; a.yscale[g] = out_mode == 1 ? y_scale[g] : nullptr;
        if (ln) { a.s[g] = ln_s[g]; a.stat_in[g] = ln_stat_in[g]; a.part_out[g] = ln_part_out[g]; }
        if (out_mode == 2) { a.head_w[g] = head_w[g]; a.head_part[g] = head_part[g]; a.hdims[g] = head_dims[g]; }
    }
    a.M = (int)M; a.N = N; a.KC = (K + 31) / 32; a.act = act; a.out_mode = out_mode;
    MMS_FREE(mms::launch_linear_split16(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_layer_clock_probe(int device, uint64_t* out, int32_t slots) {
    (void)device;
    if (refused(check_layer_clock_probe(out, slots))) return 1;
    mms::set_split16_clock_probe(out, out ? slots : 0);
    return 0;
}

__attribute__((visibility("default"))) int mms_row_stats_chan_group(int device, int32_t groups, int64_t M, int32_t slots, const float* const* part,
                                                                    float* const* stat, float eps, void* s) {
    MMS_DEV(device)
    if (refused(check_row_stats_chan_group(groups, M, slots, part, stat))) return 1;
    mms::RowStatsArgs a = {};
    for (int g = 0; g < groups; g++) { a.part[g] = part[g]; a.stat[g] = stat[g]; }
    a.M = M; a.slots = slots; a.width = 64 * slots; a.eps = eps;
    MMS_FREE(mms::launch_row_stats_chan(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_marl_heads_finish(int device, int32_t groups, int64_t M, int32_t slots, const float* const* part,
                                                                 const float* const* head_part, const float* const* hs, const float* const* hc,
                                                                 const int32_t* A, const float* const* std, float* const* out, float* const* logp,
                                                                 const int32_t* out_pitch, int64_t* const* counters, uint64_t seed, int64_t row_offset,
                                                                 float eps, void* s) {
    MMS_DEV(device)
    if (refused(check_marl_heads_finish(groups, M, slots, part, head_part, hs, hc, A, out, out_pitch))) return 1;
    mms::HeadsFinishArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.part[g] = part[g]; a.head_part[g] = head_part[g]; a.hs[g] = hs[g]; a.hc[g] = hc[g]; a.out[g] = out[g];
        a.std[g] = std ? std[g] : nullptr;
        a.logp[g] = logp ? logp[g] : nullptr;
        a.counters[g] = counters ? counters[g] : nullptr;
        a.A[g] = A[g];
        a.out_pitch[g] = out_pitch ? out_pitch[g] : A[g];
    }
    a.seed = seed; a.M = M; a.row_offset = row_offset; a.slots = slots; a.width = 64 * slots; a.eps = eps;
    MMS_FREE(mms::launch_marl_heads_finish(a, groups, (hipStream_t)s));
    return 0;
}

// ---- grouped policy inference (MAPPO / HAPPO: all agents' networks per launch) -----------------------------------------------
__attribute__((visibility("default"))) int mms_linear_group_act(int device, int32_t groups, int64_t M, int32_t N, int32_t K, const float* const* x,
                                                                const float* const* w, const float* const* b, float* const* y, int32_t act,
                                                                const float* const* ln_s, const float* const* ln_stat_in, float* const* ln_part_out,
                                                                void* s) {
    MMS_DEV(device)
    if (refused(check_linear_group_act(groups, M, N, K, x, w, b, y, act, ln_s, ln_stat_in, ln_part_out))) return 1;
    mms::LinearArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.x[g] = x[g]; a.w[g] = w[g]; a.b[g] = b[g]; a.y[g] = y[g];
        if (ln_s) { a.s[g] = ln_s[g]; a.stat_in[g] = ln_stat_in[g]; }
        if (ln_part_out) a.part_out[g] = ln_part_out[g];
    }
    a.M = (int)M; a.N = N; a.K = K; a.act = act & 15; a.blocked = (act & 16) != 0;
    MMS_FREE(mms::launch_linear_act(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_row_stats_group(int device, int32_t groups, int64_t M, int32_t slots, int32_t width, const float* const* part,
                                                               float* const* stat, float eps, void* s) {
    MMS_DEV(device)
    if (refused(check_row_stats_group(groups, M, slots, width, part, stat))) return 1;
    mms::RowStatsArgs a = {};
    for (int g = 0; g < groups; g++) { a.part[g] = part[g]; a.stat[g] = stat[g]; }
    a.M = M; a.slots = slots; a.width = width; a.eps = eps;
    MMS_FREE(mms::launch_row_stats(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_row_moments_group(int device, int32_t groups, int64_t M, int32_t K, int32_t x_pitch, const float* const* x,
                                                                 float* const* stat, float eps, void* s) {
    MMS_DEV(device)
    if (x_pitch == 0) x_pitch = K;
    if (refused(check_row_moments_group(groups, M, K, x_pitch, x, stat))) return 1;
    mms::LayerNormArgs a = {};
    for (int g = 0; g < groups; g++) { a.x[g] = x[g]; a.y[g] = stat[g]; }
    a.M = M; a.K = K; a.Kp = K; a.x_pitch = x_pitch; a.eps = eps; a.stats_only = 1;
    MMS_FREE(mms::launch_layernorm(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_layernorm_group(int device, int32_t groups, int64_t M, int32_t K, int32_t Kp, int32_t x_pitch,
                                                               const float* const* x, const float* const* gamma, const float* const* beta, float* const* y,
                                                               float eps, void* s) {
    MMS_DEV(device)
    if (x_pitch == 0) x_pitch = K;
    if (refused(check_layernorm_group(groups, M, K, Kp, x_pitch, x, gamma, beta, y))) return 1;
    mms::LayerNormArgs a = {};
    for (int g = 0; g < groups; g++) { a.x[g] = x[g]; a.gamma[g] = gamma[g]; a.beta[g] = beta[g]; a.y[g] = y[g]; }
    a.M = M; a.K = K; a.Kp = Kp; a.x_pitch = x_pitch; a.eps = eps;
    MMS_FREE(mms::launch_layernorm(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_marl_heads_act(int device, int32_t groups, int64_t M, int32_t H, const float* const* h,
                                                              const float* const* gamma, const float* const* beta, const float* const* w,
                                                              const float* const* b, const int32_t* A, const float* const* std, float* const* out,
                                                              float* const* logp, const int32_t* out_pitch, int64_t* const* counters, uint64_t seed,
                                                              int64_t row_offset, float eps, void* s) {
    MMS_DEV(device)
    if (refused(check_marl_heads_act(groups, M, H, h, gamma, beta, w, b, A, out, out_pitch, eps))) return 1;
    mms::HeadsArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.h[g] = h[g]; a.gamma[g] = eps >= 0.f ? gamma[g] : nullptr; a.beta[g] = eps >= 0.f ? beta[g] : nullptr; a.w[g] = w[g]; a.b[g] = b[g]; a.A[g] = A[g]; a.out[g] = out[g];
        a.out_pitch[g] = out_pitch ? out_pitch[g] : A[g];
        a.std[g] = std ? std[g] : nullptr;
        a.logp[g] = logp ? logp[g] : nullptr;
        a.counters[g] = counters ? counters[g] : nullptr;
    }
    a.seed = seed; a.M = M; a.row_offset = row_offset; a.H = H; a.eps = eps;
    MMS_FREE(mms::launch_marl_heads(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_marl_heads_eval(int device, int32_t groups, int64_t M, int32_t H, const float* const* h,
                                                               const float* const* gamma, const float* const* beta, const float* const* w,
                                                               const float* const* b, const int32_t* A, const float* const* std,
                                                               const float* const* act, const int32_t* act_pitch, float* const* logp,
                                                               const int32_t* logp_pitch, const float* const* old_logp, const int32_t* old_pitch,
                                                               const float* const* factor_in, float* const* factor_out, float eps, void* s) {
    MMS_DEV(device)
    if (refused(check_marl_heads_eval(groups, M, H, h, gamma, beta, w, b, A, std, act, act_pitch, logp, logp_pitch, old_logp, old_pitch, factor_in,
                                      factor_out, eps)))
        return 1;
    mms::HeadsEvalArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.h[g] = h[g]; a.gamma[g] = eps >= 0.f ? gamma[g] : nullptr; a.beta[g] = eps >= 0.f ? beta[g] : nullptr; a.w[g] = w[g]; a.b[g] = b[g];
        a.A[g] = A[g]; a.std[g] = std[g]; a.act[g] = act[g];
        a.logp[g] = logp ? logp[g] : nullptr;
        a.factor_out[g] = factor_out ? factor_out[g] : nullptr;
        a.old_logp[g] = (a.factor_out[g] && old_logp) ? old_logp[g] : nullptr;
        a.factor_in[g] = (a.factor_out[g] && factor_in) ? factor_in[g] : nullptr;
        a.act_pitch[g] = act_pitch ? act_pitch[g] : A[g];
        a.logp_pitch[g] = logp_pitch ? logp_pitch[g] : A[g];
        a.old_pitch[g] = old_pitch ? old_pitch[g] : A[g];
    }
    a.M = M; a.H = H; a.eps = eps;
    MMS_FREE(mms::launch_marl_heads_eval(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_gru_group(int device, int32_t groups, int64_t M, int32_t K, int32_t H, const float* const* x, int64_t x_pitch,
                                                         const float* const* h, int64_t h_pitch, const float* const* mask, int64_t mask_pitch,
                                                         const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                                                         const float* const* b_hh, float* const* h_out, int64_t h_out_pitch, float* const* y, void* s) {
    MMS_DEV(device)
    if (refused(check_gru_group(groups, M, K, H, x, x_pitch, h, h_pitch, mask, mask_pitch, w_ih, w_hh, b_ih, b_hh, h_out, h_out_pitch, y))) return 1;
    mms::GruArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.x[g] = x[g]; a.h[g] = h[g]; a.mask[g] = mask ? mask[g] : nullptr;
        a.w_ih[g] = w_ih[g]; a.w_hh[g] = w_hh[g]; a.b_ih[g] = b_ih[g]; a.b_hh[g] = b_hh[g];
        a.h_out[g] = h_out[g]; a.y[g] = y ? y[g] : nullptr;
    }
    a.x_pitch = x_pitch; a.h_pitch = h_pitch; a.mask_pitch = mask_pitch; a.h_out_pitch = h_out_pitch;
    a.M = (int)M; a.K = K; a.H = H;
    MMS_FREE(mms::launch_gru_group(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_gru_gates_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* gi, const float* const* gh,
                                                               int64_t g_pitch, const float* const* h, int64_t h_pitch, const float* const* mask,
                                                               int64_t mask_pitch, const float* const* b_hh, float* const* h_out, int64_t h_out_pitch,
                                                               float* const* y, void* s) {
    MMS_DEV(device)
    if (refused(check_gru_gates_group(groups, M, H, gi, gh, g_pitch, h, h_pitch, mask, mask_pitch, b_hh, h_out, h_out_pitch, y))) return 1;
    mms::GruGatesArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.gi[g] = gi[g]; a.gh[g] = gh[g]; a.h[g] = h[g]; a.mask[g] = mask ? mask[g] : nullptr;
        a.b_hh[g] = b_hh[g]; a.h_out[g] = h_out[g]; a.y[g] = y ? y[g] : nullptr;
    }
    a.g_pitch = g_pitch; a.h_pitch = h_pitch; a.mask_pitch = mask_pitch; a.h_out_pitch = h_out_pitch;
    a.M = (int)M; a.H = H;
    MMS_FREE(mms::launch_gru_gates_group(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_gru_gates_grad_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* gi,
                                                                    const float* const* gh, int64_t g_pitch, const float* const* h, int64_t h_pitch,
                                                                    const float* const* mask, int64_t mask_pitch, const float* const* b_hh,
                                                                    const float* const* dh_out, int64_t dh_out_pitch, const float* const* dy,
                                                                    int64_t dy_pitch, float* const* dgi, float* const* dgh, int64_t dg_pitch,
                                                                    float* const* dh, int64_t dh_pitch, float* const* dbias, void* workspace,
                                                                    int64_t* ws_bytes, void* s) {
    MMS_DEV(device)
    const bool shapes = groups >= 1 && groups <= MMS_MAX_GROUPS && M >= 0 && M <= 0x7fffffff && H >= 4 && H <= 1024 && (H % 4) == 0;
    const int64_t need = shapes ? mms::gru_grad_ws_bytes(groups, M, H) : 0;
    if (refused(check_gru_gates_grad_group(groups, M, H, gi, gh, g_pitch, h, h_pitch, mask, mask_pitch, b_hh, dh_out, dh_out_pitch, dy, dy_pitch, dgi, dgh,
                                           dg_pitch, dh, dh_pitch, dbias, workspace, ws_bytes, need)))
        return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    mms::GruGradArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.gi[g] = gi[g]; a.gh[g] = gh[g]; a.h[g] = h[g]; a.mask[g] = mask ? mask[g] : nullptr; a.b_hh[g] = b_hh[g];
        a.dh_out[g] = dh_out[g]; a.dy[g] = dy ? dy[g] : nullptr;
        a.dgi[g] = dgi[g]; a.dgh[g] = dgh[g]; a.dh[g] = dh[g]; a.dbias[g] = dbias ? dbias[g] : nullptr;
    }
    a.part = static_cast<double*>(workspace);
    a.g_pitch = g_pitch; a.h_pitch = h_pitch; a.mask_pitch = mask_pitch; a.dh_out_pitch = dh_out_pitch; a.dy_pitch = dy_pitch;
    a.dg_pitch = dg_pitch; a.dh_pitch = dh_pitch;
    a.M = (int)M; a.H = H;
    MMS_FREE(mms::launch_gru_gates_grad_group(a, groups, (hipStream_t)s));
    return 0;
}

// ---- the ELU + LayerNorm blocks of the MARL networks, forward and backward (elu_ln_kernels.hip) ------------------------------------

__attribute__((visibility("default"))) int mms_elu_ln_group(int device, int32_t groups, int64_t M, int32_t H, float eps, const float* const* z, int64_t z_pitch,
                                                            const float* const* bias, const float* const* gamma, const float* const* beta, float* const* y,
                                                            int64_t y_pitch, float* const* stat, void* s) {
    MMS_DEV(device)
    if (refused(check_elu_ln_group(groups, M, H, eps, z, z_pitch, bias, gamma, beta, y, y_pitch, stat))) return 1;
    mms::EluLnArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.z[g] = z[g]; a.bias[g] = bias[g]; a.gamma[g] = gamma[g]; a.beta[g] = beta[g]; a.y[g] = y[g]; a.stat[g] = stat[g];
    }
    a.z_pitch = z_pitch; a.y_pitch = y_pitch; a.eps = eps; a.M = (int)M; a.H = H;
    MMS_FREE(mms::launch_elu_ln_group(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_elu_ln_planes16_group(int device, int32_t groups, int64_t M, int32_t H, float eps, const float* const* z,
                                                                     int64_t z_pitch, const float* const* bias, const float* const* gamma,
                                                                     const float* const* beta, float* const* y, int64_t y_pitch, float* const* stat,
                                                                     void* const* planes, float* const* scale, float* const* inv, void* s) {
    MMS_DEV(device)
    if (refused(check_elu_ln_planes16_group(groups, M, H, eps, z, z_pitch, bias, gamma, beta, y, y_pitch, stat, planes, scale, inv))) return 1;
    mms::EluLnPlanesArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.e.z[g] = z[g]; a.e.bias[g] = bias[g]; a.e.gamma[g] = gamma[g]; a.e.beta[g] = beta[g]; a.e.y[g] = y[g]; a.e.stat[g] = stat[g];
        a.planes[g] = planes[g]; a.scale[g] = scale[g]; a.inv[g] = inv[g];
    }
    a.e.z_pitch = z_pitch; a.e.y_pitch = y_pitch; a.e.eps = eps; a.e.M = (int)M; a.e.H = H;
    MMS_FREE(mms::launch_elu_ln_planes16_group(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_elu_ln_grad_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* z, int64_t z_pitch,
                                                                 const float* const* bias, const float* const* gamma, const float* const* stat,
                                                                 const float* const* dy, int64_t dy_pitch, float* const* dz, int64_t dz_pitch,
                                                                 float* const* dparams, void* workspace, int64_t* ws_bytes, void* s) {
    MMS_DEV(device)
    const int64_t need = elu_ln_shapes(groups, M, H) ? mms::elu_ln_grad_ws_bytes(groups, M, H) : 0;
    if (refused(check_elu_ln_grad_group(groups, M, H, z, z_pitch, bias, gamma, stat, dy, dy_pitch, dz, dz_pitch, dparams, workspace, ws_bytes, need))) return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    mms::EluLnGradArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.z[g] = z[g]; a.bias[g] = bias[g]; a.gamma[g] = gamma[g]; a.stat[g] = stat[g]; a.dy[g] = dy[g]; a.dz[g] = dz[g];
        a.dparams[g] = dparams ? dparams[g] : nullptr;
    }
    a.part = static_cast<double*>(workspace);
    a.z_pitch = z_pitch; a.dy_pitch = dy_pitch; a.dz_pitch = dz_pitch; a.M = (int)M; a.H = H;
    MMS_FREE(mms::launch_elu_ln_grad_group(a, groups, (hipStream_t)s));
    return 0;
}

// ---- the output heads of the MAPPO / HAPPO update, forward and backward (marl_heads_grad_kernels.hip) ------------------------------

__attribute__((visibility("default"))) int mms_marl_heads_fwd_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* f, int64_t f_pitch,
                                                                    const float* const* w, const float* const* b, const int32_t* A,
                                                                    const float* const* log_std, float x_coef, float y_coef, float* const* out,
                                                                    float* const* std_out, void* s) {
    MMS_DEV(device)
    if (refused(check_marl_heads_fwd_group(groups, M, H, f, f_pitch, w, b, A, log_std, x_coef, out, std_out))) return 1;
    mms::MarlHeadsFwdArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.f[g] = f[g]; a.w[g] = w[g]; a.b[g] = b[g]; a.out[g] = out[g]; a.A[g] = A[g];
        a.log_std[g] = log_std ? log_std[g] : nullptr;
        a.std[g] = a.log_std[g] ? std_out[g] : nullptr;
    }
    a.f_pitch = f_pitch; a.x_coef = x_coef; a.y_coef = y_coef; a.M = (int)M; a.H = H;
    MMS_FREE(mms::launch_marl_heads_fwd_group(a, groups, (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_marl_heads_grad_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* f, int64_t f_pitch,
                                                                     const float* const* w, const int32_t* A, const float* const* dout,
                                                                     const float* const* log_std, const float* const* dstd, float x_coef, float y_coef,
                                                                     float* const* df, int64_t df_pitch, float* const* dw, float* const* db,
                                                                     float* const* dlog_std, void* workspace, int64_t* ws_bytes, void* s) {
    MMS_DEV(device)
    const int64_t need = check_marl_heads_shapes("", groups, M, H, A).empty() ? mms::marl_heads_grad_ws_bytes(groups, M, H, A) : 0;
    if (refused(check_marl_heads_grad_group(groups, M, H, f, f_pitch, w, A, dout, log_std, dstd, x_coef, df, df_pitch, dw, db, dlog_std, workspace, ws_bytes,
                                            need)))
        return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    mms::MarlHeadsGradArgs a = {};
    for (int g = 0; g < groups; g++) {
        a.f[g] = f[g]; a.w[g] = w[g]; a.dout[g] = dout[g]; a.A[g] = A[g];
        a.df[g] = df ? df[g] : nullptr; a.dw[g] = dw ? dw[g] : nullptr; a.db[g] = db ? db[g] : nullptr;
        a.dlog_std[g] = dlog_std ? dlog_std[g] : nullptr;
        a.log_std[g] = a.dlog_std[g] ? log_std[g] : nullptr; a.dstd[g] = a.dlog_std[g] ? dstd[g] : nullptr;
    }
    a.part = static_cast<double*>(workspace);
    a.f_pitch = f_pitch; a.df_pitch = df_pitch; a.x_coef = x_coef; a.y_coef = y_coef; a.M = (int)M; a.H = H;
    MMS_FREE(mms::launch_marl_heads_grad_group(a, groups, (hipStream_t)s));
    return 0;
}

// ---- TRPO curvature products (trpo_kernels.hip) -----------------------------------------------------------------------------------

// The caller's workspace against the plan: answers the size query (2), refuses one that is too small or misaligned (1, error set), or 0 to go on
static int mlp_workspace(const char* who, int32_t layers, int64_t M, const int32_t* dims, bool rop, void* workspace, int64_t* ws_bytes, mms::MlpPlan* P) {
    if (!mms::mlp_plan(layers, M, dims, rop, P)) return fail(nullptr, std::string(who) + ": no plan for these shapes");
    if (!workspace) {
        *ws_bytes = (int64_t)P->total;
        return 2;
    }
    if (*ws_bytes < (int64_t)P->total)
        return fail(nullptr, std::string(who) + ": workspace too small (" + std::to_string(*ws_bytes) + " bytes, needs " + std::to_string(P->total) + ")");
    if (addr(workspace) & 255) return fail(nullptr, std::string(who) + ": workspace must be 256-byte aligned");
    return 0;
}

__attribute__((visibility("default"))) int mms_mlp_grad(int device, int32_t layers, int64_t M, const int32_t* dims, const float* x, const float* const* h,
                                                        const float* const* w, const float* g, float* const* dw, float* const* db,
                                                        float* const* d_out, float* const* e_out, void* workspace, int64_t* ws_bytes, void* s) {
    MMS_DEV(device)
    if (refused(check_mlp_grad(layers, M, dims, x, h, w, g, dw, db, d_out, e_out, workspace, ws_bytes))) return 1;
    mms::MlpPlan P;
    const int ws = mlp_workspace("mms_mlp_grad", layers, M, dims, false, workspace, ws_bytes, &P);
    if (ws != 0) return ws == 2 ? 0 : 1;
    MMS_FREE(mms::mlp_grad(P, x, h, w, g, dw, db, d_out, e_out, static_cast<uint8_t*>(workspace), (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_mlp_grad_rop(int device, int32_t layers, int64_t M, const int32_t* dims, const float* x,
                                                            const float* const* h, const float* const* w, const float* const* v,
                                                            const float* const* c, const float* g, const float* const* d, const float* const* e,
                                                            float* rmu, float* const* rdw, float* const* rdb, void* workspace, int64_t* ws_bytes,
                                                            void* s) {
    MMS_DEV(device)
    if (refused(check_mlp_grad_rop(layers, M, dims, x, h, w, v, c, g, d, e, rmu, rdw, rdb, workspace, ws_bytes))) return 1;
    mms::MlpPlan P;
    const int ws = mlp_workspace("mms_mlp_grad_rop", layers, M, dims, true, workspace, ws_bytes, &P);
    if (ws != 0) return ws == 2 ? 0 : 1;
    MMS_FREE(mms::mlp_grad_rop(P, x, h, w, v, c, g, d, e, rmu, rdw, rdb, static_cast<uint8_t*>(workspace), (hipStream_t)s));
    return 0;
}

// ---- HATRPO's Fisher-vector product: J^T g and J v of the LayerNorm-ELU actor (ln_mlp_kernels.hip) ------------------------------------

__attribute__((visibility("default"))) int mms_ln_mlp_grad(int device, int32_t blocks, int64_t M, const int32_t* dims, float eps, const float* x,
                                                           const float* const* h, const float* const* ln_g, const float* const* ln_t,
                                                           const float* const* w, const float* g, float* const* dln_g, float* const* dln_t,
                                                           float* const* dw, float* const* db, void* workspace, int64_t* ws_bytes, void* s) {
    MMS_DEV(device)
    mms::LnMlpPlan Q;
    int64_t need = 0;
    if (check_ln_mlp_shapes("mms_ln_mlp_grad", blocks, M, dims, ws_bytes).empty()) {
        if (!mms::ln_mlp_plan(blocks, M, dims, &Q)) return fail(nullptr, "mms_ln_mlp_grad: no plan for these shapes");
        need = (int64_t)Q.total;
    }
    if (refused(check_ln_mlp_grad(blocks, M, dims, eps, x, h, ln_g, ln_t, w, g, dln_g, dln_t, dw, db, workspace, ws_bytes, need))) return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    MMS_FREE(mms::ln_mlp_grad(Q, eps, x, h, ln_g, ln_t, w, g, dln_g, dln_t, dw, db, static_cast<uint8_t*>(workspace), (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_ln_mlp_jvp(int device, int32_t blocks, int64_t M, const int32_t* dims, float eps, const float* x,
                                                          const float* const* h, const float* const* ln_g, const float* const* ln_t,
                                                          const float* const* w, const float* const* vg, const float* const* vt,
                                                          const float* const* vw, const float* const* vc, const float* col_scale, float* rmu,
                                                          void* workspace, int64_t* ws_bytes, void* s) {
    MMS_DEV(device)
    mms::LnMlpPlan Q;
    int64_t need = 0;
    if (check_ln_mlp_shapes("mms_ln_mlp_jvp", blocks, M, dims, ws_bytes).empty()) {
        if (!mms::ln_mlp_plan(blocks, M, dims, &Q)) return fail(nullptr, "mms_ln_mlp_jvp: no plan for these shapes");
        need = (int64_t)Q.total;
    }
    if (refused(check_ln_mlp_jvp(blocks, M, dims, eps, x, h, ln_g, ln_t, w, vg, vt, vw, vc, rmu, workspace, ws_bytes, need))) return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    MMS_FREE(mms::ln_mlp_jvp(Q, eps, x, h, ln_g, ln_t, w, vg, vt, vw, vc, col_scale, rmu, static_cast<uint8_t*>(workspace), (hipStream_t)s));
    return 0;
}

// ---- the PPO update's loss head (ppo_loss_kernels.hip) ------------------------------------------------------------------------------

__attribute__((visibility("default"))) int mms_ppo_loss(int device, int64_t M, int32_t A, const float* mu, const float* log_std, const float* value,
                                                        const int64_t* indices, const float* actions, const float* old_logp, const float* adv,
                                                        const float* returns, const float* target_values, const float* old_mu,
                                                        const float* old_sigma, float clip, float value_coef, float entropy_coef,
                                                        int32_t clipped_value, float* out, float* dmu, float* dlog_std, float* dvalue,
                                                        void* workspace, int64_t* ws_bytes, void* s) {
    MMS_DEV(device)
    const bool shapes = M >= 1 && M <= 0x7fffffff && A >= 1 && A <= MMS_PPO_LOSS_MAX_A;
    const int64_t need = shapes ? mms::ppo_loss_ws_bytes(M, A) : 0;
    if (refused(check_ppo_loss(M, A, mu, log_std, value, actions, old_logp, adv, returns, target_values, old_mu, old_sigma, out, dmu, dlog_std, dvalue,
                               workspace, ws_bytes, need)))
        return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    MMS_FREE(mms::launch_ppo_loss(M, A, mu, log_std, value, indices, actions, old_logp, adv, returns, target_values, old_mu, old_sigma, clip, value_coef,
                                  entropy_coef, clipped_value, out, dmu, dlog_std, dvalue, workspace, (hipStream_t)s));
    return 0;
}

// ---- the head of TRPO's policy step (trpo_loss_kernels.hip) -------------------------------------------------------------------------

__attribute__((visibility("default"))) int mms_trpo_heads(int device, int64_t M, int32_t A, const float* mu, const float* log_std, const float* rmu,
                                                          const int64_t* indices, const float* actions, const float* adv, const float* old_mu,
                                                          const float* old_sigma, const float* old_logp, int32_t old_logp_dense, float* out,
                                                          float* logp, float* gsur, float* gkl, float* gn, void* workspace, int64_t* ws_bytes,
                                                          void* s) {
    MMS_DEV(device)
    const bool shapes = M >= 1 && M <= 0x7fffffff && A >= 1 && A <= MMS_PPO_LOSS_MAX_A;
    const int64_t need = shapes ? mms::trpo_heads_ws_bytes(M, A) : 0;
    if (refused(check_trpo_heads(M, A, mu, log_std, rmu, actions, adv, old_mu, old_sigma, old_logp, out, logp, gsur, gkl, gn, workspace, ws_bytes, need)))
        return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    MMS_FREE(mms::launch_trpo_heads(M, A, mu, log_std, rmu, indices, actions, adv, old_mu, old_sigma, old_logp, old_logp_dense != 0, out, logp, gsur, gkl,
                                    gn, workspace, (hipStream_t)s));
    return 0;
}

// ---- the MAPPO / HAPPO update's loss head (marl_loss_kernels.hip) -----------------------------------------------------------------

__attribute__((visibility("default"))) int mms_marl_ppo_loss(int device, int64_t M, int32_t A, const float* mu, const float* std, const float* value,
                                                             const int64_t* indices, const mms_marl_loss_fields* fields, float clip,
                                                             float value_loss_coef, float entropy_coef, float huber_delta, int32_t use_huber,
                                                             int32_t clipped_value, int32_t policy_masks, int32_t value_masks, int32_t use_norm,
                                                             const float* norm_mean, const float* norm_var, float* out, float* dmu, float* dstd,
                                                             float* dvalue, float* row_logp, void* workspace, int64_t* ws_bytes, void* s) {
    MMS_DEV(device)
    const bool shapes = M >= 1 && M <= 0x7fffffff && A >= 1 && A <= MMS_MARL_LOSS_MAX_A;
    const int64_t need = shapes ? mms::marl_loss_ws_bytes(M, A) : 0;
    if (refused(check_marl_ppo_loss(M, A, mu, std, value, fields, policy_masks, value_masks, use_norm, norm_mean, norm_var, out, dmu, dstd, dvalue,
                                    workspace, ws_bytes, need)))
        return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    MMS_FREE(mms::launch_marl_ppo_loss(M, A, mu, std, value, indices, *fields, clip, value_loss_coef, entropy_coef, huber_delta, use_huber, clipped_value,
                                       policy_masks, value_masks, use_norm, norm_mean, norm_var, out, dmu, dstd, dvalue, row_logp, workspace,
                                       (hipStream_t)s));
    return 0;
}

__attribute__((visibility("default"))) int mms_marl_ppo_loss_group(int device, int32_t groups, int64_t M, int32_t A, const mms_marl_loss_group* table,
                                                                   float clip, float value_loss_coef, float entropy_coef, float huber_delta,
                                                                   int32_t use_huber, int32_t clipped_value, int32_t policy_masks, int32_t value_masks,
                                                                   int32_t use_norm, void* workspace, int64_t* ws_bytes, void* s) {
    MMS_DEV(device)
    const bool shapes = groups >= 1 && groups <= MMS_MAX_GROUPS && M >= 1 && M <= 0x7fffffff && A >= 1 && A <= MMS_MARL_LOSS_MAX_A;
    const int64_t need = shapes ? mms::marl_loss_group_ws_bytes(groups, M, A) : 0;
    if (refused(check_marl_ppo_loss_group(groups, M, A, table, policy_masks, value_masks, use_norm, workspace, ws_bytes, need))) return 1;
    if (!workspace) { *ws_bytes = need; return 0; }                // the size query
    MMS_FREE(mms::launch_marl_ppo_loss_group(groups, M, A, table, clip, value_loss_coef, entropy_coef, huber_delta, use_huber, clipped_value, policy_masks,
                                             value_masks, use_norm, workspace, (hipStream_t)s));
    return 0;
}

}  // extern "C"
