// mms_cpu.cpp -- the CPU build of the engine behind the SAME C ABI (include/mms.h): lib/libmms_cpu.so.
//
// What it is for: the reference selects a CPU pipeline with `--sim_device cpu` (agents/tasks/agent_base/base_task.py:27-32,
// vec_task.py:126-139; BASELINE configs[0] "OneAnt num_envs=64 ... sim_device=cpu -- plumbing, no GPU").  This library is that
// pipeline: explicit and opt-in (mms_config.device = -1, `device_type="cpu"` in the task constructors), NEVER a fallback -- the
// HIP library still fails without a GPU and nothing selects this one automatically.
// What it is built from: the per-lane functions of the HIP step kernels (../mms_lane.h through lane_step.h) and the per-column
// functions of the rollout kernels (../rollout_lane.h) -- the product's own math, compiled for the host, OpenMP over envs.
// It shares no source with the oracle (oracle/mms_oracle.c), which stays the checker.
// Streams: the `hip_stream` arguments are ignored; every call has completed when it returns.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../mms_host.h"
#include "../rollout_lane.h"
#include "../ppo_loss_lane.h"
#include "../trpo_loss_lane.h"
#include "../marl_loss_lane.h"
#include "../q_lane.h"
#include "../q_loss_lane.h"
#include "../maddpg_lane.h"
#include "../sac_lane.h"
#include "../sac_grad_lane.h"
#include "../det_head_lane.h"
#include "../gru_lane.h"
#include "../gru_grad_lane.h"
#include "../elu_ln_lane.h"
#include "../marl_heads_grad_lane.h"
#include "../marl_eval_lane.h"
#include "lane_step.h"

#define MMS_API extern "C" __attribute__((visibility("default")))

struct mms_engine : mms_host_state {};

template <typename T> static T* buf(mms_engine* e, const char* name) { return (T*)find(e, name)->ptr; }

MMS_API int mms_abi_version(void) { return MMS_ABI_VERSION; }
MMS_API const char* mms_last_error(mms_handle h) { return h ? h->err.c_str() : g_error.c_str(); }

MMS_API int mms_destroy(mms_handle h) {
    if (!h) return 0;
    for (auto& b : h->bufs) free(b.ptr);
    delete h;
    return 0;
}

MMS_API int mms_create(const mms_config* cfg, mms_handle* out) {
    mms_engine* e = new mms_engine();
    std::string bad = engine_init(e, cfg, out);
    if (bad.empty() && cfg->device != -1) bad = "mms_create: this is the CPU build of the engine (libmms_cpu.so); device must be -1";
    if (!bad.empty()) { delete e; return fail(nullptr, bad); }
    e->bufs = buffer_table(*e);
    for (auto& b : e->bufs) b.ptr = calloc(b.bytes ? b.bytes : 16, 1);
    fill_scene(*e, buf<float>(e, "initial_root_states"), buf<float>(e, "env_origin"), buf<float>(e, "prev"), buf<int64_t>(e, "reset"), buf<float>(e, "dr_params"));
    memcpy(buf<float>(e, "root_states"), buf<float>(e, "initial_root_states"), find(e, "root_states")->bytes);
    *out = e;
    return 0;
}

MMS_API int mms_get_tensor(mms_handle h, const char* name, mms_tensor* out) { return host_get_tensor(h, name, out); }

MMS_API int mms_ppo_heads_act(int device, const float* hidden, const float* weight, const float* bias, int32_t H, const float* value,
                              const float* vhidden, const float* vweight, const float* vbias, int32_t VH, const float* log_std, uint64_t seed,
                              int64_t* counters, int64_t row_offset, int32_t reference_scale, float* actions_out, float* act_slot,
                              float* logp_slot, float* value_slot, float* mu_slot, float* sigma_slot, int64_t N, int32_t A, void*);

static int do_step(mms_handle h, int physics) {
    if (null_handle(h, "mms_step")) return 1;
    const float* head_actions = nullptr;
    if (physics && h->head_on) {
        // the fused policy head (mms_bind_policy_head): on the host the heads operator runs in front of the step, into the action tensor
        // the step then reads -- the same values as the two calls made separately
        const mms_policy_head& p = h->head;
        float* dst = p.actions_out ? p.actions_out : buf<float>(h, "actions");
        h->head_on = false;
        // (with the tiled copy of the actor's last layer bound, THAT is what is read -- as on the device; element
        //  ((ct (H / 4) + k / 4) 16 + i) 4 + k % 4 = weight[16 ct + i][k] -- so a stale or mis-laid copy shows up in the host tests too)
        std::vector<float> untiled;
        if (p.weight_tiles) {
            untiled.resize((size_t)p.A * p.H);
            for (int j = 0; j < p.A; j++)
                for (int k = 0; k < p.H; k++)
                    untiled[(size_t)j * p.H + k] = p.weight_tiles[((size_t)((j >> 4) * (p.H / 4) + (k >> 2)) * 16 + (j & 15)) * 4 + (k & 3)];
        }
        if (mms_ppo_heads_act(-1, p.hidden, p.weight_tiles ? untiled.data() : p.weight, p.bias, p.H, nullptr, p.vhidden, p.vweight, p.vbias, p.VH, p.log_std, p.seed, p.counters, p.row_offset,
                              p.reference_scale, dst, p.act_slot, p.logp_slot, p.value_slot, p.mu_slot, p.sigma_slot, h->cfg.num_envs, p.A, nullptr))
            return fail(h, "mms_step: the bound policy head failed: " + g_error);
        head_actions = dst;
    }
    mms::HostBufs b{head_actions ? const_cast<float*>(head_actions) : (h->actions_in ? const_cast<float*>(h->actions_in) : buf<float>(h, "actions")), h->write_raw_obs ? buf<float>(h, "obs") : nullptr,
                    h->write_clipped_obs ? buf<float>(h, "obs_clipped") : nullptr, buf<float>(h, "rew"), buf<int64_t>(h, "reset"),
                    buf<int64_t>(h, "progress"), buf<float>(h, "root_states"), buf<float>(h, "initial_root_states"),
                    buf<float>(h, "dof_state"), buf<float>(h, "env_origin"), buf<float>(h, "prev"), buf<float>(h, "reset_noise"),
                    buf<float>(h, "foot_sensors"), buf<int64_t>(h, "reset_count"), h->dr_enabled ? buf<float>(h, "dr_params") : nullptr};
    b.obs_out = h->obs_out; b.rew_out = h->rew_out; b.done_out = h->done_out;
    b.obs_planes = (uint16_t*)h->obs_planes; b.obs_planes_scale = h->obs_planes_scale;
    const mms_config* C = &h->cfg;
#pragma omp parallel for schedule(static)
    for (int env = 0; env < C->num_envs; env++) {
        if (C->task == MMS_TASK_MULTI_INGENUITY) mms::host_heli_env(C, b, env, physics);
        else mms::host_ant_env(C, b, env, physics, h->obs_dim, h->prev_dim);
    }
    return 0;
}
MMS_API int mms_step(mms_handle h, void*) { return do_step(h, 1); }
MMS_API int mms_post_step(mms_handle h, void*) { return do_step(h, 0); }

MMS_API int mms_reset_all(mms_handle h, void*) {
    if (null_handle(h, "mms_reset_all")) return 1;
    int64_t* r = buf<int64_t>(h, "reset");
    for (int i = 0; i < h->cfg.num_envs; i++) r[i] = 1;
    return 0;
}

MMS_API int mms_set_state(mms_handle h, const char* name, const void* src, int, const int64_t* env_ids, int64_t n, void*) {
    mms_buffer* b = nullptr;
    if (host_set_state_check(h, name, src, env_ids, n, &b)) return 1;
    if (!env_ids) { memcpy(b->ptr, src, b->bytes); return 0; }
    for (int64_t i = 0; i < n; i++) memcpy((char*)b->ptr + env_ids[i] * b->row_bytes, (const char*)src + i * b->row_bytes, (size_t)b->row_bytes);
    return 0;
}

MMS_API int mms_bind_obs_out(mms_handle h, void* dst) { return host_bind_obs_out(h, dst); }
MMS_API int mms_bind_obs_planes16(mms_handle h, void* planes, float scale) { return host_bind_obs_planes16(h, planes, scale); }
MMS_API int mms_bind_actions(mms_handle h, const float* src) { return host_bind_actions(h, src); }
MMS_API int mms_set_dr(mms_handle h, int32_t enable) { return host_set_dr(h, enable); }
MMS_API int mms_set_obs_outputs(mms_handle h, int32_t raw, int32_t clipped) { return host_set_obs_outputs(h, raw, clipped); }
MMS_API int mms_bind_rollout_out(mms_handle h, float* rew_out, uint8_t* done_out) { return host_bind_rollout_out(h, rew_out, done_out); }
MMS_API int mms_bind_policy_head(mms_handle h, const mms_policy_head* head) {
    // the heads operator runs in front of the host step wherever the engine has the shape of the device's fused layout
    return host_bind_policy_head(h, head, h && h->cfg.task == MMS_TASK_TEN_ANT && h->cfg.num_agents == 10 && h->cfg.num_envs % 16 == 0);
}

// ---- rollout functions (device argument: -1) ---------------------------------------------------------------------------------
static int cpu_only(int device) {
    if (device != -1) { g_error = "libmms_cpu.so: device must be -1"; return 1; }
    return 0;
}
MMS_API int mms_marl_views(int device, const float* obs_clipped, float* obs_all, int64_t n, int32_t agents, int32_t per_agent, int32_t shared, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_marl_views(obs_clipped, obs_all, n, agents, per_agent, shared))) return 1;
    const int64_t total = n * agents * (per_agent + shared);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < total; i++) obs_all[i] = obs_clipped[mms::marl_view_source(i, agents, per_agent, shared)];
    return 0;
}
MMS_API int mms_gae_ppo(int device, const float* rewards, const uint8_t* dones, const float* values, const float* last_values, float* returns,
                        float* advantages, double* stats, int32_t T, int64_t N, float gamma, float lam, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_gae_ppo(rewards, dones, values, last_values, returns, advantages, stats, T, N))) return 1;
    // partial sums per 256 columns (a block of the device's launch), added in order: the result does not depend on the number of threads
    // or on the order in which they finish (an OpenMP reduction's does), so mms_gae_ppo_normalized is bit-reproducible here as well
    const int64_t chunks = (N + 255) / 256;
    std::vector<double> psum((size_t)chunks), psq((size_t)chunks);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < chunks; c++) {
        double s = 0.0, q = 0.0;
        const int64_t end = (c + 1) * 256 < N ? (c + 1) * 256 : N;
        for (int64_t i = c * 256; i < end; i++) mms::gae_ppo_column(rewards, dones, values, last_values, returns, advantages, T, N, i, gamma, lam, s, q);
        psum[(size_t)c] = s; psq[(size_t)c] = q;
    }
    double sum = 0.0, sq = 0.0;
    for (int64_t c = 0; c < chunks; c++) { sum += psum[(size_t)c]; sq += psq[(size_t)c]; }
    stats[0] = sum; stats[1] = sq; stats[2] = (double)T * (double)N;
    return 0;
}
MMS_API int mms_adv_normalize(int device, float* advantages, const double* stats, int64_t count, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_adv_normalize(advantages, stats, count))) return 1;
    float fm, inv;
    mms::adv_norm_params(stats, fm, inv);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < count; i++) advantages[i] = (advantages[i] - fm) * inv;
    return 0;
}
MMS_API int mms_layer_clock_probe(int device, uint64_t* out, int32_t slots) {
    (void)device;
    if (refused(check_layer_clock_probe(out, slots))) return 1;
    return 0;                                     // (no shader clock on this build: nothing is stored)
}

MMS_API int mms_gae_ppo_normalized(int device, const float* rewards, const uint8_t* dones, const float* values, const float* last_values, float* returns,
                                   float* advantages, double* stats, int32_t T, int64_t N, float gamma, float lam, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_gae_ppo_normalized(rewards, dones, values, last_values, returns, advantages, stats, T, N))) return 1;
    if (mms_gae_ppo(device, rewards, dones, values, last_values, returns, advantages, stats, T, N, gamma, lam, nullptr)) return 1;
    return mms_adv_normalize(device, advantages, stats, (int64_t)T * N, nullptr);
}
MMS_API int mms_gae_marl(int device, const float* rewards, const float* value_preds, const float* masks, float* returns, int32_t T, int64_t N,
                         float gamma, float lam, int32_t use_norm, const float* norm_mean, const float* norm_var, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_gae_marl("mms_gae_marl", rewards, value_preds, masks, returns, T, N, 1, use_norm, norm_mean, norm_var))) return 1;
    const float mean = use_norm ? norm_mean[0] : 0.f, var = use_norm ? norm_var[0] : 1.f;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < N; i++) mms::gae_marl_column(rewards, value_preds, masks, returns, T, N, N, i, i, gamma, lam, use_norm, mean, var);
    return 0;
}
MMS_API int mms_gae_marl_agents(int device, const float* rewards, const float* value_preds, const float* masks, float* returns, int32_t T,
                                int64_t N, int32_t A, float gamma, float lam, int32_t use_norm, const float* norm_mean, const float* norm_var, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_gae_marl("mms_gae_marl_agents", rewards, value_preds, masks, returns, T, N, A, use_norm, norm_mean, norm_var))) return 1;
    const int64_t cols = N * A;
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < cols; c++) {
        const int64_t i = c / A;
        const int k = (int)(c - i * A);
        mms::gae_marl_column(rewards, value_preds, masks, returns, T, N, cols, c, i, gamma, lam, use_norm, use_norm ? norm_mean[k] : 0.f,
                             use_norm ? norm_var[k] : 1.f);
    }
    return 0;
}

// one row of ActorCritic.act's sampling tail + the add_transitions stores (module.py:73-87, storage.py:33-47)
static void sample_row(const float* mean_row, float value_now, bool have_value, const float* log_std, uint64_t seed, int64_t* counters,
                       int64_t row_offset, int ref_scale, float* actions_out, float* act_slot, float* logp_slot, float* value_slot,
                       float* mu_slot, float* sigma_slot, int64_t row, int A) {
    const int64_t c = counters[row];
    // the wave's butterfly sum of the GPU kernel (lane j holds actions j, j + 64; xor 32, 16, ... 1), reproduced on 64 slots
    float lane[64];
    for (int l = 0; l < 64; l++) lane[l] = 0.f;
    for (int j = 0; j < A; j++) {
        float term;
        const float act = mms::ppo_sample_one(mean_row[j], log_std[j], seed, (uint64_t)(row_offset + row), (uint64_t)c, (uint32_t)j, ref_scale, term);
        lane[j & 63] += term;
        if (actions_out) actions_out[row * A + j] = act;
        if (act_slot) act_slot[row * A + j] = act;
        if (mu_slot) mu_slot[row * A + j] = mean_row[j];
        if (sigma_slot) sigma_slot[row * A + j] = log_std[j];
    }
    for (int m = 32; m >= 1; m >>= 1) {
        float nxt[64];
        for (int l = 0; l < 64; l++) nxt[l] = lane[l] + lane[l ^ m];
        memcpy(lane, nxt, sizeof(lane));
    }
    if (logp_slot) logp_slot[row] = lane[0];
    if (value_slot && have_value) value_slot[row] = value_now;
    counters[row] = c + 1;
}
MMS_API int mms_ppo_act(int device, const float* mean, const float* value, const float* log_std, uint64_t seed, int64_t* counters,
                        int64_t row_offset, int32_t reference_scale, float* actions_out, float* act_slot, float* logp_slot, float* value_slot,
                        float* mu_slot, float* sigma_slot, int64_t N, int32_t A, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_ppo_act(mean, log_std, counters, N, A))) return 1;
#pragma omp parallel for schedule(static)
    for (int64_t row = 0; row < N; row++)
        sample_row(mean + row * A, value ? value[row] : 0.f, value != nullptr, log_std, seed, counters, row_offset, reference_scale, actions_out,
                   act_slot, logp_slot, value_slot, mu_slot, sigma_slot, row, A);
    return 0;
}
MMS_API int mms_ppo_heads_act(int device, const float* hidden, const float* weight, const float* bias, int32_t H, const float* value,
                              const float* vhidden, const float* vweight, const float* vbias, int32_t VH, const float* log_std, uint64_t seed,
                              int64_t* counters, int64_t row_offset, int32_t reference_scale, float* actions_out, float* act_slot,
                              float* logp_slot, float* value_slot, float* mu_slot, float* sigma_slot, int64_t N, int32_t A, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_ppo_heads_act(hidden, weight, bias, H, vhidden, vweight, vbias, VH, log_std, counters, N, A))) return 1;
#pragma omp parallel for schedule(static)
    for (int64_t row = 0; row < N; row++) {
        float mean[128];
        for (int j = 0; j < A; j++) {
            float s = 0.f;
            for (int k = 0; k < H; k++) s = fmaf(hidden[row * (int64_t)H + k], weight[(int64_t)j * H + k], s);
            mean[j] = s + bias[j];
        }
        float v = value ? value[row] : 0.f;
        if (vhidden) {
            float s = 0.f;
            for (int k = 0; k < VH; k++) s = fmaf(vhidden[row * (int64_t)VH + k], vweight[k], s);
            v = s + vbias[0];
        }
        sample_row(mean, v, vhidden != nullptr || value != nullptr, log_std, seed, counters, row_offset, reference_scale, actions_out, act_slot,
                   logp_slot, value_slot, mu_slot, sigma_slot, row, A);
    }
    return 0;
}
MMS_API int mms_sac_heads_act(int device, const float* hidden, int32_t H, const float* mu_weight, const float* mu_bias, const float* ls_weight,
                              const float* ls_bias, float act_limit, float epsilon, int32_t deterministic, uint64_t seed, int64_t* counters,
                              int64_t row_offset, float* actions_out, float* act_slot, float* logp_slot, float* u_slot, float* mu_slot,
                              float* log_std_slot, int64_t N, int32_t A, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_sac_heads_act(hidden, H, mu_weight, mu_bias, ls_weight, ls_bias, deterministic, counters, N, A))) return 1;
    const bool want_logp = logp_slot != nullptr;
#pragma omp parallel for schedule(static)
    for (int64_t row = 0; row < N; row++) {
        const float* h = hidden + row * (int64_t)H;
        const int64_t c = deterministic ? 0 : counters[row];
        float lane[64];                     // the kernel's wave butterfly (lane j holds actions j, j + 64; xor 32, 16, ... 1)
        for (int l = 0; l < 64; l++) lane[l] = 0.f;
        for (int j = 0; j < A; j++) {
            float mu = 0.f, ls = 0.f;
            for (int k = 0; k < H; k++) mu = fmaf(h[k], mu_weight[(int64_t)j * H + k], mu);
            for (int k = 0; k < H; k++) ls = fmaf(h[k], ls_weight[(int64_t)j * H + k], ls);
            mu += mu_bias[j];
            float u, lsc, term;
            const float act = mms::sac_sample_one(mu, ls + ls_bias[j], deterministic, seed, (uint64_t)(row_offset + row), (uint64_t)c, (uint32_t)j,
                                                  act_limit, epsilon, want_logp, u, lsc, term);
            lane[j & 63] += term;
            const int64_t at = row * A + j;
            if (actions_out) actions_out[at] = act;
            if (act_slot) act_slot[at] = act;
            if (u_slot) u_slot[at] = u;
            if (mu_slot) mu_slot[at] = mu;
            if (log_std_slot) log_std_slot[at] = lsc;
        }
        if (want_logp) {
            for (int m = 32; m >= 1; m >>= 1) {
                float nxt[64];
                for (int l = 0; l < 64; l++) nxt[l] = lane[l] + lane[l ^ m];
                memcpy(lane, nxt, sizeof(lane));
            }
            logp_slot[row] = lane[0];
        }
        if (!deterministic) counters[row] = c + 1;
    }
    return 0;
}
MMS_API int mms_q_heads_backup(int device, int64_t M, int32_t H, const float* h0, const float* w0, const float* b0, float* q0_out, const float* h1,
                               const float* w1, const float* b1, float* q1_out, const float* reward, const uint8_t* done, const float* logp,
                               float gamma, float alpha, float* backup, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_q_heads_backup(M, H, h0, w0, b0, q0_out, h1, w1, b1, q1_out, reward, done, backup))) return 1;
    const int G = h1 ? 2 : 1;
    const float* hs[2] = {h0, h1};
    const float* ws[2] = {w0, w1};
    const float* bs[2] = {b0, b1};
    float* qs[2] = {q0_out, q1_out};
#pragma omp parallel for schedule(static)
    for (int64_t row = 0; row < M; row++) {
        float q[2] = {0.f, 0.f};
        for (int g = 0; g < G; g++) {
            float s = 0.f;
            for (int k = 0; k < H; k++) s = fmaf(hs[g][row * (int64_t)H + k], ws[g][k], s);
            q[g] = mms::q_value(s, bs[g][0]);
            if (qs[g]) qs[g][row] = q[g];
        }
        if (backup) {
            const float qm = G == 2 ? mms::q_min(q[0], q[1]) : q[0];
            backup[row] = mms::q_backup(reward[row], done[row], qm, logp != nullptr, logp ? logp[row] : 0.f, gamma, alpha);
        }
    }
    return 0;
}
// The loss heads with a gradient (include/mms.h: mms_q_heads_loss) over ../q_loss_lane.h: the HIP kernel's partition and its order of
// every double sum (q_loss_partition, q_loss_slot_sum, the finish pass's segments), OpenMP over the workgroups, so dw, db and the loss
// are the HIP build's bits wherever q is; q is this build's mms_q_heads_backup chain.  No workspace.
template <int G>
static void q_heads_loss_cpu(int64_t M, int H, const float* const* hs, const float* const* ws, const float* const* bs, int mode, const float* target,
                             const float* logp, float alpha, float scale, float* loss, float* const* qs, float* const* dhs, float* const* dws,
                             float* const* dbs) {
    const mms::QLossPartition p = mms::q_loss_partition(M, H);
    const int NC = mms::q_loss_columns(G, H);
    std::vector<double> part((size_t)p.blocks * NC, 0.0);
#pragma omp parallel for schedule(static)
    for (int64_t blk = 0; blk < p.blocks; blk++) {
        std::vector<double> slot((size_t)NC * mms::kQLossRows, 0.0);          // [column][row slot]
        for (int64_t it = 0; it < p.iters; it++)
            for (int r = 0; r < mms::kQLossRows; r++) {
                const int64_t row = (blk * p.iters + it) * mms::kQLossRows + r;
                if (row >= M) continue;
                float q[2] = {0.f, 0.f};
                double dq[2] = {0.0, 0.0};
                for (int g = 0; g < G; g++) {
                    float s = 0.f;
                    for (int k = 0; k < H; k++) s = fmaf(hs[g][row * (int64_t)H + k], ws[g][k], s);
                    q[g] = mms::q_value(s, bs[g][0]);
                    if (qs[g]) qs[g][row] = q[g];
                }
                const double term = mms::q_loss_row<G>(mode, q, mode == 0 ? target[row] : 0.f, logp != nullptr, logp ? logp[row] : 0.f, alpha, scale,
                                                       (double)M, dq);
                slot[(size_t)(NC - 1) * mms::kQLossRows + r] += term;
                for (int g = 0; g < G; g++) {
                    const float* x = hs[g] + row * (int64_t)H;
                    if (dhs[g])
                        for (int k = 0; k < H; k++) dhs[g][row * (int64_t)H + k] = mms::q_loss_dh(mode, dq[g], ws[g][k]);
                    if (dws[g]) {
                        double* c = slot.data() + (size_t)g * (H + 1) * mms::kQLossRows;
                        const double d = dq[g];
                        for (int k = 0; k < H; k++) c[(size_t)k * mms::kQLossRows + r] += d * (double)x[k];
                        c[(size_t)H * mms::kQLossRows + r] += d;
                    }
                }
            }
        for (int c = 0; c < NC; c++) part[(size_t)blk * NC + c] = mms::q_loss_slot_sum(slot.data() + (size_t)c * mms::kQLossRows);
    }
    for (int c = 0; c < NC; c++) {
        float* dst = nullptr;
        if (c == NC - 1) dst = loss;
        else if (dws[c / (H + 1)]) dst = c % (H + 1) < H ? dws[c / (H + 1)] + c % (H + 1) : dbs[c / (H + 1)];
        if (!dst) continue;
        double t = 0.0;
        for (int seg = 0; seg < mms::kQLossSegments; seg++) {
            const int64_t first = seg * p.per_segment, last = first + p.per_segment < p.blocks ? first + p.per_segment : p.blocks;
            t += first < last ? mms::q_loss_segment_sum(part.data() + c, NC, first, last) : 0.0;
        }
        *dst = c == NC - 1 ? (float)(t / (double)M) : (float)t;
    }
}
MMS_API int mms_q_heads_loss(int device, int64_t M, int32_t H, const float* h0, const float* w0, const float* b0, const float* h1, const float* w1,
                             const float* b1, int32_t mode, const float* target, const float* logp, float alpha, float scale, float* loss,
                             float* q0_out, float* q1_out, float* dh0, float* dh1, float* dw0, float* db0, float* dw1, float* db1, void* workspace,
                             int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_q_heads_loss(M, H, h0, w0, b0, h1, w1, b1, mode, target, loss, q1_out, dh0, dh1, dw0, db0, dw1, db1, workspace, ws_bytes, 0))) return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }                  // the size query
    const float* hs[2] = {h0, h1};
    const float* ws[2] = {w0, w1};
    const float* bs[2] = {b0, b1};
    float* qs[2] = {q0_out, q1_out};
    float* dhs[2] = {dh0, dh1};
    float* dws[2] = {dw0, dw1};
    float* dbs[2] = {db0, db1};
    if (mode == 1) target = nullptr;
    else logp = nullptr;
    if (h1) q_heads_loss_cpu<2>(M, H, hs, ws, bs, mode, target, logp, alpha, scale, loss, qs, dhs, dws, dbs);
    else q_heads_loss_cpu<1>(M, H, hs, ws, bs, mode, target, logp, alpha, scale, loss, qs, dhs, dws, dbs);
    return 0;
}
MMS_API int mms_det_heads_act_group(int device, int32_t groups, int64_t M, int32_t H, int32_t A, int32_t agent0, const float* const* h,
                                    const float* const* w, const float* const* b, const float* act_limit, float sigma, uint64_t seed,
                                    int64_t* counters, int64_t row_offset, float* const* act_out, int64_t act_pitch, float* joint_out,
                                    int64_t joint_pitch, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_det_heads_act_group(groups, M, H, A, agent0, h, w, b, act_limit, sigma, counters, act_out, act_pitch, joint_out, joint_pitch))) return 1;
    const bool noisy = sigma > 0.f;
#pragma omp parallel for schedule(static)
    for (int64_t row = 0; row < M; row++) {
        const int64_t c = noisy ? counters[row] : 0;
        for (int g = 0; g < groups; g++) {
            const float* x = h[g] + row * (int64_t)H;
            float* out = act_out ? act_out[g] : nullptr;
            const int64_t jcol0 = (int64_t)(agent0 + g) * A;
            for (int k = 0; k < A; k++) {
                float s = 0.f;
                for (int j = 0; j < H; j++) s = fmaf(x[j], w[g][(int64_t)k * H + j], s);
                float act = mms::det_action(s + b[g][k], act_limit[g]);
                if (noisy) act = mms::det_explore(act, sigma, seed, (uint64_t)(row_offset + row), (uint64_t)c, (uint32_t)(jcol0 + k), act_limit[g]);
                if (out) out[row * act_pitch + k] = act;
                if (joint_out) joint_out[row * joint_pitch + jcol0 + k] = act;
            }
        }
        if (noisy) counters[row] = c + 1;
    }
    return 0;
}
// One deterministic actor head (include/mms.h: mms_det_heads_act): the grouped loop above for one network -- the same fmaf chain, so the
// same bits as mms_det_heads_act_group(groups = 1, agent0 = 0) of this build -- with tanh(pre) kept and the clipped smoothing noise.
MMS_API int mms_det_heads_act(int device, int64_t M, int32_t H, int32_t A, const float* h, const float* w, const float* b, float act_limit, float sigma,
                              float noise_clip, uint64_t seed, int64_t* counters, int64_t row_offset, float* act_out, int64_t act_pitch, float* tanh_out,
                              void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_det_heads_act(M, H, A, h, w, b, act_limit, sigma, noise_clip, counters, act_out, act_pitch, tanh_out))) return 1;
    const bool noisy = sigma > 0.f;
    const float clip = det_noise_clip(noise_clip);
#pragma omp parallel for schedule(static)
    for (int64_t row = 0; row < M; row++) {
        const int64_t c = noisy ? counters[row] : 0;
        const float* x = h + row * (int64_t)H;
        for (int k = 0; k < A; k++) {
            float s = 0.f;
            for (int j = 0; j < H; j++) s = fmaf(x[j], w[(int64_t)k * H + j], s);
            const float pre = s + b[k];
            float act = mms::det_action(pre, act_limit);
            if (tanh_out) tanh_out[row * A + k] = tanhf(pre);
            if (noisy)
                act = clip >= 0.f ? mms::det_smooth(act, sigma, clip, seed, (uint64_t)(row_offset + row), (uint64_t)c, (uint32_t)k, act_limit)
                                  : mms::det_explore(act, sigma, seed, (uint64_t)(row_offset + row), (uint64_t)c, (uint32_t)k, act_limit);
            if (act_out) act_out[row * act_pitch + k] = act;
        }
        if (noisy) counters[row] = c + 1;
    }
    return 0;
}
// The backward of that head's epilogue (include/mms.h: mms_det_heads_grad) over ../det_head_lane.h, on mms_sac_heads_grad's plan below:
// rows in at most 1024 chunks of at least 256 (OpenMP over chunks), a chunk's column sums in double over ascending rows, the chunks
// added in ascending order and rounded once -- the result does not depend on the number of threads.  No workspace.
MMS_API int mms_det_heads_grad(int device, int64_t N, int32_t A, float act_limit, const float* t, const float* g, int64_t grad_pitch, float* dy,
                               float* dbias, void* workspace, int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_det_heads_grad(N, A, t, g, grad_pitch, dy, workspace, ws_bytes, 0))) return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }                  // the size query
    if (N == 0) return 0;
    int64_t chunk = (N + 1023) / 1024;
    chunk = chunk < 256 ? 256 : chunk;
    const int64_t nchunks = (N + chunk - 1) / chunk;
    std::vector<double> part(dbias ? (size_t)nchunks * A : 0, 0.0);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < nchunks; c++) {
        double* p = dbias ? part.data() + c * A : nullptr;
        const int64_t end = (c + 1) * chunk < N ? (c + 1) * chunk : N;
        for (int64_t row = c * chunk; row < end; row++)
            for (int j = 0; j < A; j++) {
                const float d = mms::det_head_grad_one(t[row * A + j], g[row * grad_pitch + j], act_limit);
                dy[row * A + j] = d;
                if (p) p[j] += (double)d;
            }
    }
    if (dbias)
        for (int q = 0; q < A; q++) {
            double s = 0.0;
            for (int64_t c = 0; c < nchunks; c++) s += part[c * A + q];
            dbias[q] = (float)s;
        }
    return 0;
}
MMS_API int mms_q_heads_backup_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* h, const float* const* w,
                                     const float* const* b, float* const* q_out, const float* const* reward, const uint8_t* const* done,
                                     float gamma, float* const* backup, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_q_heads_backup_group(groups, M, H, h, w, b, q_out, reward, done, backup))) return 1;
#pragma omp parallel for schedule(static)
    for (int64_t row = 0; row < M; row++) {
        for (int g = 0; g < groups; g++) {
            float s = 0.f;                  // mms_q_heads_backup's chain for one network
            for (int k = 0; k < H; k++) s = fmaf(h[g][row * (int64_t)H + k], w[g][k], s);
            const float q = mms::q_value(s, b[g][0]);
            if (q_out && q_out[g]) q_out[g][row] = q;
            if (backup && backup[g]) backup[g][row] = mms::q_backup(reward[g][row], done[g][row], q, false, 0.f, gamma, 0.f);
        }
    }
    return 0;
}
// The backward of the head's epilogue (include/mms.h: mms_sac_heads_grad) over ../sac_grad_lane.h.  Rows in at most 1024 chunks of at
// least 256 (OpenMP over chunks): a chunk's column sums in double over ascending rows, the chunks added in ascending order and rounded
// once -- the result does not depend on the number of threads.  No workspace.
MMS_API int mms_sac_heads_grad(int device, int64_t N, int32_t A, float act_limit, float epsilon, const float* u, const float* mu, const float* log_std,
                               const float* grad_action, const float* grad_logp, float* dy, float* dbias, void* workspace, int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_sac_heads_grad(N, A, u, mu, log_std, grad_action, grad_logp, dy, workspace, ws_bytes, 0))) return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }                  // the size query
    if (N == 0) return 0;
    const int C = 2 * A;
    int64_t chunk = (N + 1023) / 1024;
    chunk = chunk < 256 ? 256 : chunk;
    const int64_t nchunks = (N + chunk - 1) / chunk;
    std::vector<double> part(dbias ? (size_t)nchunks * C : 0, 0.0);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < nchunks; c++) {
        double* p = dbias ? part.data() + c * C : nullptr;
        const int64_t end = (c + 1) * chunk < N ? (c + 1) * chunk : N;
        for (int64_t row = c * chunk; row < end; row++) {
            const float g_l = grad_logp ? grad_logp[row] : 0.f;
            for (int j = 0; j < A; j++) {
                const int64_t e = row * A + j;
                float dmu, dls;
                mms::sac_grad_one(u[e], mu[e], log_std[e], grad_action ? grad_action[e] : 0.f, g_l, act_limit, epsilon, dmu, dls);
                dy[row * C + j] = dmu;
                dy[row * C + A + j] = dls;
                if (p) { p[j] += (double)dmu; p[A + j] += (double)dls; }
            }
        }
    }
    if (dbias)
        for (int q = 0; q < C; q++) {
            double s = 0.0;
            for (int64_t c = 0; c < nchunks; c++) s += part[c * C + q];
            dbias[q] = (float)s;
        }
    return 0;
}
MMS_API int64_t mms_param_step_partials(int32_t tensors, const int64_t* numel) { return param_step_partials(tensors, numel); }
// The HIP build's two passes over its chunk tables (param_step_args.h), a chunk per loop iteration: the partials are added in index
// order, so the result does not depend on the number of threads.
MMS_API int mms_param_step(int device, int32_t tensors, const int64_t* numel, float* const* param, const float* const* grad, float* const* exp_avg,
                           float* const* exp_avg_sq, float* const* target, double lr, double beta1, double beta2, double eps, double weight_decay,
                           int64_t step, double max_norm, double polyak, int32_t flags, double* partials, float* norm_out, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_param_step(tensors, numel, param, grad, exp_avg, exp_avg_sq, target, lr, beta1, beta2, eps, weight_decay, step, max_norm, polyak, flags,
                                 partials, norm_out)))
        return 1;
    if (tensors == 0) return 0;
    const mms::ParamArgs a = build_param_args(tensors, numel, param, grad, exp_avg, exp_avg_sq, target, lr, beta1, beta2, eps, weight_decay, step, max_norm,
                                              polyak, partials, norm_out);
    const int norm_chunks = a.norm_first[mms::kParamMaxTensors], step_chunks = a.step_first[mms::kParamMaxTensors];
    float coef = 1.f;
    if (a.use_norm) {
#pragma omp parallel for schedule(static)
        for (int k = 0; k < norm_chunks; k++) {
            const int t = mms::param_chunk_tensor(a, false, k);
            const int64_t lo = (int64_t)(k - a.norm_first[t]) * mms::kParamChunk, hi = std::min(a.numel[t], lo + mms::kParamChunk);
            double s = 0.0;
            for (int64_t e = lo; e < hi; e++) s += (double)a.g[t][e] * (double)a.g[t][e];
            partials[k] = s;
        }
        double sum = 0.0;
        for (int k = 0; k < norm_chunks; k++) sum += partials[k];
        const float total = (float)sqrt(sum);
        coef = mms::param_clip_coef(total, a.max_norm);
        if (norm_out) *norm_out = total;
    }
#pragma omp parallel for schedule(static)
    for (int k = 0; k < step_chunks; k++) {
        const int t = mms::param_chunk_tensor(a, true, k);
        const int64_t lo = (int64_t)(k - a.step_first[t]) * mms::kParamChunk, hi = std::min(a.numel[t], lo + mms::kParamChunk);
        float *p = a.p[t], *m = a.m[t], *v = a.v[t], *tg = a.t[t];
        const float* g = a.g[t];
        for (int64_t e = lo; e < hi; e++) {
            float P = p[e];
            if (m) {
                mms::param_adam(P, g[e], m[e], v[e], coef, a.c);
                p[e] = P;
            }
            if (tg) tg[e] = mms::param_polyak(tg[e], P, a.c);
        }
    }
    return 0;
}
static float act_fn(float v, int act) {
    if (act == 1) return (v > 0.f) ? v : (expf(v) - 1.f);
    if (act == 2) return fmaxf(v, 0.f);
    if (act == 3) return tanhf(v);
    return v;
}
MMS_API int mms_linear2_act(int device, int64_t M, int32_t N, int32_t K, const float* x0, const float* w0, const float* b0, float* y0,
                            const float* x1, const float* w1, const float* b1, float* y1, int32_t act, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_linear2_act(M, N, K, x0, w0, b0, y0, x1, w1, b1, y1, act))) return 1;
    const bool two = x1 != nullptr;
    const float* xs[2] = {x0, x1};
    const float* ws[2] = {w0, w1};
    const float* bs[2] = {b0, b1};
    float* ys[2] = {y0, y1};
    for (int g = 0; g < (two ? 2 : 1); g++) {
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++)
            for (int n = 0; n < N; n++) {
                float s = 0.f;
                for (int k = 0; k < K; k++) s = fmaf(xs[g][m * K + k], ws[g][(int64_t)n * K + k], s);    // (the fp32 MFMA is an fmaf chain too)
                ys[g][m * N + n] = act_fn(s + bs[g][n], act);
            }
    }
    return 0;
}

// ---- split-operand layers (csrc/split_kernels.hip): fp32 carried as three bf16 planes, format P32 = bf16 [rows, KC, 3, 32] ------------
// On the host the planes are summed back (a0 + a1 + a2 IS the fp32 number) and the product is the same fmaf chain as mms_linear2_act.
static inline uint16_t f2bf(float f) {                                    // round to nearest even, as v_cvt_pk_bf16_f32
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static inline float bf2f(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static inline void split3(float v, uint16_t* p0, uint16_t* p1, uint16_t* p2) {
    *p0 = f2bf(v); v -= bf2f(*p0);
    *p1 = f2bf(v); v -= bf2f(*p1);
    *p2 = f2bf(v);
}
static inline float join3(const uint16_t* chunk, int j) { return (bf2f(chunk[j]) + bf2f(chunk[32 + j])) + bf2f(chunk[64 + j]); }

static void split_planes_rows(int64_t rows, int32_t K, int32_t x_pitch, const float* x, void* planes) {
    const int KC = (K + 31) / 32;
    uint16_t* out = (uint16_t*)planes;
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < rows; r++)
        for (int kc = 0; kc < KC; kc++) {
            uint16_t* c = out + (r * KC + kc) * 96;
            for (int j = 0; j < 32; j++) {
                const int k = kc * 32 + j;
                split3(k < K ? x[r * x_pitch + k] : 0.f, c + j, c + 32 + j, c + 64 + j);
            }
        }
}

MMS_API int mms_split_planes(int device, int64_t rows, int32_t K, int32_t x_pitch, const float* x, void* planes, void*) {
    if (cpu_only(device)) return 1;
    if (x_pitch == 0) x_pitch = K;
    if (refused(check_split_planes(rows, K, x_pitch, x, planes))) return 1;
    split_planes_rows(rows, K, x_pitch, x, planes);
    return 0;
}

MMS_API int mms_split_planes_group(int device, int32_t groups, int64_t rows, int32_t K, int32_t x_pitch, const float* const* x, void* const* planes, void*) {
    if (cpu_only(device)) return 1;
    if (x_pitch == 0) x_pitch = K;
    if (refused(check_split_planes_group(groups, rows, K, x_pitch, x, planes))) return 1;
    for (int g = 0; g < groups; g++) split_planes_rows(rows, K, x_pitch, x[g], planes[g]);
    return 0;
}

// The layer on decoded operands, shared by the two plane formats: `wf` [N][KC * 32] and `decode_x(m, xr)` give the operands as the
// floats the planes stand for (times their row scales in the H32 format, undone by `rescale(m, n)` = 1 for P32), `encode_y(m, row)`
// stores the finished row (out_mode 0 / 1).
template <class DecodeX, class Rescale, class EncodeY>
static void split_layer_rows(int64_t M, int32_t N, int KC, const std::vector<float>& wf, const float* b, int32_t act, int32_t out_mode, const float* ln_s,
                             const float* ln_stat_in, float* ln_part_out, const float* head_w, float* head_part, int32_t head_dim, DecodeX decode_x,
                             Rescale rescale, EncodeY encode_y) {
    const int slots = N / 64;
    const bool ln = ln_s != nullptr;
#pragma omp parallel for schedule(static)
    for (int64_t m = 0; m < M; m++) {
        std::vector<float> xr((size_t)KC * 32), row((size_t)N);
        decode_x(m, xr.data());
        for (int n = 0; n < N; n++) {
            float s = 0.f;
            const float* wr = wf.data() + (size_t)n * KC * 32;
            for (int k = 0; k < KC * 32; k++) s = fmaf(xr[k], wr[k], s);
            s *= rescale(m, n);
            if (ln) s = ln_stat_in[2 * m + 1] * (s - ln_stat_in[2 * m] * ln_s[n]);
            row[n] = act_fn(s + b[n], act);
        }
        if (ln)
            for (int sl = 0; sl < slots; sl++) {                                    // (sum, M2 about the slot mean) per 64 columns
                float sum = 0.f, m2 = 0.f;
                for (int n = 64 * sl; n < 64 * sl + 64; n++) sum += row[n];
                const float mean = sum * (1.f / 64.f);
                for (int n = 64 * sl; n < 64 * sl + 64; n++) m2 += (row[n] - mean) * (row[n] - mean);
                ln_part_out[((size_t)sl * M + m) * 2 + 0] = sum;
                ln_part_out[((size_t)sl * M + m) * 2 + 1] = m2;
            }
        if (out_mode == 2) {
            for (int sl = 0; sl < slots; sl++)
                for (int j = 0; j < head_dim; j++) {
                    float p = 0.f;
                    for (int n = 64 * sl; n < 64 * sl + 64; n++) p += row[n] * head_w[(size_t)j * N + n];
                    head_part[((size_t)sl * M + m) * ((head_dim + 3) & ~3) + j] = p;
                }
        } else {
            encode_y(m, row.data());
        }
    }
}

MMS_API int mms_linear_group_act_split(int device, int32_t groups, int64_t M, int32_t N, int32_t K, const void* const* x, const void* const* w,
                                       const float* const* b, void* const* y, int32_t act, int32_t out_mode, const float* const* ln_s,
                                       const float* const* ln_stat_in, float* const* ln_part_out, const float* const* head_w, float* const* head_part,
                                       const int32_t* head_dims, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_split_layer(false, groups, M, N, K, x, w, b, y, nullptr, nullptr, nullptr, act, out_mode, ln_s, ln_stat_in, ln_part_out, head_w, head_part, head_dims))) return 1;
    const bool ln = ln_s != nullptr;
    const int KC = (K + 31) / 32, NC = N / 32;
    for (int g = 0; g < groups; g++) {
        const uint16_t* xp = (const uint16_t*)x[g];
        const uint16_t* wp = (const uint16_t*)w[g];
        std::vector<float> wf((size_t)N * KC * 32);
        for (int64_t n = 0; n < N; n++)
            for (int k = 0; k < KC * 32; k++) wf[n * KC * 32 + k] = join3(wp + (n * KC + k / 32) * 96, k % 32);
        void* yg = out_mode != 2 ? y[g] : nullptr;
        split_layer_rows(M, N, KC, wf, b[g], act, out_mode, ln ? ln_s[g] : nullptr, ln ? ln_stat_in[g] : nullptr, ln ? ln_part_out[g] : nullptr,
                         out_mode == 2 ? head_w[g] : nullptr, out_mode == 2 ? head_part[g] : nullptr, out_mode == 2 ? head_dims[g] : 0,
                         [&](int64_t m, float* xr) { for (int k = 0; k < KC * 32; k++) xr[k] = join3(xp + (m * KC + k / 32) * 96, k % 32); },
                         [](int64_t, int) { return 1.f; },
                         [&](int64_t m, const float* row) {
                             if (out_mode == 1) {
                                 for (int n = 0; n < N; n++) {
                                     uint16_t* c = (uint16_t*)yg + (m * NC + n / 32) * 96 + n % 32;
                                     split3(row[n], c, c + 32, c + 64);
                                 }
                             } else {
                                 memcpy((float*)yg + m * N, row, (size_t)N * 4);
                             }
                         });
    }
    return 0;
}

// ---- the same with two scaled fp16 planes per operand (csrc/split16_kernels.hip), format H32 = f16 [rows, KC, 2, 32] -------------------
// The format and its bound rules: planes16_lane.h; one element in and out: planes16_put / planes16_get (lane_step.h).
using mms::chain_scales;
using mms::planes16_elem;
using mms::planes16_get;
using mms::planes16_put;
using mms::pow2_scale;

// One row -> its planes (planes may be NULL) and its power-of-two scale: the largest magnitude, then 32 k at a time under that scale,
// the tail zero.  at(k) = element k of the row, k < K; the same value at every call.  Returns the largest magnitude.
template <class At>
static float split_row16(uint16_t* planes, int64_t r, int K, At at, float& sc, float& iv) {
    const int KC = (K + 31) / 32;
    float big = 0.f;
    for (int k = 0; k < K; k++) big = fmaxf(big, fabsf(at(k)));
    pow2_scale(big, sc, iv);
    for (int k = 0; k < KC * 32 && planes; k++) planes16_put(planes16_elem(planes, r, KC, k), k < K ? at(k) * sc : 0.f);
    return big;
}
// ... and the scales of the layers behind row r, from its bound
static void chain_rows16(int32_t nchains, int32_t L, const float* chain, float bound, float* chain_scale, float* chain_inv, int64_t rows, int64_t r) {
    for (int c = 0; c < nchains; c++) chain_scales(chain + (size_t)c * L * 2, c, L, bound, chain_scale, chain_inv, rows, r);
}

static void split_planes16_rows(int32_t groups, int64_t rows, int32_t K, int32_t x_pitch, const float* const* x, void* const* planes, float* const* scale,
                                float* const* inv, int32_t nchains, int32_t L, const float* const* chain, float* const* chain_scale,
                                float* const* chain_inv, float* const* stat, float eps) {
    for (int g = 0; g < groups; g++) {
        const float* xg = x[g];
#pragma omp parallel for schedule(static)
        for (int64_t r = 0; r < rows; r++) {
            float sc, iv;
            const float big = split_row16((uint16_t*)planes[g], r, K, [&](int k) { return xg[r * x_pitch + k]; }, sc, iv);
            if (scale[g]) scale[g][r] = sc;
            if (inv[g]) inv[g][r] = iv;
            if (stat) {                                                   // two-pass LayerNorm statistics of the row
                float sum = 0.f, m2 = 0.f;
                for (int k = 0; k < K; k++) sum += xg[r * x_pitch + k];
                const float mean = sum / (float)K;
                for (int k = 0; k < K; k++) m2 += (xg[r * x_pitch + k] - mean) * (xg[r * x_pitch + k] - mean);
                stat[g][2 * r] = mean;
                stat[g][2 * r + 1] = 1.0f / sqrtf(m2 / (float)K + eps);
            }
            if (nchains > 0) chain_rows16(nchains, L, chain[g], big, chain_scale[g], chain_inv[g], rows, r);
        }
    }
}

MMS_API int mms_split_planes16_group(int device, int32_t groups, int64_t rows, int32_t K, int32_t x_pitch, const float* const* x, void* const* planes,
                                     float* const* scale, float* const* inv, int32_t nchains, int32_t L, const float* const* chain,
                                     float* const* chain_scale, float* const* chain_inv, float* const* stat, float eps, void*) {
    if (cpu_only(device)) return 1;
    if (x_pitch == 0) x_pitch = K;
    if (refused(check_split_planes16_group(groups, rows, K, x_pitch, x, planes, scale, inv, nchains, L, chain, chain_scale, chain_inv, stat))) return 1;
    split_planes16_rows(groups, rows, K, x_pitch, x, planes, scale, inv, nchains, L, chain, chain_scale, chain_inv, stat, eps);
    return 0;
}

// The same for rows that are the concatenation of two sources (include/mms.h): element k of a row is read from x0 (k < K0) or x1 --
// operation by operation what split_planes16_rows does on the materialised concatenation, hence the same bits.
MMS_API int mms_split_planes16_cat(int device, int64_t rows, int32_t K0, int32_t pitch0, const float* x0, int32_t K1, int32_t pitch1, const float* x1,
                                   void* planes, float* scale, float* inv, int32_t nchains, int32_t L, const float* chain, float* chain_scale,
                                   float* chain_inv, void*) {
    if (cpu_only(device)) return 1;
    if (pitch0 == 0) pitch0 = K0;
    if (pitch1 == 0) pitch1 = K1;
    if (refused(check_split_planes16_cat(rows, K0, pitch0, x0, K1, pitch1, x1, planes, nchains, L, chain, chain_scale, chain_inv))) return 1;
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < rows; r++) {
        float sc, iv;
        const float big = split_row16((uint16_t*)planes, r, K0 + K1, [&](int k) { return k < K0 ? x0[r * pitch0 + k] : x1[r * pitch1 + (k - K0)]; }, sc, iv);
        if (scale) scale[r] = sc;
        if (inv) inv[r] = iv;
        chain_rows16(nchains, L, chain, big, chain_scale, chain_inv, rows, r);
    }
    return 0;
}

// The device-side refresh of the weights' planes and of the bound chain (include/mms.h).  l1 follows the kernel's summation order
// (split16_planes_kernel: P lanes per row walk the row's 8-element pieces p = lane, lane + P, ...; xor butterfly over the lanes), so
// that the bound -- and with it every hidden activation's power-of-two scale -- is the same number on both builds.
MMS_API int mms_weight_planes16_group(int device, int32_t groups, const int64_t* N, const int32_t* K, const float* const* w, void* const* planes,
                                      float* const* scale, float* const* inv, float* const* l1, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_weight_planes16_group(groups, N, K, w, planes, scale, inv))) return 1;
    for (int g = 0; g < groups; g++) {
        if (N[g] == 0) continue;
        split_planes16_rows(1, N[g], K[g], K[g], w + g, planes + g, scale + g, inv + g, 0, 0, nullptr, nullptr, nullptr, nullptr, 0.f);
        if (!l1 || !l1[g]) continue;
        const int Kg = K[g], KC = (Kg + 31) / 32, pieces = KC * 4;
        int P = 1;
        while (P < pieces && P < 64) P <<= 1;
#pragma omp parallel for schedule(static)
        for (int64_t r = 0; r < N[g]; r++) {
            float lane[64];
            for (int sub = 0; sub < P; sub++) {
                float a = 0.f;
                for (int p = sub; p < pieces; p += P)
                    for (int j = 0; j < 8; j++) { const int k = p * 8 + j; a += (k < Kg) ? fabsf(w[g][r * Kg + k]) : 0.f; }
                lane[sub] = a;
            }
            for (int m = P >> 1; m >= 1; m >>= 1) {
                float nxt[64];
                for (int i = 0; i < P; i++) nxt[i] = lane[i] + lane[i ^ m];
                for (int i = 0; i < P; i++) lane[i] = nxt[i];
            }
            l1[g][r] = lane[0];
        }
    }
    return 0;
}

MMS_API int mms_chain_refresh16(int device, int32_t nchains, int32_t L, const float* const* l1, const float* const* bias, const int32_t* n, float* chain,
                                float bound0, int64_t rows, float* chain_scale, float* chain_inv, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_chain_refresh16(nchains, L, l1, n, chain, bound0, rows, chain_scale, chain_inv))) return 1;
    for (int e = 0; e < nchains * L; e++) {
        float m = 0.f, b = 0.f;
        for (int i = 0; i < n[e]; i++) {
            m = fmaxf(m, l1[e][i]);
            if (bias && bias[e]) b = fmaxf(b, fabsf(bias[e][i]));
        }
        chain[2 * e] = m;
        chain[2 * e + 1] = b;
    }
    for (int64_t r = 0; r < rows; r++) chain_rows16(nchains, L, chain, bound0, chain_scale, chain_inv, rows, r);
    return 0;
}

// The folded-LayerNorm layers' weight side (csrc/fold16_kernels.hip; include/mms.h)
MMS_API int mms_fold_planes16_group(int device, int32_t groups, const int64_t* N, const int32_t* K, const float* const* w, const float* const* gamma,
                                    const float* const* beta, const float* const* bias, void* const* planes, float* const* inv, float* const* s_out,
                                    float* const* c_out, float* const* rb, float* const* wt, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_fold_planes16_group(groups, N, K, w, planes, inv))) return 1;
    for (int g = 0; g < groups; g++) {
        const int Kg = K[g];
        const float* gm = gamma ? gamma[g] : nullptr;
        const float* bt = beta ? beta[g] : nullptr;
        uint16_t* out = planes ? (uint16_t*)planes[g] : nullptr;
#pragma omp parallel for schedule(static)
        for (int64_t r = 0; r < N[g]; r++) {
            const float* wr = w[g] + r * Kg;
            const auto wt_at = [&](int k) { return gm ? wr[k] * gm[k] : wr[k]; };            // W~[r, k]
            float s = 0.f, c = 0.f, l2 = 0.f;
            for (int k = 0; k < Kg; k++) {
                const float v = wt_at(k);
                s += v;
                l2 += v * v;
                if (bt) c += wr[k] * bt[k];
            }
            if (bias && bias[g]) c += bias[g][r];
            float sc, iv;
            split_row16(out, r, Kg, wt_at, sc, iv);
            if (wt && wt[g])
                for (int k = 0; k < Kg; k++) wt[g][r * Kg + k] = wt_at(k);
            if (inv && inv[g]) inv[g][r] = iv;
            if (s_out && s_out[g]) s_out[g][r] = s;
            if (c_out && c_out[g]) c_out[g][r] = c;
            if (rb && rb[g]) rb[g][r] = mms::fold_row_bound(l2, Kg, c);
        }
    }
    return 0;
}

MMS_API int mms_fold_scales16_group(int device, int32_t groups, const float* const* rb, const int32_t* n, int64_t M, float* const* scale1,
                                    float* const* ysc, float* const* yinv, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_fold_scales16_group(groups, rb, n, M))) return 1;
    for (int g = 0; g < groups; g++) {
        float m = 0.f;
        for (int i = 0; i < n[g]; i++) m = fmaxf(m, rb[g][i]);
        float sc, iv;
        pow2_scale(mms::fold_net_bound(m), sc, iv);
        if (scale1 && scale1[g]) scale1[g][0] = sc;
        for (int64_t r = 0; r < M; r++) {
            if (ysc && ysc[g]) ysc[g][r] = sc;
            if (yinv && yinv[g]) yinv[g][r] = iv;
        }
    }
    return 0;
}

MMS_API int mms_linear_group_act_split16(int device, int32_t groups, int64_t M, int32_t N, int32_t K, const void* const* x, const void* const* w,
                                         const float* const* b, void* const* y, const float* const* x_inv, const float* const* w_inv,
                                         const float* const* y_scale, int32_t act, int32_t out_mode, const float* const* ln_s,
                                         const float* const* ln_stat_in, float* const* ln_part_out, const float* const* head_w, float* const* head_part,
                                         const int32_t* head_dims, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_split_layer(true, groups, M, N, K, x, w, b, y, x_inv, w_inv, y_scale, act, out_mode, ln_s, ln_stat_in, ln_part_out, head_w, head_part, head_dims))) return 1;
    const bool ln = ln_s != nullptr;
    const int KC = (K + 31) / 32, NC = N / 32;
    for (int g = 0; g < groups; g++) {
        const uint16_t* xp = (const uint16_t*)x[g];
        const uint16_t* wp = (const uint16_t*)w[g];
        std::vector<float> wf((size_t)N * KC * 32);
        for (int64_t n = 0; n < N; n++)
            for (int k = 0; k < KC * 32; k++) wf[n * KC * 32 + k] = planes16_get(planes16_elem(wp, n, KC, k));
        void* yg = out_mode != 2 ? y[g] : nullptr;
        const float* xi = x_inv[g];
        const float* wi = w_inv[g];
        const float* ys = out_mode == 1 ? y_scale[g] : nullptr;
        split_layer_rows(M, N, KC, wf, b[g], act, out_mode, ln ? ln_s[g] : nullptr, ln ? ln_stat_in[g] : nullptr, ln ? ln_part_out[g] : nullptr,
                         out_mode == 2 ? head_w[g] : nullptr, out_mode == 2 ? head_part[g] : nullptr, out_mode == 2 ? head_dims[g] : 0,
                         [&](int64_t m, float* xr) { for (int k = 0; k < KC * 32; k++) xr[k] = planes16_get(planes16_elem(xp, m, KC, k)); },
                         [&](int64_t m, int n) { return wi[n] * xi[m]; },
                         [&](int64_t m, const float* row) {
                             if (out_mode == 1) {
                                 for (int n = 0; n < N; n++) planes16_put(planes16_elem((uint16_t*)yg, m, NC, n), row[n] * ys[m]);
                             } else {
                                 memcpy((float*)yg + m * N, row, (size_t)N * 4);
                             }
                         });
    }
    return 0;
}

// log(std) + 0.5 log(2 pi) in double, rounded once (policy_kernels.hip: log_density_const); logp = fma(-z / 2, z, -this)
static inline float log_density_const(float sd) { return (float)(log((double)sd) + 0.9189385332046727); }

static void chan_combine(const float* part, int64_t M, int64_t row, int slots, float& mean, float& m2) {
    float sum = 0.f;
    for (int k = 0; k < slots; k++) sum += part[((size_t)k * M + row) * 2];
    mean = sum / (64.f * (float)slots);
    m2 = 0.f;
    for (int k = 0; k < slots; k++) {
        const float d = part[((size_t)k * M + row) * 2] * (1.f / 64.f) - mean;
        m2 += part[((size_t)k * M + row) * 2 + 1] + 64.f * d * d;
    }
}

MMS_API int mms_row_stats_chan_group(int device, int32_t groups, int64_t M, int32_t slots, const float* const* part, float* const* stat, float eps, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_row_stats_chan_group(groups, M, slots, part, stat))) return 1;
    for (int g = 0; g < groups; g++) {
        for (int64_t r = 0; r < M; r++) {
            float mean, m2;
            chan_combine(part[g], M, r, slots, mean, m2);
            stat[g][2 * r] = mean;
            stat[g][2 * r + 1] = 1.0f / sqrtf(m2 / (64.f * (float)slots) + eps);
        }
    }
    return 0;
}

MMS_API int mms_marl_heads_finish(int device, int32_t groups, int64_t M, int32_t slots, const float* const* part, const float* const* head_part,
                                  const float* const* hs, const float* const* hc, const int32_t* A, const float* const* std, float* const* out,
                                  float* const* logp, const int32_t* out_pitch, int64_t* const* counters, uint64_t seed, int64_t row_offset, float eps, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_marl_heads_finish(groups, M, slots, part, head_part, hs, hc, A, out, out_pitch))) return 1;
    for (int g = 0; g < groups; g++) {
        const int pitch = out_pitch ? out_pitch[g] : A[g];
        const float* sd = std ? std[g] : nullptr;
        int64_t* cnt = (sd && counters) ? counters[g] : nullptr;
        for (int64_t r = 0; r < M; r++) {
            float mean, m2;
            chan_combine(part[g], M, r, slots, mean, m2);
            const float rstd = 1.0f / sqrtf(m2 / (64.f * (float)slots) + eps);
            const int64_t c = cnt ? cnt[r] : 0;
            for (int j = 0; j < A[g]; j++) {
                float dot = 0.f;
                for (int k = 0; k < slots; k++) dot += head_part[g][((size_t)k * M + r) * ((A[g] + 3) & ~3) + j];
                const float mu = rstd * (dot - mean * hs[g][j]) + hc[g][j];
                if (!sd) { out[g][r * pitch + j] = mu; continue; }
                const float z = mms::rand_normal(seed + (uint64_t)g, (uint64_t)(row_offset + r), (uint64_t)c, (uint32_t)j);
                out[g][r * pitch + j] = mu + sd[j] * z;
                if (logp && logp[g]) logp[g][r * pitch + j] = fmaf(-0.5f * z, z, -log_density_const(sd[j]));
            }
            if (cnt) cnt[r] = c + 1;
        }
    }
    return 0;
}

// ---- grouped policy inference (plain loops) -------------------------------------------------------------------------------------
// A dot product in one fixed order: sixteen fp32 partial sums over k % 16, each step p <- fl(p + a b) with the product exact (formed
// and added in double, rounded to fp32: the fused multiply-add's arithmetic without depending on the host's ISA), a remainder of
// n % 16 terms into the first ones, then the halving tree p[j] += p[j + 8], + 4, + 2, + 1.  An output sees n / 16 + 4 roundings of
// partial sums instead of the n of a single chain: the error of a blocked fp32 product, which is what the library products that the
// tests take as their yardstick have (a recurrent policy's state carries a layer's error from step to step).
static inline float dot16(const float* a, const float* b, int n) {
    float p[16] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 16 <= n; k += 16)
        for (int j = 0; j < 16; j++) p[j] = (float)((double)p[j] + (double)a[k + j] * (double)b[k + j]);
    for (int j = 0; k + j < n; j++) p[j] = (float)((double)p[j] + (double)a[k + j] * (double)b[k + j]);
    for (int w = 8; w >= 1; w >>= 1)
        for (int j = 0; j < w; j++) p[j] += p[j + w];
    return p[0];
}
MMS_API int mms_linear_group_act(int device, int32_t groups, int64_t M, int32_t N, int32_t K, const float* const* x, const float* const* w,
                                 const float* const* b, float* const* y, int32_t act, const float* const* ln_s, const float* const* ln_stat_in,
                                 float* const* ln_part_out, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_linear_group_act(groups, M, N, K, x, w, b, y, act, ln_s, ln_stat_in, ln_part_out))) return 1;
    for (int g = 0; g < groups; g++) {
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++) {
            for (int n = 0; n < N; n++) {
                float s = dot16(x[g] + m * K, w[g] + (int64_t)n * K, K);
                if (ln_s) s = ln_stat_in[g][2 * m + 1] * (s - ln_stat_in[g][2 * m] * ln_s[g][n]);      // rstd (W~ h - mean s)
                y[g][m * N + n] = act_fn(s + b[g][n], act & 15);
            }
            if (ln_part_out)                                                                            // slot = 64 consecutive columns
                for (int slot = 0; slot < N / 64; slot++) {
                    float ps = 0.f, pq = 0.f;
                    for (int n = 64 * slot; n < 64 * slot + 64; n++) { const float v = y[g][m * N + n]; ps += v; pq += v * v; }
                    ln_part_out[g][((int64_t)slot * M + m) * 2] = ps;
                    ln_part_out[g][((int64_t)slot * M + m) * 2 + 1] = pq;
                }
        }
    }
    return 0;
}
MMS_API int mms_row_stats_group(int device, int32_t groups, int64_t M, int32_t slots, int32_t width, const float* const* part, float* const* stat,
                                float eps, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_row_stats_group(groups, M, slots, width, part, stat))) return 1;
    for (int g = 0; g < groups; g++) {
        for (int64_t m = 0; m < M; m++) {
            float sum = 0.f, sq = 0.f;
            for (int k = 0; k < slots; k++) { sum += part[g][((int64_t)k * M + m) * 2]; sq += part[g][((int64_t)k * M + m) * 2 + 1]; }
            const float mean = sum / (float)width;
            const float var = fmaxf(sq / (float)width - mean * mean, 0.f);
            stat[g][2 * m] = mean;
            stat[g][2 * m + 1] = 1.0f / sqrtf(var + eps);
        }
    }
    return 0;
}
static void ln_row(const float* x, int K, float eps, float& mean, float& rstd) {
    float s = 0.f;
    for (int k = 0; k < K; k++) s += x[k];
    mean = s / (float)K;
    float q = 0.f;
    for (int k = 0; k < K; k++) q += (x[k] - mean) * (x[k] - mean);
    rstd = 1.0f / sqrtf(q / (float)K + eps);
}
MMS_API int mms_row_moments_group(int device, int32_t groups, int64_t M, int32_t K, int32_t x_pitch, const float* const* x, float* const* stat,
                                  float eps, void*) {
    if (cpu_only(device)) return 1;
    if (x_pitch == 0) x_pitch = K;
    if (refused(check_row_moments_group(groups, M, K, x_pitch, x, stat))) return 1;
    for (int g = 0; g < groups; g++) {
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++) ln_row(x[g] + m * x_pitch, K, eps, stat[g][2 * m], stat[g][2 * m + 1]);
    }
    return 0;
}
MMS_API int mms_layernorm_group(int device, int32_t groups, int64_t M, int32_t K, int32_t Kp, int32_t x_pitch, const float* const* x,
                                const float* const* gamma, const float* const* beta, float* const* y, float eps, void*) {
    if (cpu_only(device)) return 1;
    if (x_pitch == 0) x_pitch = K;
    if (refused(check_layernorm_group(groups, M, K, Kp, x_pitch, x, gamma, beta, y))) return 1;
    for (int g = 0; g < groups; g++) {
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++) {
            float mean, rstd;
            ln_row(x[g] + m * x_pitch, K, eps, mean, rstd);
            for (int k = 0; k < K; k++) y[g][m * Kp + k] = (x[g][m * x_pitch + k] - mean) * rstd * gamma[g][k] + beta[g][k];
            for (int k = K; k < Kp; k++) y[g][m * Kp + k] = 0.f;
        }
    }
    return 0;
}
// One GRU cell step per network (include/mms.h: mms_gru_group) over ../gru_lane.h, every dot product by dot16 (above).
MMS_API int mms_gru_group(int device, int32_t groups, int64_t M, int32_t K, int32_t H, const float* const* x, int64_t x_pitch, const float* const* h,
                          int64_t h_pitch, const float* const* mask, int64_t mask_pitch, const float* const* w_ih, const float* const* w_hh,
                          const float* const* b_ih, const float* const* b_hh, float* const* h_out, int64_t h_out_pitch, float* const* y, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_gru_group(groups, M, K, H, x, x_pitch, h, h_pitch, mask, mask_pitch, w_ih, w_hh, b_ih, b_hh, h_out, h_out_pitch, y))) return 1;
    for (int g = 0; g < groups; g++) {
        const float *wi = w_ih[g], *wh = w_hh[g], *bi = b_ih[g], *bh = b_hh[g];
        float* yg = y ? y[g] : nullptr;
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++) {
            float hm[mms::kGruMaxH];
            const float* xr = x[g] + m * x_pitch;
            const float* hr = h[g] + m * h_pitch;
            if (mask) {
                const float mk = mask[g][m * mask_pitch];
                for (int k = 0; k < H; k++) hm[k] = mms::gru_masked(mk, hr[k]);
            } else {
                for (int k = 0; k < H; k++) hm[k] = hr[k];
            }
            for (int j = 0; j < H; j++) {
                const float s_r = dot16(xr, wi + (int64_t)j * K, K) + dot16(hm, wh + (int64_t)j * H, H);
                const float s_z = dot16(xr, wi + (int64_t)(H + j) * K, K) + dot16(hm, wh + (int64_t)(H + j) * H, H);
                const float s_ni = dot16(xr, wi + (int64_t)(2 * H + j) * K, K);
                const float s_nh = dot16(hm, wh + (int64_t)(2 * H + j) * H, H);
                const float o = mms::gru_cell(s_r, s_z, s_ni, s_nh, bi[j], bi[H + j], bi[2 * H + j], bh[j], bh[H + j], bh[2 * H + j], hm[j]);
                h_out[g][m * h_out_pitch + j] = o;
                if (yg) yg[m * H + j] = o;
            }
        }
    }
    return 0;
}
// The gate arithmetic alone on given pre-activations (include/mms.h: mms_gru_gates_group): ../gru_lane.h's gru_gates per element.
MMS_API int mms_gru_gates_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* gi, const float* const* gh, int64_t g_pitch,
                                const float* const* h, int64_t h_pitch, const float* const* mask, int64_t mask_pitch, const float* const* b_hh,
                                float* const* h_out, int64_t h_out_pitch, float* const* y, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_gru_gates_group(groups, M, H, gi, gh, g_pitch, h, h_pitch, mask, mask_pitch, b_hh, h_out, h_out_pitch, y))) return 1;
    for (int g = 0; g < groups; g++) {
        const float* bh = b_hh[g];
        float* yg = y ? y[g] : nullptr;
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++) {
            const float *ir = gi[g] + m * g_pitch, *hr = gh[g] + m * g_pitch, *hs = h[g] + m * h_pitch;
            const float mk = mask ? mask[g][m * mask_pitch] : 1.f;
            for (int j = 0; j < H; j++) {
                const float o = mms::gru_gates(mask != nullptr, mk, ir[j], ir[H + j], ir[2 * H + j], hr[j], hr[H + j], hr[2 * H + j], bh[j], bh[H + j], bh[2 * H + j], hs[j]);
                h_out[g][m * h_out_pitch + j] = o;
                if (yg) yg[m * H + j] = o;
            }
        }
    }
    return 0;
}
// The backward of that gate step (include/mms.h: mms_gru_gates_grad_group) over ../gru_grad_lane.h.  The rows in the chunks of
// gru_grad_chunk_rows(M, H) (OpenMP over chunks): a chunk's column sums in double over ascending rows, the chunks added in ascending
// order and rounded once -- the result does not depend on the number of threads or on `groups`.  No workspace.
MMS_API int mms_gru_gates_grad_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* gi, const float* const* gh, int64_t g_pitch,
                                     const float* const* h, int64_t h_pitch, const float* const* mask, int64_t mask_pitch, const float* const* b_hh,
                                     const float* const* dh_out, int64_t dh_out_pitch, const float* const* dy, int64_t dy_pitch, float* const* dgi,
                                     float* const* dgh, int64_t dg_pitch, float* const* dh, int64_t dh_pitch, float* const* dbias, void* workspace,
                                     int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_gru_gates_grad_group(groups, M, H, gi, gh, g_pitch, h, h_pitch, mask, mask_pitch, b_hh, dh_out, dh_out_pitch, dy, dy_pitch, dgi, dgh,
                                           dg_pitch, dh, dh_pitch, dbias, workspace, ws_bytes, 0)))
        return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }                  // the size query
    if (M == 0) return 0;
    const int64_t chunk = mms::gru_grad_chunk_rows(M, H), nchunks = mms::gru_grad_chunks(M, H);
    const int C = 4 * H;
    for (int g = 0; g < groups; g++) {
        const float* bh = b_hh[g];
        const float* dyg = dy ? dy[g] : nullptr;
        float* db = dbias ? dbias[g] : nullptr;
        std::vector<double> part(db ? (size_t)nchunks * C : 0, 0.0);
#pragma omp parallel for schedule(static)
        for (int64_t c = 0; c < nchunks; c++) {
            double* p = db ? part.data() + c * C : nullptr;
            const int64_t end = (c + 1) * chunk < M ? (c + 1) * chunk : M;
            for (int64_t m = c * chunk; m < end; m++) {
                const float *ir = gi[g] + m * g_pitch, *hr = gh[g] + m * g_pitch, *hs = h[g] + m * h_pitch, *go = dh_out[g] + m * dh_out_pitch;
                const float* gy = dyg ? dyg + m * dy_pitch : nullptr;
                float *di = dgi[g] + m * dg_pitch, *dg = dgh[g] + m * dg_pitch, *dhr = dh[g] + m * dh_pitch;
                const float mk = mask ? mask[g][m * mask_pitch] : 1.f;
                for (int j = 0; j < H; j++) {
                    const float G = gy ? go[j] + gy[j] : go[j];
                    const mms::GruGateGrad o = mms::gru_gates_grad(mask != nullptr, mk, ir[j], ir[H + j], ir[2 * H + j], hr[j], hr[H + j], hr[2 * H + j], bh[j],
                                                                   bh[H + j], bh[2 * H + j], hs[j], G);
                    di[j] = o.dpr; di[H + j] = o.dpz; di[2 * H + j] = o.dpn;
                    dg[j] = o.dgh_r; dg[H + j] = o.dgh_z; dg[2 * H + j] = o.dgh_n;
                    dhr[j] = o.dh;
                    if (p) { p[j] += (double)o.dpr; p[H + j] += (double)o.dpz; p[2 * H + j] += (double)o.dpn; p[3 * H + j] += (double)o.rdpn; }
                }
            }
        }
        if (db)
            for (int q = 0; q < C; q++) {
                double s = 0.0;
                for (int64_t c = 0; c < nchunks; c++) s += part[c * C + q];
                db[q] = (float)s;
            }
    }
    return 0;
}
// The ELU + LayerNorm block behind its product (include/mms.h: mms_elu_ln_group) over ../elu_ln_lane.h: per row, the two sums in double
// over ascending columns.
// planes != NULL (mms_elu_ln_planes16_group): each row of y is then split as mms_split_planes16_group splits it (split_row16).
static void elu_ln_rows(int32_t groups, int64_t M, int32_t H, float eps, const float* const* z, int64_t z_pitch, const float* const* bias,
                        const float* const* gamma, const float* const* beta, float* const* y, int64_t y_pitch, float* const* stat, void* const* planes,
                        float* const* scale, float* const* inv) {
    for (int g = 0; g < groups; g++) {
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++) {
            float a[mms::kEluLnMaxH];
            const float* zr = z[g] + m * z_pitch;
            double s = 0.0, v = 0.0;
            for (int j = 0; j < H; j++) { a[j] = mms::elu_ln_act(mms::elu_ln_u(zr[j], bias[g][j])); s += (double)a[j]; }
            const float mean = mms::elu_ln_mean(s, H);
            for (int j = 0; j < H; j++) v += mms::elu_ln_dev2(a[j], mean);
            const float rstd = mms::elu_ln_rstd(v, H, eps);
            float* yr = y[g] + m * y_pitch;
            for (int j = 0; j < H; j++) yr[j] = mms::elu_ln_out(mms::elu_ln_xhat(a[j], mean, rstd), gamma[g][j], beta[g][j]);
            stat[g][2 * m] = mean;
            stat[g][2 * m + 1] = rstd;
            if (!planes) continue;
            float sc, iv;
            split_row16((uint16_t*)planes[g], m, H, [&](int k) { return yr[k]; }, sc, iv);
            if (scale[g]) scale[g][m] = sc;
            if (inv[g]) inv[g][m] = iv;
        }
    }
}
MMS_API int mms_elu_ln_group(int device, int32_t groups, int64_t M, int32_t H, float eps, const float* const* z, int64_t z_pitch, const float* const* bias,
                             const float* const* gamma, const float* const* beta, float* const* y, int64_t y_pitch, float* const* stat, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_elu_ln_group(groups, M, H, eps, z, z_pitch, bias, gamma, beta, y, y_pitch, stat))) return 1;
    elu_ln_rows(groups, M, H, eps, z, z_pitch, bias, gamma, beta, y, y_pitch, stat, nullptr, nullptr, nullptr);
    return 0;
}
MMS_API int mms_elu_ln_planes16_group(int device, int32_t groups, int64_t M, int32_t H, float eps, const float* const* z, int64_t z_pitch,
                                      const float* const* bias, const float* const* gamma, const float* const* beta, float* const* y, int64_t y_pitch,
                                      float* const* stat, void* const* planes, float* const* scale, float* const* inv, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_elu_ln_planes16_group(groups, M, H, eps, z, z_pitch, bias, gamma, beta, y, y_pitch, stat, planes, scale, inv))) return 1;
    elu_ln_rows(groups, M, H, eps, z, z_pitch, bias, gamma, beta, y, y_pitch, stat, planes, scale, inv);
    return 0;
}
// Its backward (include/mms.h: mms_elu_ln_grad_group).  The rows in the chunks of elu_ln_chunk_rows(M, H) (OpenMP over chunks): a
// chunk's column sums in double over ascending rows, the chunks added in ascending order and rounded once -- the result does not depend
// on the number of threads or on `groups`.  No workspace.  M == 0: zeros into dparams.
MMS_API int mms_elu_ln_grad_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* z, int64_t z_pitch, const float* const* bias,
                                  const float* const* gamma, const float* const* stat, const float* const* dy, int64_t dy_pitch, float* const* dz,
                                  int64_t dz_pitch, float* const* dparams, void* workspace, int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_elu_ln_grad_group(groups, M, H, z, z_pitch, bias, gamma, stat, dy, dy_pitch, dz, dz_pitch, dparams, workspace, ws_bytes, 0))) return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }                  // the size query
    const int64_t chunk = mms::elu_ln_chunk_rows(M, H), nchunks = mms::elu_ln_chunks(M, H);
    const int C = 3 * H;
    for (int g = 0; g < groups; g++) {
        float* dp = dparams ? dparams[g] : nullptr;
        std::vector<double> part(dp ? (size_t)nchunks * C : 0, 0.0);
#pragma omp parallel for schedule(static)
        for (int64_t c = 0; c < nchunks; c++) {
            double* p = dp ? part.data() + c * C : nullptr;
            const int64_t end = (c + 1) * chunk < M ? (c + 1) * chunk : M;
            float u[mms::kEluLnMaxH], a[mms::kEluLnMaxH];
            double xh[mms::kEluLnMaxH];
            for (int64_t m = c * chunk; m < end; m++) {
                const float *zr = z[g] + m * z_pitch, *gy = dy[g] + m * dy_pitch;
                const float mean = stat[g][2 * m], rstd = stat[g][2 * m + 1];
                double s1 = 0.0, s2 = 0.0;
                for (int j = 0; j < H; j++) {
                    u[j] = mms::elu_ln_u(zr[j], bias[g][j]);
                    a[j] = mms::elu_ln_act(u[j]);
                    xh[j] = mms::elu_ln_xhat(a[j], mean, rstd);
                    const double q = mms::elu_ln_q(gy[j], gamma[g][j]);
                    s1 += q;
                    s2 += q * xh[j];
                }
                const double c1 = mms::elu_ln_row_mean(s1, H), c2 = mms::elu_ln_row_mean(s2, H);
                float* dr = dz[g] + m * dz_pitch;
                for (int j = 0; j < H; j++) {
                    const float o = mms::elu_ln_dz(u[j], a[j], xh[j], rstd, mms::elu_ln_q(gy[j], gamma[g][j]), c1, c2);
                    dr[j] = o;
                    if (p) { p[j] += (double)o; p[H + j] += (double)gy[j] * xh[j]; p[2 * H + j] += (double)gy[j]; }
                }
            }
        }
        if (dp)
            for (int q = 0; q < C; q++) {
                double s = 0.0;
                for (int64_t c = 0; c < nchunks; c++) s += part[c * C + q];
                dp[q] = (float)s;
            }
    }
    return 0;
}
// The update's output heads (include/mms.h: mms_marl_heads_fwd_group) over ../marl_heads_grad_lane.h: a row's sums over ascending columns
// in double, the bias behind them, one rounding.
MMS_API int mms_marl_heads_fwd_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* f, int64_t f_pitch, const float* const* w,
                                     const float* const* b, const int32_t* A, const float* const* log_std, float x_coef, float y_coef, float* const* out,
                                     float* const* std_out, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_marl_heads_fwd_group(groups, M, H, f, f_pitch, w, b, A, log_std, x_coef, out, std_out))) return 1;
    for (int g = 0; g < groups; g++) {
        const int n = A[g];
        if (log_std && log_std[g])
            for (int j = 0; j < n; j++) std_out[g][j] = mms::heads_std(log_std[g][j], x_coef, y_coef);
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++) {
            const float* fr = f[g] + m * f_pitch;
            for (int j = 0; j < n; j++) {
                const float* wr = w[g] + (int64_t)j * H;
                double s = 0.0;
                for (int k = 0; k < H; k++) s += mms::heads_prod(fr[k], wr[k]);
                out[g][m * n + j] = mms::heads_out(s, b[g][j]);
            }
        }
    }
    return 0;
}
// Their backward (include/mms.h: mms_marl_heads_grad_group).  The rows in the chunks of heads_chunk_rows(M, H) (OpenMP over chunks): a
// chunk's sums over ascending rows in double, the chunks added in ascending order and rounded once -- the result does not depend on the
// number of threads or on `groups`.  No workspace.  M == 0: zeros into dw and db.
MMS_API int mms_marl_heads_grad_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* f, int64_t f_pitch, const float* const* w,
                                      const int32_t* A, const float* const* dout, const float* const* log_std, const float* const* dstd, float x_coef,
                                      float y_coef, float* const* df, int64_t df_pitch, float* const* dw, float* const* db, float* const* dlog_std,
                                      void* workspace, int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_marl_heads_grad_group(groups, M, H, f, f_pitch, w, A, dout, log_std, dstd, x_coef, df, df_pitch, dw, db, dlog_std, workspace, ws_bytes, 0)))
        return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }                  // the size query
    const int64_t chunk = mms::heads_chunk_rows(M, H), nchunks = mms::heads_chunks(M, H);
    for (int g = 0; g < groups; g++) {
        const int n = A[g];
        const int64_t C = mms::heads_part_doubles(n, H);
        float *dfg = df ? df[g] : nullptr, *dwg = dw ? dw[g] : nullptr, *dbg = db ? db[g] : nullptr;
        if (dlog_std && dlog_std[g])
            for (int j = 0; j < n; j++) dlog_std[g][j] = mms::heads_dlog_std(dstd[g][j], log_std[g][j], x_coef, y_coef);
        std::vector<double> part(dwg ? (size_t)(nchunks * C) : 0, 0.0);
#pragma omp parallel for schedule(static)
        for (int64_t c = 0; c < nchunks; c++) {
            double* p = dwg ? part.data() + c * C : nullptr;
            const int64_t end = (c + 1) * chunk < M ? (c + 1) * chunk : M;
            for (int64_t m = c * chunk; m < end; m++) {
                const float *fr = f[g] + m * f_pitch, *d = dout[g] + m * n;
                if (dfg)
                    for (int k = 0; k < H; k++) {
                        double s = 0.0;
                        for (int j = 0; j < n; j++) s += mms::heads_prod(d[j], w[g][(int64_t)j * H + k]);
                        dfg[m * df_pitch + k] = (float)s;
                    }
                if (p)
                    for (int j = 0; j < n; j++) {
                        for (int k = 0; k < H; k++) p[(int64_t)j * H + k] += mms::heads_prod(d[j], fr[k]);
                        p[(int64_t)n * H + j] += (double)d[j];
                    }
            }
        }
        if (dwg)
            for (int64_t q = 0; q < C; q++) {
                double s = 0.0;
                for (int64_t c = 0; c < nchunks; c++) s += part[c * C + q];
                if (q < (int64_t)n * H) dwg[q] = (float)s;
                else dbg[q - (int64_t)n * H] = (float)s;
            }
    }
    return 0;
}
MMS_API int mms_marl_heads_act(int device, int32_t groups, int64_t M, int32_t H, const float* const* h, const float* const* gamma,
                               const float* const* beta, const float* const* w, const float* const* b, const int32_t* A, const float* const* std,
                               float* const* out, float* const* logp, const int32_t* out_pitch, int64_t* const* counters, uint64_t seed,
                               int64_t row_offset, float eps, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_marl_heads_act(groups, M, H, h, gamma, beta, w, b, A, out, out_pitch, eps))) return 1;
    for (int g = 0; g < groups; g++) {
        const int op = out_pitch ? out_pitch[g] : A[g];
        const float* sd = std ? std[g] : nullptr;
        float* lp = logp ? logp[g] : nullptr;
        int64_t* cnt = counters ? counters[g] : nullptr;
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++) {
            float mean, rstd, xh[1024];
            if (eps >= 0.f) {
                ln_row(h[g] + m * H, H, eps, mean, rstd);
                for (int k = 0; k < H; k++) xh[k] = (h[g][m * H + k] - mean) * rstd * gamma[g][k] + beta[g][k];
            } else {
                for (int k = 0; k < H; k++) xh[k] = h[g][m * H + k];
            }
            const int64_t c = cnt ? cnt[m] : 0;
            for (int j = 0; j < A[g]; j++) {
                float p = 0.f;
                for (int k = 0; k < H; k++) p += xh[k] * w[g][(int64_t)j * H + k];
                p += b[g][j];
                if (sd) {
                    const float z = mms::rand_normal(seed + (uint64_t)g, (uint64_t)(row_offset + m), (uint64_t)c, (uint32_t)j);
                    p += sd[j] * z;
                    if (lp) lp[m * op + j] = fmaf(-0.5f * z, z, -log_density_const(sd[j]));
                }
                out[g][m * op + j] = p;
            }
            if (sd && cnt) cnt[m] = c + 1;
        }
    }
    return 0;
}

// include/mms.h: mms_marl_heads_eval -- marl_eval_lane.h's statements, a row's sums over ascending columns in double
MMS_API int mms_marl_heads_eval(int device, int32_t groups, int64_t M, int32_t H, const float* const* h, const float* const* gamma,
                                const float* const* beta, const float* const* w, const float* const* b, const int32_t* A, const float* const* std,
                                const float* const* act, const int32_t* act_pitch, float* const* logp, const int32_t* logp_pitch,
                                const float* const* old_logp, const int32_t* old_pitch, const float* const* factor_in, float* const* factor_out,
                                float eps, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_marl_heads_eval(groups, M, H, h, gamma, beta, w, b, A, std, act, act_pitch, logp, logp_pitch, old_logp, old_pitch, factor_in,
                                      factor_out, eps)))
        return 1;
    for (int g = 0; g < groups; g++) {
        const int64_t ap = act_pitch ? act_pitch[g] : A[g], lpp = logp_pitch ? logp_pitch[g] : A[g], opp = old_pitch ? old_pitch[g] : A[g];
        float* lp = logp ? logp[g] : nullptr;
        float* fo = factor_out ? factor_out[g] : nullptr;
        const float* fi = (fo && factor_in) ? factor_in[g] : nullptr;
        const float* old = fo ? old_logp[g] : nullptr;
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++) {
            double xn[mms::kEvalMaxH];
            const float* hr = h[g] + m * H;
            if (eps >= 0.f) {
                double s = 0.0, q = 0.0;
                for (int k = 0; k < H; k++) s += (double)hr[k];
                const double mean = mms::eval_mean(s, H);
                for (int k = 0; k < H; k++) q += mms::eval_dev2(hr[k], mean);
                const double rstd = mms::eval_rstd(q, H, eps);
                for (int k = 0; k < H; k++) xn[k] = mms::eval_norm(hr[k], mean, rstd, gamma[g][k], beta[g][k]);
            } else {
                for (int k = 0; k < H; k++) xn[k] = hr[k];
            }
            double sum = 0.0;
            for (int j = 0; j < A[g]; j++) {
                double dot = 0.0;
                for (int k = 0; k < H; k++) dot += mms::eval_term(xn[k], w[g][(int64_t)j * H + k]);
                const float v = mms::eval_logp(act[g][m * ap + j], mms::eval_mu(dot, b[g][j]), std[g][j]);
                if (fo) sum += mms::eval_diff(v, old[m * opp + j]);
                if (lp) lp[m * lpp + j] = v;
            }
            if (fo) fo[m] = mms::eval_factor(fi ? fi[m] : 1.f, sum);
        }
    }
    return 0;
}

// ---- TRPO curvature products (csrc/trpo_kernels.hip): backward and R-op of an ELU MLP as plain loops -----------------------------------
// Products accumulate in double and round once (a second opinion for the HIP build, not a bit-equal copy of it).  No workspace.
static inline double elu_d1(float h) { return h > 0.f ? 1.0 : (double)h + 1.0; }
static inline double elu_d2(float h) { return h > 0.f ? 0.0 : (double)h + 1.0; }

// out [R, C] = A^T B with A [M, R], B [M, C] (+ out when acc): the contraction over rows
static void mlp_tn(int64_t M, int R, int C, const float* A, const float* B, float* out, bool acc) {
#pragma omp parallel for schedule(static)
    for (int r = 0; r < R; r++)
        for (int c = 0; c < C; c++) {
            double s = acc ? out[(int64_t)r * C + c] : 0.0;
            for (int64_t m = 0; m < M; m++) s += (double)A[m * R + r] * B[m * C + c];
            out[(int64_t)r * C + c] = (float)s;
        }
}
static void mlp_colsum(int64_t M, int R, const float* A, float* out) {
    for (int r = 0; r < R; r++) {
        double s = 0.0;
        for (int64_t m = 0; m < M; m++) s += A[m * R + r];
        out[r] = (float)s;
    }
}
// out [M, K] = sum over terms of D_t W_t (D_t [M, N], W_t [N, K]), in double, then rounded
static void mlp_nn(int64_t M, int N, int K, int terms, const float* const* D, const float* const* W, double* out) {
#pragma omp parallel for schedule(static)
    for (int64_t m = 0; m < M; m++)
        for (int k = 0; k < K; k++) {
            double s = 0.0;
            for (int t = 0; t < terms; t++)
                for (int n = 0; n < N; n++) s += (double)D[t][m * N + n] * W[t][(int64_t)n * K + k];
            out[m * K + k] = s;
        }
}

MMS_API int mms_mlp_grad(int device, int32_t L, int64_t M, const int32_t* dims, const float* x, const float* const* h, const float* const* w,
                         const float* g, float* const* dw, float* const* db, float* const* d_out, float* const* e_out, void* workspace,
                         int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_mlp_grad(L, M, dims, x, h, w, g, dw, db, d_out, e_out, workspace, ws_bytes))) return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }                  // the size query (callers pass any non-NULL workspace to run)
    std::vector<float> dcur(g, g + M * dims[L]), dnext;
    std::vector<double> e;
    for (int l = L; l >= 1; l--) {
        const float* hin = l == 1 ? x : h[l - 2];
        mlp_tn(M, dims[l], dims[l - 1], dcur.data(), hin, dw[l - 1], false);
        mlp_colsum(M, dims[l], dcur.data(), db[l - 1]);
        if (l > 1) {
            const int K = dims[l - 1];
            e.assign((size_t)M * K, 0.0);
            const float* D[1] = {dcur.data()};
            const float* W[1] = {w[l - 1]};
            mlp_nn(M, dims[l], K, 1, D, W, e.data());
            dnext.assign((size_t)M * K, 0.f);
            for (int64_t i = 0; i < M * K; i++) {
                const float ev = (float)e[i];
                if (e_out) e_out[l - 2][i] = ev;
                dnext[i] = (float)((double)ev * elu_d1(h[l - 2][i]));
                if (d_out) d_out[l - 2][i] = dnext[i];
            }
            dcur.swap(dnext);
        }
    }
    return 0;
}

MMS_API int mms_mlp_grad_rop(int device, int32_t L, int64_t M, const int32_t* dims, const float* x, const float* const* h, const float* const* w,
                             const float* const* v, const float* const* c, const float* g, const float* const* d, const float* const* e,
                             float* rmu, float* const* rdw, float* const* rdb, void* workspace, int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_mlp_grad_rop(L, M, dims, x, h, w, v, c, g, d, e, rmu, rdw, rdb, workspace, ws_bytes))) return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }
    // R-forward: Ra_l = Rh_{l-1} W_l^T + h_{l-1} V_l^T + c_l, Rh_l = f'(h_l) Ra_l
    std::vector<std::vector<float>> Ra(L + 1), Rh(L);
    for (int l = 1; l <= L; l++) {
        const int N = dims[l], K = dims[l - 1];
        const float* hin = l == 1 ? x : h[l - 2];
        Ra[l].assign((size_t)M * N, 0.f);
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++)
            for (int n = 0; n < N; n++) {
                double s = c[l - 1][n];
                for (int k = 0; k < K; k++) {
                    s += (double)hin[m * K + k] * v[l - 1][(int64_t)n * K + k];
                    if (l > 1) s += (double)Rh[l - 1][m * K + k] * w[l - 1][(int64_t)n * K + k];
                }
                Ra[l][m * N + n] = (float)s;
            }
        if (l < L) {
            Rh[l].assign((size_t)M * N, 0.f);
            for (int64_t i = 0; i < M * N; i++) Rh[l][i] = (float)(elu_d1(h[l - 1][i]) * Ra[l][i]);
        }
    }
    memcpy(rmu, Ra[L].data(), sizeof(float) * M * dims[L]);
    // R-backward
    std::vector<float> Rd;                                        // Rd_l (empty: Rd_L = 0)
    std::vector<double> T;
    for (int l = L; l >= 1; l--) {
        const int N = dims[l], K = dims[l - 1];
        const float* dl = l == L ? g : d[l - 1];
        const float* hin = l == 1 ? x : h[l - 2];
        std::vector<float> acc((size_t)N * K, 0.f);
        if (l < L) mlp_tn(M, N, K, Rd.data(), hin, acc.data(), false);
        if (l >= 2) mlp_tn(M, N, K, dl, Rh[l - 1].data(), acc.data(), l < L);
        memcpy(rdw[l - 1], acc.data(), sizeof(float) * N * K);
        if (l < L) mlp_colsum(M, N, Rd.data(), rdb[l - 1]);
        else memset(rdb[l - 1], 0, sizeof(float) * N);
        if (l >= 2) {
            T.assign((size_t)M * K, 0.0);
            const float* D[2] = {dl, Rd.data()};
            const float* W[2] = {v[l - 1], w[l - 1]};
            mlp_nn(M, N, K, l < L ? 2 : 1, D, W, T.data());
            std::vector<float> nd((size_t)M * K);
            for (int64_t i = 0; i < M * K; i++) {
                const float hv = h[l - 2][i];
                nd[i] = (float)(T[i] * elu_d1(hv) + (double)e[l - 2][i] * elu_d2(hv) * Ra[l - 1][i]);
            }
            Rd.swap(nd);
        }
    }
    return 0;
}

// ---- HATRPO's Fisher-vector product (include/mms.h: mms_ln_mlp_grad, mms_ln_mlp_jvp): plain loops ------------------------------------
// Every sum (row statistics, row means, products, column sums) accumulates in double and rounds once; what passes from one level to the
// next (da_l, du_l, Ru_l) is stored in float, as the HIP build stores it.  The workspace holds the row statistics in double.
struct LnLevel {
    const float* v;      // the level's saved activation
    const float *g, *t;
    const double* st;    // [M, 2]
    int K;
    double xhat(int64_t m, int k) const { return ((double)v[m * K + k] - st[2 * m]) * st[2 * m + 1]; }
    double u(int64_t m, int k) const { return (double)g[k] * xhat(m, k) + (double)t[k]; }
};

static void ln_stats(int64_t M, int K, const float* v, float eps, double* st) {
#pragma omp parallel for schedule(static)
    for (int64_t m = 0; m < M; m++) {
        double s = 0.0, q = 0.0;
        for (int k = 0; k < K; k++) s += v[m * K + k];
        const double mean = s / K;
        for (int k = 0; k < K; k++) q += ((double)v[m * K + k] - mean) * ((double)v[m * K + k] - mean);
        st[2 * m] = mean;
        st[2 * m + 1] = 1.0 / sqrt(q / K + (double)eps);
    }
}

static LnLevel ln_level(int l, int64_t M, const int32_t* dims, const float* x, const float* const* h, const float* const* ln_g, const float* const* ln_t,
                        float eps, void* workspace) {
    double* st = static_cast<double*>(workspace) + (size_t)l * M * 2;
    const float* v = l == 0 ? x : h[l - 1];
    ln_stats(M, dims[l], v, eps, st);
    return LnLevel{v, ln_g[l], ln_t[l], st, dims[l]};
}

MMS_API int mms_ln_mlp_grad(int device, int32_t L, int64_t M, const int32_t* dims, float eps, const float* x, const float* const* h,
                            const float* const* ln_g, const float* const* ln_t, const float* const* w, const float* g, float* const* dln_g,
                            float* const* dln_t, float* const* dw, float* const* db, void* workspace, int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    const int64_t need = check_ln_mlp_shapes("mms_ln_mlp_grad", L, M, dims, ws_bytes).empty() ? ln_mlp_cpu_ws_bytes(L, M) : 0;
    if (refused(check_ln_mlp_grad(L, M, dims, eps, x, h, ln_g, ln_t, w, g, dln_g, dln_t, dw, db, workspace, ws_bytes, need))) return 1;
    if (!workspace) { *ws_bytes = need; return 0; }               // the size query
    std::vector<float> d(g, g + M * dims[L + 1]), du, da;
    for (int j = L + 1; j >= 1; j--) {
        const int N = dims[j], K = dims[j - 1];
        const LnLevel lv = ln_level(j - 1, M, dims, x, h, ln_g, ln_t, eps, workspace);
#pragma omp parallel for schedule(static)
        for (int n = 0; n < N; n++)                                // dW_j = d_j^T u_{j-1}
            for (int k = 0; k < K; k++) {
                double s = 0.0;
                for (int64_t m = 0; m < M; m++) s += (double)d[m * N + n] * lv.u(m, k);
                dw[j - 1][(int64_t)n * K + k] = (float)s;
            }
        mlp_colsum(M, N, d.data(), db[j - 1]);
        du.assign((size_t)M * K, 0.f);
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++)                            // du_{j-1} = d_j W_j
            for (int k = 0; k < K; k++) {
                double s = 0.0;
                for (int n = 0; n < N; n++) s += (double)d[m * N + n] * w[j - 1][(int64_t)n * K + k];
                du[m * K + k] = (float)s;
            }
        for (int k = 0; k < K; k++) {
            double sg = 0.0, st = 0.0;
            for (int64_t m = 0; m < M; m++) {
                sg += (double)du[m * K + k] * lv.xhat(m, k);
                st += (double)du[m * K + k];
            }
            dln_g[j - 1][k] = (float)sg;
            dln_t[j - 1][k] = (float)st;
        }
        if (j == 1) break;
        da.assign((size_t)M * K, 0.f);
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++) {
            double m1 = 0.0, m2 = 0.0;
            for (int k = 0; k < K; k++) {
                const double q = (double)du[m * K + k] * lv.g[k];
                m1 += q;
                m2 += q * lv.xhat(m, k);
            }
            m1 /= K;
            m2 /= K;
            for (int k = 0; k < K; k++) {
                const double q = (double)du[m * K + k] * lv.g[k];
                da[m * K + k] = (float)(lv.st[2 * m + 1] * (q - m1 - lv.xhat(m, k) * m2) * elu_d1(lv.v[m * K + k]));
            }
        }
        d.swap(da);
    }
    return 0;
}

MMS_API int mms_ln_mlp_jvp(int device, int32_t L, int64_t M, const int32_t* dims, float eps, const float* x, const float* const* h,
                           const float* const* ln_g, const float* const* ln_t, const float* const* w, const float* const* vg,
                           const float* const* vt, const float* const* vw, const float* const* vc, const float* col_scale, float* rmu,
                           void* workspace, int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    const int64_t need = check_ln_mlp_shapes("mms_ln_mlp_jvp", L, M, dims, ws_bytes).empty() ? ln_mlp_cpu_ws_bytes(L, M) : 0;
    if (refused(check_ln_mlp_jvp(L, M, dims, eps, x, h, ln_g, ln_t, w, vg, vt, vw, vc, rmu, workspace, ws_bytes, need))) return 1;
    if (!workspace) { *ws_bytes = need; return 0; }               // the size query
    std::vector<float> ru, ra;
    for (int l = 0; l <= L + 1; l++) {
        if (l >= 1) {                                              // Ra_l = Ru_{l-1} W_l^T + u_{l-1} V_l^T + c_l
            const int N = dims[l], K = dims[l - 1];
            const LnLevel below{l == 1 ? x : h[l - 2], ln_g[l - 1], ln_t[l - 1], static_cast<double*>(workspace) + (size_t)(l - 1) * M * 2, K};
            ra.assign((size_t)M * N, 0.f);
#pragma omp parallel for schedule(static)
            for (int64_t m = 0; m < M; m++)
                for (int n = 0; n < N; n++) {
                    double s = vc[l - 1][n];
                    for (int k = 0; k < K; k++)
                        s += (double)ru[m * K + k] * w[l - 1][(int64_t)n * K + k] + below.u(m, k) * vw[l - 1][(int64_t)n * K + k];
                    ra[m * N + n] = (float)s;
                }
        }
        if (l == L + 1) break;
        const int K = dims[l];
        const LnLevel lv = ln_level(l, M, dims, x, h, ln_g, ln_t, eps, workspace);
        ru.assign((size_t)M * K, 0.f);
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < M; m++) {
            double m1 = 0.0, m2 = 0.0;
            if (l >= 1) {
                for (int k = 0; k < K; k++) {
                    const double rh = elu_d1(lv.v[m * K + k]) * ra[m * K + k];
                    m1 += rh;
                    m2 += rh * lv.xhat(m, k);
                }
                m1 /= K;
                m2 /= K;
            }
            for (int k = 0; k < K; k++) {
                const double xh = lv.xhat(m, k);
                double o = (double)vg[l][k] * xh + (double)vt[l][k];
                if (l >= 1) o += (double)lv.g[k] * lv.st[2 * m + 1] * (elu_d1(lv.v[m * K + k]) * ra[m * K + k] - m1 - xh * m2);
                ru[m * K + k] = (float)o;
            }
        }
    }
    const int A = dims[L + 1];
    for (int64_t m = 0; m < M; m++)
        for (int j = 0; j < A; j++) rmu[m * A + j] = col_scale ? ra[m * A + j] * col_scale[j] : ra[m * A + j];
    return 0;
}

// ---- the PPO update's loss head (include/mms.h: mms_ppo_loss) over ../ppo_loss_lane.h -----------------------------------------------
// Rows in at most 1024 chunks of at least 256 (OpenMP over chunks): a row's logp and KL term summed in double over ascending columns,
// a chunk's partials in double over ascending rows, the chunks added in ascending order and rounded once -- the result does not depend
// on the number of threads.  No workspace.
MMS_API int mms_ppo_loss(int device, int64_t M, int32_t A, const float* mu, const float* log_std, const float* value, const int64_t* indices,
                         const float* actions, const float* old_logp, const float* adv, const float* returns, const float* target_values,
                         const float* old_mu, const float* old_sigma, float clip, float value_coef, float entropy_coef, int32_t clipped_value,
                         float* out, float* dmu, float* dlog_std, float* dvalue, void* workspace, int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_ppo_loss(M, A, mu, log_std, value, actions, old_logp, adv, returns, target_values, old_mu, old_sigma, out, dmu, dlog_std, dvalue,
                               workspace, ws_bytes, 0)))
        return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }                  // the size query
    const bool grads = dmu != nullptr;
    int64_t chunk = (M + 1023) / 1024;
    chunk = chunk < 256 ? 256 : chunk;
    const int64_t nchunks = (M + chunk - 1) / chunk;
    const float inv_m = 1.0f / (float)M;
    float einv[MMS_PPO_LOSS_MAX_A], den[MMS_PPO_LOSS_MAX_A];
    double entropy = 0.0;
    for (int j = 0; j < A; j++) {
        mms::ppo_col_consts(log_std[j], einv[j], den[j]);
        entropy += (double)mms::ppo_entropy_term(log_std[j]);
    }
    std::vector<double> part((size_t)nchunks * (3 + A), 0.0);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < nchunks; c++) {
        double* p = part.data() + c * (3 + A);
        const int64_t end = (c + 1) * chunk < M ? (c + 1) * chunk : M;
        float z[MMS_PPO_LOSS_MAX_A];
        for (int64_t row = c * chunk; row < end; row++) {
            const int64_t src = indices ? indices[row] : row;
            const float *m = mu + row * A, *a = actions + src * A, *om = old_mu + src * A, *os = old_sigma + src * A;
            double logp = 0.0, kl = 0.0;
            for (int j = 0; j < A; j++) {
                logp += (double)mms::ppo_logp_term(a[j], m[j], log_std[j], einv[j], z[j]);
                kl += (double)mms::ppo_kl_term(log_std[j], os[j], om[j], m[j], den[j]);
            }
            const mms::PpoRow r = mms::ppo_row(logp, old_logp[src], adv[src], value[row], returns[src], target_values[src], clip, value_coef,
                                               clipped_value != 0, inv_m);
            p[0] += (double)r.surrogate;
            p[1] += (double)r.value_loss;
            p[2] += kl;
            if (grads) {
                dvalue[row] = r.dvalue;
                for (int j = 0; j < A; j++) {
                    dmu[row * A + j] = mms::ppo_dmu(r.g, z[j], einv[j]);
                    p[3 + j] += (double)mms::ppo_dlog_std_term(r.g, z[j]);
                }
            }
        }
    }
    std::vector<double> tot(3 + A, 0.0);
    for (int64_t c = 0; c < nchunks; c++)
        for (int q = 0; q < 3 + A; q++) tot[q] += part[c * (3 + A) + q];
    mms::ppo_finish_scalars(tot[0], tot[1], tot[2], entropy, M, value_coef, entropy_coef, out);
    if (grads)
        for (int j = 0; j < A; j++) dlog_std[j] = mms::ppo_finish_dlog_std(tot[3 + j], entropy_coef);
    return 0;
}

// ---- the head of TRPO's policy step (include/mms.h: mms_trpo_heads) over ../trpo_loss_lane.h -----------------------------------------
// Chunks and sums as mms_ppo_loss above: a row's logp and KL term in double over ascending columns, a chunk's two partials in double
// over ascending rows, the chunks added in ascending order, one division by M and one rounding.  No workspace.
MMS_API int mms_trpo_heads(int device, int64_t M, int32_t A, const float* mu, const float* log_std, const float* rmu, const int64_t* indices,
                           const float* actions, const float* adv, const float* old_mu, const float* old_sigma, const float* old_logp,
                           int32_t old_logp_dense, float* out, float* logp_out, float* gsur, float* gkl, float* gn, void* workspace, int64_t* ws_bytes,
                           void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_trpo_heads(M, A, mu, log_std, rmu, actions, adv, old_mu, old_sigma, old_logp, out, logp_out, gsur, gkl, gn, workspace, ws_bytes, 0)))
        return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }                  // the size query
    const bool sums = out != nullptr, want_lp = sums || logp_out || gsur, want_r = sums || gsur;
    int64_t chunk = (M + 1023) / 1024;
    chunk = chunk < 256 ? 256 : chunk;
    const int64_t nchunks = (M + chunk - 1) / chunk;
    const float inv_m = 1.0f / (float)M;
    float einv[MMS_PPO_LOSS_MAX_A], den[MMS_PPO_LOSS_MAX_A], cden[MMS_PPO_LOSS_MAX_A];
    for (int j = 0; j < A; j++) {
        mms::ppo_col_consts(log_std[j], einv[j], den[j]);
        cden[j] = mms::trpo_col_den(log_std[j], M);
    }
    std::vector<double> part((size_t)nchunks * 2, 0.0);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < nchunks; c++) {
        double* p = part.data() + c * 2;
        const int64_t end = (c + 1) * chunk < M ? (c + 1) * chunk : M;
        float z[MMS_PPO_LOSS_MAX_A];
        for (int64_t row = c * chunk; row < end; row++) {
            const int64_t src = indices ? indices[row] : row;
            double logp = 0.0, kl = 0.0;
            if (want_lp)
                for (int j = 0; j < A; j++) logp += (double)mms::ppo_logp_term(actions[src * A + j], mu[row * A + j], log_std[j], einv[j], z[j]);
            if (sums)
                for (int j = 0; j < A; j++)
                    kl += (double)mms::ppo_kl_term(log_std[j], old_sigma[src * A + j], old_mu[src * A + j], mu[row * A + j], den[j]);
            float g = 0.f;
            if (want_r) {
                const mms::TrpoRow r = mms::trpo_row(logp, old_logp[old_logp_dense ? row : src], adv[src], inv_m);
                g = r.g;
                if (sums) p[0] += (double)r.term;
            }
            if (sums) p[1] += kl;
            if (logp_out) logp_out[row] = (float)logp;
            for (int j = 0; j < A; j++) {
                if (gsur) gsur[row * A + j] = mms::trpo_gsur(g, z[j], einv[j]);
                if (gkl) gkl[row * A + j] = mms::trpo_gkl(mu[row * A + j], old_mu[src * A + j], cden[j]);
                if (gn) gn[row * A + j] = mms::trpo_gn(rmu[row * A + j], cden[j]);
            }
        }
    }
    if (sums) {
        double tot[2] = {0.0, 0.0};
        for (int64_t c = 0; c < nchunks; c++)
            for (int q = 0; q < 2; q++) tot[q] += part[c * 2 + q];
        out[0] = mms::trpo_finish_mean(tot[0], M);
        out[1] = mms::trpo_finish_mean(tot[1], M);
    }
    return 0;
}

// ---- the MAPPO / HAPPO update's loss head (include/mms.h: mms_marl_ppo_loss) over ../marl_loss_lane.h -------------------------------
// Chunks and sums as mms_ppo_loss above: a row's sums in double over ascending columns, a chunk's partials in double over ascending
// rows, the chunks added in ascending order and rounded once; the mask sum in double over ascending rows.  No workspace.
static void marl_ppo_loss_one(int64_t M, int32_t A, const float* mu, const float* std, const float* value, const int64_t* indices,
                              const mms_marl_loss_fields& f, float clip, float value_loss_coef, float entropy_coef, float huber_delta, int32_t use_huber,
                              int32_t clipped_value, int32_t policy_masks, int32_t value_masks, int32_t use_norm, const float* norm_mean,
                              const float* norm_var, float* out, float* dmu, float* dstd, float* dvalue, float* row_logp) {
    const bool grads = dmu != nullptr, pm = policy_masks != 0, vm = value_masks != 0;
    int64_t chunk = (M + 1023) / 1024;
    chunk = chunk < 256 ? 256 : chunk;
    const int64_t nchunks = (M + chunk - 1) / chunk;
    const double inv_m = 1.0 / (double)M;
    mms::MarlCol col[MMS_MARL_LOSS_MAX_A];
    double entropy = 0.0;
    for (int j = 0; j < A; j++) {
        col[j] = mms::marl_col_consts(std[j]);
        entropy += mms::marl_entropy_term(std[j]);
    }
    mms::MarlScalars sc;
    sc.clip = clip; sc.value_coef = value_loss_coef; sc.delta = huber_delta;
    sc.huber = use_huber != 0; sc.clipped_value = clipped_value != 0; sc.use_norm = use_norm != 0;
    sc.norm_mean = use_norm ? (double)norm_mean[0] : 0.0;
    sc.norm_inv_sd = use_norm ? 1.0 / sqrt((double)norm_var[0]) : 1.0;
    double msum = 0.0;
    if (pm || vm)
        for (int64_t row = 0; row < M; row++) msum += (double)f.active_masks.base[(indices ? indices[row] : row) * f.active_masks.pitch];
    const double inv_msum = (pm || vm) ? 1.0 / msum : 0.0;
    std::vector<double> part((size_t)nchunks * (3 + A), 0.0);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < nchunks; c++) {
        double* p = part.data() + c * (3 + A);
        const int64_t end = (c + 1) * chunk < M ? (c + 1) * chunk : M;
        float d[MMS_MARL_LOSS_MAX_A];
        for (int64_t row = c * chunk; row < end; row++) {
            const int64_t src = indices ? indices[row] : row;
            const float *m = mu + row * A, *a = f.actions.base + src * f.actions.pitch, *ol = f.old_logp.base + src * f.old_logp.pitch;
            double dlogp = 0.0, logp = 0.0;
            for (int j = 0; j < A; j++) {
                const double t = mms::marl_logp_term(a[j], m[j], col[j], d[j]);
                dlogp += t - (double)ol[j];
                logp += t;
            }
            const float mask = (pm || vm) ? f.active_masks.base[src * f.active_masks.pitch] : 1.0f;
            const float fac = f.factor.base ? f.factor.base[src * f.factor.pitch] : 1.0f;
            const mms::MarlRow r = mms::marl_row(dlogp, f.adv.base[src * f.adv.pitch], fac, value[row], f.value_preds.base[src * f.value_preds.pitch],
                                                 f.returns.base[src * f.returns.pitch], sc, pm ? (double)mask * inv_msum : inv_m, vm ? (double)mask * inv_msum : inv_m);
            p[0] += pm ? (double)mask * (double)r.surrogate : (double)r.surrogate;
            p[1] += vm ? (double)mask * (double)r.value_loss : (double)r.value_loss;
            p[2] += (double)r.ratio;
            if (row_logp) row_logp[row] = (float)logp;
            if (grads) {
                dvalue[row] = r.dvalue;
                for (int j = 0; j < A; j++) {
                    dmu[row * A + j] = mms::marl_dmu(r.g, d[j], col[j]);
                    p[3 + j] += mms::marl_dstd_term(r.g, d[j], col[j]);
                }
            }
        }
    }
    std::vector<double> tot(3 + A, 0.0);
    for (int64_t c = 0; c < nchunks; c++)
        for (int q = 0; q < 3 + A; q++) tot[q] += part[c * (3 + A) + q];
    const double ent_scale = pm ? 1.0 : 1.0 / (double)A;
    mms::marl_finish_scalars(tot[0], tot[1], tot[2], entropy, pm ? msum : (double)M, vm ? msum : (double)M, ent_scale, M, value_loss_coef, entropy_coef, out);
    if (grads)
        for (int j = 0; j < A; j++) dstd[j] = mms::marl_finish_dstd(tot[3 + j], std[j], entropy_coef, ent_scale);
}

MMS_API int mms_marl_ppo_loss(int device, int64_t M, int32_t A, const float* mu, const float* std, const float* value, const int64_t* indices,
                              const mms_marl_loss_fields* fields, float clip, float value_loss_coef, float entropy_coef, float huber_delta,
                              int32_t use_huber, int32_t clipped_value, int32_t policy_masks, int32_t value_masks, int32_t use_norm,
                              const float* norm_mean, const float* norm_var, float* out, float* dmu, float* dstd, float* dvalue, float* row_logp,
                              void* workspace, int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_marl_ppo_loss(M, A, mu, std, value, fields, policy_masks, value_masks, use_norm, norm_mean, norm_var, out, dmu, dstd, dvalue,
                                    workspace, ws_bytes, 0)))
        return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }                  // the size query
    marl_ppo_loss_one(M, A, mu, std, value, indices, *fields, clip, value_loss_coef, entropy_coef, huber_delta, use_huber, clipped_value, policy_masks,
                      value_masks, use_norm, norm_mean, norm_var, out, dmu, dstd, dvalue, row_logp);
    return 0;
}

// one group after the other, each as the single entry evaluates it: group g's bits are mms_marl_ppo_loss's on group g's arguments
MMS_API int mms_marl_ppo_loss_group(int device, int32_t groups, int64_t M, int32_t A, const mms_marl_loss_group* table, float clip,
                                    float value_loss_coef, float entropy_coef, float huber_delta, int32_t use_huber, int32_t clipped_value,
                                    int32_t policy_masks, int32_t value_masks, int32_t use_norm, void* workspace, int64_t* ws_bytes, void*) {
    if (cpu_only(device)) return 1;
    if (refused(check_marl_ppo_loss_group(groups, M, A, table, policy_masks, value_masks, use_norm, workspace, ws_bytes, 0))) return 1;
    if (!workspace) { *ws_bytes = 0; return 0; }                  // the size query
    for (int g = 0; g < groups; g++) {
        const mms_marl_loss_group& t = table[g];
        marl_ppo_loss_one(M, A, t.mu, t.std, t.value, t.indices, t.fields, clip, value_loss_coef, entropy_coef, huber_delta, use_huber, clipped_value,
                          policy_masks, value_masks, use_norm, t.norm_mean, t.norm_var, t.out, t.dmu, t.dstd, t.dvalue, t.row_logp);
    }
    return 0;
}
