/*
 * mms.h -- C ABI of the MI355X-native multi-agent physics + rollout engine ("mms").
 *
 * This is the INNER drop-in boundary: what the reference's task files obtain
 * today from the closed Isaac Gym binary through `self.gym.*` calls.  The reference has no FFI of
 * its own for this path (it is Python calling a vendor binary), so each entry point cites the
 * reference call sites it replaces.  Plain pointers and sizes only; no torch types.
 *
 *   reference call site (under /root/reference)                         replaced by
 *   ------------------------------------------------------------------  -----------------------
 *   gymapi.acquire_gym / create_sim / add_ground / create_env /          mms_create
 *     load_asset / create_box / create_actor / prepare_sim
 *     (agents/tasks/agent_base/base_task.py:25,83,122;
 *      agents/tasks/ten_ant.py:205-633; one_ant.py:150-312;
 *      multi_ingenuity.py:120-226)
 *   acquire_actor_root_state_tensor / acquire_dof_state_tensor /         mms_get_tensor
 *     acquire_force_sensor_tensor + gymtorch.wrap_tensor
 *     (ten_ant.py:84-104; one_ant.py:78-103; multi_ingenuity.py:77-95)
 *   pre_physics_step + gym.simulate + fetch_results +                    mms_step
 *     post_physics_step (refresh_*, reset_idx, compute_observations,
 *     compute_reward)  (base_task.py:129-149; ten_ant.py:886-926)
 *   set_actor_root_state_tensor_indexed / set_dof_state_tensor_indexed   mms_set_state (tests),
 *     (ten_ant.py:856-868)                                               in-kernel reset
 *   RolloutStorage.compute_returns (algorithms/rl/ppo/storage.py:51-65)  mms_gae_ppo
 *   SeparatedReplayBuffer.compute_returns                                mms_gae_marl
 *     (algorithms/marl/utils/separated_buffer.py:153-164)
 *   MultiVecTaskPython.step slicing (agent_base/multi_vec_task.py:       mms_marl_views
 *     105-142)
 *   apply_randomizations actor_params: set_actor_rigid_body_properties   mms_set_dr + "dr_params"
 *     / set_actor_dof_properties (base_task.py:343-395)
 *   ActorCritic.act sampling tail + RolloutStorage.add_transitions       mms_ppo_act, mms_ppo_heads_act,
 *     (algorithms/rl/ppo/module.py:73-87; storage.py:33-47)              mms_bind_rollout_out
 *   ActorCritic hidden layers (module.py:27-52)                          mms_linear2_act, mms_linear_group_act_split,
 *                                                                        mms_split_planes(_group), mms_split_planes16_group,
 *                                                                        mms_linear_group_act_split16, mms_row_stats_chan_group,
 *                                                                        mms_marl_heads_finish
 *   Actor / Critic forward of every MAPPO / HAPPO agent                  mms_linear_group_act, mms_layernorm_group,
 *     (algorithms/marl/actor_critic.py:43-69, 137-155; runner.py:186-216)  mms_row_stats_group, mms_marl_heads_act
 *   Actor.evaluate_actions before and after every agent's update and    mms_marl_heads_eval (behind the grouped layers)
 *     the factor product of Runner.train (algorithms/marl/runner.py:282-313;
 *     utils/act.py evaluate_actions; utils/distributions.py:31-34)
 *   RNNLayer's single-step branch of every recurrent agent              mms_gru_group, mms_gru_gates_group
 *     (algorithms/utils/rnn.py:25-29; marl/actor_critic.py:64-65, 164-165)
 *   RNNLayer's sequence branch in ppo_update and autograd's backward    mms_gru_gates_group (forward),
 *     through time of its nn.GRU pieces (algorithms/utils/rnn.py:30-77;   mms_gru_gates_grad_group (backward); opt-in,
 *     reached from marl/mappo_trainer.py:130, happo_trainer.py:121)       config key fused_rnn_update
 *   MLPLayer's Linear + ELU + LayerNorm blocks in ppo_update and         mms_elu_ln_group (forward),
 *     autograd's backward of them (algorithms/utils/mlp.py:19-35;          mms_elu_ln_grad_group (backward); opt-in,
 *     reached from marl/mappo_trainer.py:124-130, happo_trainer.py:115)    config key fused_block_update
 *   ... with the blocks' forward products on the two-plane fp16 layer     mms_elu_ln_planes16_group (forward, leaves y as
 *     kernel instead of the library                                        fp32 and as H32 planes); opt-in, config key block_products
 *   DiagGaussian.fc_mean with its std expression and Critic.v_out in     mms_marl_heads_fwd_group (forward),
 *     ppo_update, and autograd's backward of them                          mms_marl_heads_grad_group (backward); opt-in,
 *     (algorithms/utils/distributions.py:94-117; actor_critic.py)          config key fused_head_update
 *   SquashedGaussianMLPActor heads + rsample + log-probability          mms_sac_heads_act
 *     (algorithms/rl/sac/module.py:23-61; sac.py:166, 374-376)
 *   autograd's backward of that head's epilogue in compute_loss_pi      mms_sac_heads_grad
 *     (sac.py:392-403)
 *   MLPQFunction last layer + min + Bellman backup (Q target)           mms_q_heads_backup
 *     (rl/sac/sac.py:379-382; td3/td3.py:370-373; ddpg/ddpg.py:368-369)
 *   MLPQFunction's torch.cat([obs, act]) in front of the two-plane      mms_split_planes16_cat
 *     fp16 layers (rl/{ddpg,td3,sac}/module.py, layers="f16x2")
 *   TRPO actor backward: torch.autograd.grad of the surrogate loss      mms_mlp_grad
 *     (algorithms/rl/trpo/trpo.py:290) and the create_graph=True
 *     gradient of the KL (:427)
 *   TRPO double backward of the KL's Hessian-vector product (:431)      mms_mlp_grad_rop
 *   TRPO.update's policy-step head behind ActorCritic.evaluate:         mms_trpo_heads
 *     surrogate, KL, their gradients with respect to mu, the KL's
 *     Gauss-Newton column scaling and the line search's scalar
 *     (algorithms/rl/trpo/trpo.py:287-298, 417-435, 464-478)
 *   HATRPO.fisher_vector_product / trpo_update's actor gradient         mms_ln_mlp_grad, mms_ln_mlp_jvp
 *     (algorithms/marl/hatrpo_trainer.py:170-179, :236)
 *   PPO.update's loss head: KL, clipped surrogate, value loss, entropy  mms_ppo_loss
 *     and their backward (algorithms/rl/ppo/ppo.py:270-302)
 *   MAPPO / HAPPO ppo_update's loss head: surrogate, entropy, PopArt /   mms_marl_ppo_loss
 *     Huber value loss, masks and their backward
 *     (algorithms/marl/mappo_trainer.py:63-179, happo_trainer.py:48-170)
 *   ... for every agent of a MAPPO run at once (the agents' updates      mms_marl_ppo_loss_group
 *     are independent: base_runner.py / runner.py's train loop)
 *   MADDPG: every agent's deterministic actor head, exploration noise    mms_det_heads_act_group
 *     and the joint action row (algorithms/marl/maddpg/module.py:36-46,
 *     :165-175); every agent's Q target tail (:218-219)                  mms_q_heads_backup_group
 *   DDPG / TD3: MLPActor's last Linear + tanh + act_limit, the target     mms_det_heads_act
 *     policy smoothing (rl/td3/td3.py:361-367, rl/ddpg/ddpg.py:357-365)
 *     and the exploration noise of act (rl/ddpg/module.py:52-58)
 *   autograd's backward of that head's epilogue in compute_loss_pi      mms_det_heads_grad
 *     (td3.py:383-388, ddpg.py:377-381)
 *   clip_grad_norm_ + Adam.step() + the polyak loop of every learner     mms_param_step
 *     (rl/sac/sac.py:325-349, rl/ppo/ppo.py, marl/mappo_trainer.py,
 *     marl/maddpg/module.py:280-292)
 *
 * Ownership: the engine owns every buffer it reports through mms_get_tensor for the lifetime of the
 * handle; callers wrap them as NON-owning views and must keep the handle alive while any view exists.
 * Threading: a handle is not thread-safe; one handle per process / GPU.  All work is enqueued on the
 * caller's HIP stream; no entry point synchronises the device except mms_create / mms_destroy.
 * Status: 0 = ok; non-zero = error, text from mms_last_error().
 * There is NO CPU fallback: mms_create of libmms.so fails when no HIP device is usable.  A SEPARATE library, libmms_cpu.so, exports
 * the same symbols for the reference's `--sim_device cpu` pipeline (base_task.py:27-32): the same lane math compiled for the host
 * (csrc/cpu/), selected only by device = -1 / device_type = "cpu", never automatically.  Device arguments of the free functions
 * (mms_gae_*, mms_ppo_*, mms_linear2_act, mms_marl_views) follow the same rule; streams are ignored by the CPU build.
 * Every entry point leaves the caller's current HIP device unchanged.
 */
#ifndef MMS_H
#define MMS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMS_ABI_VERSION 4
#define MMS_DR_FLOATS 33       /* per-ant physical domain-randomisation block, see mms_set_dr */

enum mms_task { MMS_TASK_TEN_ANT = 0, MMS_TASK_ONE_ANT = 1, MMS_TASK_MULTI_INGENUITY = 2,
                /* agents/tasks/multi_ant_circle.py: two ants per env at (+-3, 0, 1), no box in the scene, 38 observation entries per ant
                 * (the same as TenAnt's), reward for walking round the r = 3 ring.  The reference cannot import or construct this task
                 * (numpy calls and bool arithmetic inside @torch.jit.script, a 19-argument call of a 16-parameter function, not
                 * registered, no YAML): what is built is its INTENDED semantics, pinned by fixtures from a patched temp copy
                 * (tests/golden/make_circle_fixture.py).  The engine keeps an inert box actor far from the ants (the ant kernels'
                 * layouts carry box lanes): root_states is [N * 3, 13], the reference's two ant rows first. */
                MMS_TASK_MULTI_ANT_CIRCLE = 3 };
enum mms_dtype { MMS_F32 = 0, MMS_I64 = 1, MMS_I32 = 2, MMS_U8 = 3 };

/* Physical model (numbers are produced by massive_marl_benchmark_amd/model.py
 * from the MJCF geometry).  All SI units, float32. */
typedef struct mms_model {
    /* ant: torso + 4 x (leg, foot); body frames are aligned at q = 0 */
    float torso_mass, torso_ixx, torso_izz, torso_radius;
    float leg_mass, leg_ia, leg_it;      /* capsule axial / transverse inertia about its COM */
    float foot_mass, foot_ia, foot_it;
    float limb_radius, leg_len, foot_len; /* capsule radius and segment lengths */
    float hip_pos[4][3];                 /* hip joint position in the torso frame */
    float limb_dir[4][3];                /* unit capsule direction of leg and foot at q = 0 */
    float ankle_axis[4][3];              /* unit ankle axis in the leg frame */
    float dof_lower[8], dof_upper[8], dof_init[8], gear[8];
    float armature, joint_damping, limit_k, limit_c, limit_ramp;
    /* contact (compliant, linearly-implicit) */
    float gnd_k, gnd_c, gnd_mu, slip_eps, pen_ramp;
    float antbox_k, antbox_c;
    float antbox_mu;                     /* ant-box Coulomb friction (regularised like the ground's); 0 = frictionless contact */
    float boxgnd_k, boxgnd_c;
    float boxgnd_mu;                     /* box-ground Coulomb friction; 0 = frictionless */
    /* box */
    float box_half[3], box_mass, box_inertia[3];
    /* helicopter (MultiIngenuity): one rigid body */
    float heli_mass, heli_inertia[3], heli_com_z, heli_rotor_z[2], heli_half, heli_max_angvel;
    float heli_gnd_k, heli_gnd_c;
    float gravity;                       /* positive magnitude along -z */
} mms_model;

typedef struct mms_config {
    int32_t abi_version;                 /* MMS_ABI_VERSION */
    int32_t task;                        /* enum mms_task */
    int32_t num_envs;                    /* envs owned by this handle (this GPU's shard) */
    int32_t num_agents;                  /* ants (10 / 1) or helicopters (4) per env */
    int32_t device;                      /* HIP device ordinal (>= 0) for libmms.so; -1 for libmms_cpu.so, the explicit opt-in CPU build */
    int32_t substeps;                    /* physics substeps per control step (cfg sim.substeps = 2) */
    int32_t max_episode_length;          /* cfg env.episodeLength */
    int32_t external_noise;              /* 1: reset noise is read from the "reset_noise" tensor */
    int64_t env_offset;                  /* global index of local env 0 (multi-GPU sharding) */
    int64_t total_envs;                  /* global env count: env-grid row length = (int)sqrt(total) */
    uint64_t seed;
    float env_spacing;                   /* cfg env.envSpacing */
    float dt;                            /* cfg sim.dt */
    float clip_actions, clip_obs;        /* wrapper clamps (vec_task.py:18,127,131) */
    float dof_vel_scale, contact_force_scale, power_scale;
    float heading_weight, up_weight, actions_cost, energy_cost, joints_at_limit_cost;
    float death_cost, termination_height;
    float quat_reward_scale, ant_dist_reward_scale, goal_dist_reward_scale;
    float ant_start_x, ant_start_z;      /* ant k starts at (x, s_k*(1.5+3*(k/2)), z), s = -,+,-,+ ... */
    float box_start[3];
    mms_model model;
} mms_config;

typedef struct mms_tensor {
    void*   ptr;                         /* device pointer */
    int64_t shape[4];
    int32_t ndim;
    int32_t dtype;                       /* enum mms_dtype */
    int32_t device;                      /* HIP device ordinal */
    int32_t reserved;
} mms_tensor;

typedef struct mms_engine* mms_handle;

/* Builds the scene for cfg->num_envs environments on cfg->device and allocates all state.
 * Replaces create_sim ... prepare_sim (see table above). */
int mms_create(const mms_config* cfg, mms_handle* out);
int mms_destroy(mms_handle h);

/* Named buffers.  Common: "actions" [N,num_actions] f32 (input of mms_step), "obs" [N,obs_dim] f32,
 * "obs_clipped" [N,obs_dim] f32 (clamped to +-clip_obs), "rew" [N] f32, "reset" [N] i64,
 * "progress" [N] i64, "root_states" [N*actors,13] f32 (env-local frame), "dof_state" [N*dofs,2] f32,
 * "env_origin" [N,3] f32, "prev" [N,prev_dim] f32 (pos_before / goal_before / box_before caches),
 * "reset_noise" [N,16] f32, "foot_sensors" [N*A,24] f32, "initial_root_states" [N*actors,13] f32,
 * "dr_params" [N*A,MMS_DR_FLOATS] f32 (see mms_set_dr),
 * "reset_count" [N] i64 (number of resets of each env so far: the counter of the reset-noise RNG, keyed with
 * the seed and the GLOBAL env index, so results do not depend on how envs are sharded over GPUs). */
int mms_get_tensor(mms_handle h, const char* name, mms_tensor* out);

/* One VecTask step: clamp actions, physics substeps, progress += 1, reset flagged envs,
 * observations, reward / reset flags, cache update -- one fused launch, stream ordered.
 * Replaces BaseTask.step (base_task.py:129-149). */
int mms_step(mms_handle h, void* hip_stream);

/* Same protocol with the physics skipped: the post-physics glue applied to whatever state the
 * buffers hold.  Used by the parity tests that supply state per step (fixture tenant_step_glue). */
int mms_post_step(mms_handle h, void* hip_stream);

/* Flags every env for reset (reset_buf := 1), as at construction (base_task.py:62-63). */
int mms_reset_all(mms_handle h, void* hip_stream);

/* Copies caller data (device or host pointer, `src_is_host`) into a named buffer.  env_ids == NULL
 * copies the whole buffer; otherwise `src` holds n rows (one per listed env) that are scattered.
 * Tests / fixtures only. */
int mms_set_state(mms_handle h, const char* name, const void* src, int src_is_host,
                  const int64_t* env_ids, int64_t n, void* hip_stream);

/* Optional extra destination for the clamped observation row, e.g. slot t of a rollout buffer
 * [T,N,obs_dim]; NULL disables.  The pointer must stay valid until the next bind. */
int mms_bind_obs_out(mms_handle h, void* dst);

/* Optional extra destination for the clamped observation row AS THE POLICY LAYERS' OPERAND PLANES (format H32 of
 * mms_linear_group_act_split16 below: f16 [N, ceil(obs_dim / 32), 2, 32], MMS_H32_BYTES(N, obs_dim) bytes, 16-byte aligned): hi and lo
 * planes of row * scale.  The row is bounded by clip_observations, so the scale is a constant (a power of two, clip_observations * scale
 * <= 2^14) and the policy needs no split pass over the observation (x_inv = 1 / scale for every row).  NULL disables.  Ant tasks only. */
int mms_bind_obs_planes16(mms_handle h, void* planes, float scale);

/* Optional source of the actions: mms_step reads `src` (f32 [N, num_actions], on the engine's device) IN PLACE instead of the
 * engine's own "actions" buffer -- the tensor VecTaskPython.step(actions) was handed (vec_task.py:126-131 clamps and copies it into
 * the task; here the clamp is in the kernel and the copy is gone).  NULL returns to the "actions" buffer.  The pointer must stay
 * valid until the next bind. */
int mms_bind_actions(mms_handle h, const float* src);

/* Physical domain randomisation of the ants (cfg/TenAnt.yaml:97-122 actor_params, applied by base_task.py:343-395 through
 * set_actor_rigid_body_properties / set_actor_dof_properties).  The caller fills "dr_params" [N*A, MMS_DR_FLOATS] per ant:
 *   [0] torso, [1..4] leg, [5..8] foot mass scale (the inertia scales with the mass: recomputeInertia is the setter's default),
 *   [9..16] joint damping scale, [17..24] lower-limit offset, [25..32] upper-limit offset (rad), joints in DOF order;
 * mms_set_dr(h, 1) makes mms_step use it (a separate kernel instantiation: the nominal path carries none of it).  The
 * observations keep the nominal limits, as the reference's do (ten_ant.py:588-599 reads them once at construction).
 * DOF stiffness is not a parameter of this path: the tasks drive the joints in effort mode (ten_ant.py:274).
 * DR and a bound policy head exclude each other in both directions and in both builds (the fused head's step kernel has no DR form):
 * mms_bind_policy_head fails while DR is on, and mms_set_dr(h, 1) while a head is bound returns non-zero with a message that names
 * mms_bind_policy_head and changes nothing -- the head stays bound for the next mms_step, DR stays off.  mms_set_dr(h, 0) always
 * succeeds. */
int mms_set_dr(mms_handle h, int32_t enable);

/* Which of the engine-owned observation rows mms_step writes: "obs" (raw, = task.obs_buf of the reference) and "obs_clipped"
 * (what VecTaskPython.step returns, vec_task.py:131).  Both on by default.  A rollout that binds a slot with mms_bind_obs_out
 * needs neither while the slot is bound: one 1552-B row per env-step instead of three.  A row that is switched off keeps its
 * last contents. */
int mms_set_obs_outputs(mms_handle h, int32_t raw, int32_t clipped);

/* Optional extra destinations for the step's reward (f32 [N]) and done flag (u8 [N], = reset_buf after the step), e.g.
 * RolloutStorage.rewards[t] / dones[t] (storage.py:40-41): add_transitions then has nothing left to copy for them.
 * NULL disables either.  Pointers must stay valid until the next bind. */
int mms_bind_rollout_out(mms_handle h, float* rew_out, uint8_t* done_out);

/* MARL wrapper views (multi_vec_task.py:105-142): obs_all [N,A,per_agent+shared] from a clamped
 * observation buffer [N, A*per_agent+shared].  n >= 0 (n = 0: an empty batch, nothing is read or written), agents >= 1,
 * per_agent >= 1, shared >= 0, both pointers required when n > 0.  Bad arguments return non-zero with mms_last_error(NULL) and write
 * nothing. */
int mms_marl_views(int device, const float* obs_clipped, float* obs_all, int64_t n, int32_t agents,
                   int32_t per_agent, int32_t shared, void* hip_stream);

/* PPO GAE (storage.py:51-65).  rewards/values/returns/advantages are [T,N] f32, dones [T,N] u8,
 * last_values [N].  Writes returns and UN-normalised advantages, and stats[0..2] =
 * {sum(adv), sum(adv^2), count} as float64 so that ranks can all-reduce them.  Every pointer is required, T >= 1, N >= 1.  Bad
 * arguments return non-zero with mms_last_error(NULL) and write nothing. */
int mms_gae_ppo(int device, const float* rewards, const uint8_t* dones, const float* values,
                const float* last_values, float* returns, float* advantages, double* stats,
                int32_t T, int64_t N, float gamma, float lam, void* hip_stream);
/* advantages := (advantages - mean) / (std + 1e-8) with the unbiased std from stats.  Both pointers are required, count >= 1.  Bad
 * arguments return non-zero with mms_last_error(NULL) and write nothing. */
int mms_adv_normalize(int device, float* advantages, const double* stats, int64_t count, void* hip_stream);
/* mms_gae_ppo + mms_adv_normalize for ONE rank (nothing to all-reduce in between), the whole of storage.py:51-65: the scan leaves
 * per-block partial sums instead of float64 atomics and the normalisation sums them in a fixed order -- bit-reproducible, and stats
 * needs no zeroing (the atomics' 24-byte memset costs two fill kernels inside a captured rollout).  stats: f64 [MMS_GAE_STATS_DOUBLES]
 * = {sum(adv), sum(adv^2), count} of the un-normalised advantages, then scratch for the partials.  Every pointer is required, T >= 1,
 * N >= 1.  Bad arguments return non-zero with mms_last_error(NULL) and write nothing. */
#define MMS_GAE_STATS_DOUBLES (3 + 2 * 2048)
int mms_gae_ppo_normalized(int device, const float* rewards, const uint8_t* dones, const float* values, const float* last_values,
                           float* returns, float* advantages, double* stats, int32_t T, int64_t N, float gamma, float lam,
                           void* hip_stream);

/* Diagnostics: the clock the chip holds inside the two-plane layer kernel (mms_linear_group_act_split16).  With `out` (device memory,
 * 2 x slots uint64, 8-byte aligned) every such launch issued after this call stores, by its workgroup 0, {shader cycles, 100-MHz ticks}
 * of that workgroup's life into out[2 (n % slots)], n = 0, 1, ... counting launches from this call: cycles / ticks x 0.1 = GHz.  The
 * reference has no counterpart (torch modules, agents/algorithms/rl/ppo/module.py:27-52); bench.py reports the figure beside
 * `roofline_policy_layers` because the kernel runs power-limited: its MFMA rate has to be read against the clock it is granted, not
 * against the 2.4 GHz the dense peak is quoted at.  out = NULL switches the probe off (the default).  Process-wide, not thread-safe;
 * launches captured in a hipGraph keep the slot they were captured with.  The CPU build accepts the call and stores nothing. */
int mms_layer_clock_probe(int device, uint64_t* out, int32_t slots);

/* MARL GAE (separated_buffer.py:153-164, use_proper_time_limits=False): value_preds [T+1,N]
 * (row T already holds next_value), masks [T+1,N], rewards [T,N], returns [T+1,N];
 * denormalisation x*sqrt(var)+mean when use_norm (PopArt / ValueNorm): norm_mean and norm_var [1] are then required (and not read
 * otherwise).  Row T of returns is not written.  rewards, value_preds, masks and returns are required, T >= 1, N >= 1.  Bad arguments
 * return non-zero with mms_last_error(NULL) and write nothing. */
int mms_gae_marl(int device, const float* rewards, const float* value_preds, const float* masks,
                 float* returns, int32_t T, int64_t N, float gamma, float lam,
                 int32_t use_norm, const float* norm_mean, const float* norm_var, void* hip_stream);

/* The same for all A agents of all envs in one launch (rollout-buffer fusion):
 * value_preds / returns [T+1,N,A] (agent fastest), rewards [T,N] and masks [T+1,N] stored once per env instead of
 * once per agent buffer (runner.py:250-255 inserts the same reward / mask into ten buffers); norm_mean / norm_var [A].  The same
 * rules, and A >= 1.  Bad arguments return non-zero with mms_last_error(NULL) and write nothing. */
int mms_gae_marl_agents(int device, const float* rewards, const float* value_preds, const float* masks,
                        float* returns, int32_t T, int64_t N, int32_t A, float gamma, float lam,
                        int32_t use_norm, const float* norm_mean, const float* norm_var, void* hip_stream);

/* The tail of ActorCritic.act (algorithms/rl/ppo/module.py:73-87) fused with RolloutStorage.add_transitions
 * (storage.py:33-47): Gaussian sample, log-probability and the stores of one rollout step in ONE launch
 * (SURVEY.md section 8f item 4).  mean [N,A] and value [N] are the outputs of the actor / critic MLPs.
 *   noise_ij ~ N(0,1): counter-based (seed, global row = row_offset + i, counters[i], j), Box-Muller; counters[i] += 1
 *   scale_j  = exp(log_std_j)^2 when reference_scale != 0 -- module.py:76-77 hands diag(sigma^2) to scale_tril -- else exp(log_std_j)
 *   action   = mean + scale * noise;   log_prob_i = sum_j (-0.5 noise_ij^2 - log(scale_j) - 0.5 log(2 pi))
 * Destinations (any may be NULL): actions_out [N,A] (e.g. the engine's "actions" buffer), act_slot / mu_slot / sigma_slot
 * [N,A], logp_slot / value_slot [N].  sigma_slot receives log_std broadcast, which is what module.py:87 returns as sigma.
 * counters is a device array [N] of int64 so that a captured hipGraph draws fresh noise on every replay.
 * mean, log_std and counters are required, N >= 0 (N = 0 succeeds and touches nothing), 1 <= A <= 128.  Bad arguments return non-zero
 * with mms_last_error(NULL) and write nothing. */
int mms_ppo_act(int device, const float* mean, const float* value, const float* log_std, uint64_t seed, int64_t* counters,
                int64_t row_offset, int32_t reference_scale, float* actions_out, float* act_slot, float* logp_slot,
                float* value_slot, float* mu_slot, float* sigma_slot, int64_t N, int32_t A, void* hip_stream);

/* mms_ppo_act with the last Linear layers of both networks folded in.  Actor (module.py:29-30: nn.Linear(pi_hid_sizes[-1],
 * actions)): mean = hidden @ weight^T + bias on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products and sums), then the
 * same sampling and stores; hidden [N,H] f32 is the output of the last activation, weight [A,H] and bias [A] are torch's Linear
 * parameters; H must be a multiple of 64, A <= 128.  Critic (module.py:49: nn.Linear(vf_hid_sizes[-1], 1)) when vhidden is given:
 * value_i = vhidden[i, :] . vweight + vbias[0] (vhidden [N,VH] f32 = output of the critic's last activation, VH a multiple of 4)
 * goes to value_slot and `value` is ignored; vhidden = NULL: `value` [N] (or NULL) is stored as in mms_ppo_act.
 * hidden, weight, vhidden and vweight are read as 16-byte vectors and must be 16-byte aligned (rows then are: H and VH are multiples
 * of 4).  Bad arguments return non-zero with mms_last_error(NULL) and write nothing. */
int mms_ppo_heads_act(int device, const float* hidden, const float* weight, const float* bias, int32_t H, const float* value,
                      const float* vhidden, const float* vweight, const float* vbias, int32_t VH, const float* log_std, uint64_t seed,
                      int64_t* counters, int64_t row_offset, int32_t reference_scale, float* actions_out, float* act_slot,
                      float* logp_slot, float* value_slot, float* mu_slot, float* sigma_slot, int64_t N, int32_t A, void* hip_stream);

/* mms_ppo_heads_act FUSED INTO THE STEP: with a head bound, the next mms_step evaluates the policy's output heads and the sampling tail
 * for its own 16 envs per workgroup in the step kernel's prologue -- the arithmetic of mms_ppo_heads_act, instruction for instruction
 * (csrc/head_block.h is the body of both) -- writes the action / log-prob / value / mu / sigma slots and takes the sampled actions from
 * LDS instead of reading an action tensor: one launch and one memory round trip less per rollout step (pre_physics_step,
 * ten_ant.py:886-891, then consumes what ActorCritic.act, module.py:73-87, would have returned).  The binding holds for ONE step: the
 * step that consumes it clears it (the slot pointers move with every rollout step).  Available where the step kernel runs its 16-envs-
 * per-workgroup TenAnt layout (num_agents 10, num_envs a multiple of 16 and >= 16 per CU, no physical DR) with H a multiple of 512 and
 * A = 80; anywhere else the call fails and the caller launches mms_ppo_heads_act.  Fields as the arguments of mms_ppo_heads_act;
 * actions_out may name the engine's "actions" buffer (kept for task.actions) or be NULL.
 * actions_out = NULL: every other slot is written as usual and the physics follows the sampled actions (what act_slot receives).  What
 * the engine's own "actions" buffer holds after such a step is UNSPECIFIED: the HIP build leaves it as it was (the actions travel through
 * LDS), the CPU build stores the sampled actions there.  A caller that wants them reads act_slot, or hands in actions_out. */
typedef struct mms_policy_head {
    const float* hidden; const float* weight; const float* bias;        /* actor: last hidden activations [N, H], last layer [A, H], [A] */
    const float* vhidden; const float* vweight; const float* vbias;     /* critic: [N, VH], [VH], [1] */
    const float* log_std;                                                /* [A] */
    int64_t* counters;                                                   /* [N] draw counters */
    float* actions_out; float* act_slot; float* logp_slot; float* value_slot; float* mu_slot; float* sigma_slot;
    uint64_t seed;
    int64_t row_offset;
    int32_t H, VH, A, reference_scale;
    const float* weight_tiles;   /* optional (NULL: `weight` is read): the actor's last layer once more, stored [ceil(A / 16)][H / 4][16][4] --
                                  * element ((ct (H / 4) + k / 4) 16 + i) 4 + k % 4 = weight[16 ct + i][k], zero for outputs >= A; 16-byte aligned.
                                  * One operand load of the head's matrix phase then reads 1 KB of contiguous memory (csrc/head_block.h). */
} mms_policy_head;
int mms_bind_policy_head(mms_handle h, const mms_policy_head* head);   /* NULL: unbind */

/* SAC's policy head (algorithms/rl/sac/module.py:23-61, SquashedGaussianMLPActor.forward after `net`) in ONE launch: what torch
 * evaluates as two GEMMs, clamp, exp, randn, fma, tanh, pow, sub, log, sum and a scale.  SAC calls it on every env step for the
 * collection (actor_critic.act, sac.py:166) and for the Q target of every update (pi(o2) under no_grad, sac.py:374-376).
 *   mu_i      = hidden_i @ mu_weight^T + mu_bias;   log_std_i = clamp(hidden_i @ ls_weight^T + ls_bias, -20, 2)   (module.py:31-35)
 *     on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products and sums); hidden [N,H] f32 is the output of `net`'s last
 *     activation, the weights [A,H] and biases [A] are torch's mu_layer / log_std_layer parameters, read in place
 *   u_ij      = mu_ij (deterministic != 0) | mu_ij + exp(log_std_ij) * z_ij (rsample, :41-44)
 *     z_ij ~ N(0,1): counter-based (seed, global row = row_offset + i, counters[i], j) as in mms_ppo_act; counters[i] += 1 in sample
 *     mode; deterministic mode draws nothing and leaves counters alone (counters may then be NULL)
 *   logp_i    = sum_j (-z_ij^2 / 2 - log_std_ij - log(2 pi) / 2 - log(1 - tanh(u_ij)^2 + epsilon))   (:46-52, z = 0 when deterministic)
 *   action_ij = act_limit * tanh(u_ij)                                                                 (:58-59)
 * Destinations (any may be NULL: no store): actions_out / act_slot (e.g. a ReplayBuffer row) / u_slot (pre-squash sample) / mu_slot /
 * log_std_slot (clamped) [N,A], logp_slot [N]; logp_slot == NULL is with_logprob=False and skips the log terms.  H a positive multiple
 * of 64, 1 <= A <= 128, hidden and both weights 16-byte aligned.  Bad arguments return non-zero with mms_last_error(NULL) and write
 * nothing. */
int mms_sac_heads_act(int device, const float* hidden, int32_t H,
                      const float* mu_weight, const float* mu_bias, const float* ls_weight, const float* ls_bias,
                      float act_limit, float epsilon, int32_t deterministic,
                      uint64_t seed, int64_t* counters, int64_t row_offset,
                      float* actions_out, float* act_slot, float* logp_slot,
                      float* u_slot, float* mu_slot, float* log_std_slot,
                      int64_t N, int32_t A, void* hip_stream);

/* The backward of that head's epilogue (csrc/sac_grad_kernels.hip): the gradient of SAC's policy loss (compute_loss_pi, sac.py:392-403)
 * with respect to the OUTPUTS of mu_layer and log_std_layer (the latter before its clamp) and the two bias gradients, from what a
 * mms_sac_heads_act call stored -- what torch autograd evaluates as the mirror image of about fifteen element-wise launches.  The
 * three products behind it (grad_hidden = dy @ [W_mu; W_ls], [gW_mu; gW_ls] = dy^T @ hidden) are left to the caller's GEMM library.
 *   u, mu, log_std [N,A]: the forward's u_slot, mu_slot and log_std_slot (clamped);  grad_action [N,A] or NULL, grad_logp [N] or NULL:
 *   d loss / d (action, logp), at least one of them.  Per element, with L = act_limit, g_a = grad_action_ij or 0, g_l = grad_logp_i or 0:
 *     t = tanh(u);  s = 1 - t^2
 *     G    = L s g_a + g_l 2 t s / (s + epsilon)                 d/du of L tanh(u) and of -log(1 - tanh(u)^2 + epsilon)
 *     dmu  = G
 *     dls  = (-20 < log_std && log_std < 2) ? G (u - mu) - g_l : 0    du/dlog_std = exp(log_std) z = u - mu; the -log_std term of logp
 *   dy [N, 2A]: dmu in columns [0, A), dls in [A, 2A);  dbias [2A] or NULL (not computed): dbias_c = sum_i dy[i, c].
 * There is no `deterministic` flag: a deterministic forward stores u == mu, so G (u - mu) = 0.  The clamp mask is read from the stored,
 * clamped log_std, because the forward clamps exactly to the bound (one measure-zero difference from torch.clamp's gradient: where the
 * layer's raw output EQUALS a bound torch passes the gradient, this gives none).
 * A row of dy depends on that row and the scalars alone, not on N or on where the row sits.  dbias: per-workgroup partials in double
 * in the workspace, then one pass that adds them in a fixed order and rounds once -- no atomics, bit-identical run to run.  At most
 * two launches on hip_stream, no host synchronisation.  16-byte accesses where u, mu, log_std, grad_action and dy are 16-byte aligned
 * (any A), element by element otherwise, with the same results.
 * workspace / ws_bytes: mms_ppo_loss's convention (NULL stores the bytes needed and returns 0 -- nothing else is read; 256-byte aligned;
 * a smaller one is an error; the CPU build needs 0 and runs on any aligned non-NULL workspace).  The workspace needs no initialisation.
 * 0 <= N <= 0x7fffffff (N == 0 succeeds and writes nothing), 1 <= A <= 128.  Inputs are taken to be finite.  Bad arguments -- both
 * gradients NULL, u, mu, log_std or dy NULL, A or N out of range, a small or misaligned workspace -- return non-zero with
 * mms_last_error(NULL) and write nothing. */
int mms_sac_heads_grad(int device, int64_t N, int32_t A, float act_limit, float epsilon,
                       const float* u, const float* mu, const float* log_std,
                       const float* grad_action, const float* grad_logp,
                       float* dy, float* dbias,
                       void* workspace, int64_t* ws_bytes, void* hip_stream);

/* The tail of the off-policy Q target in ONE launch: the last layer of one or two critics (MLPQFunction's Linear(H, 1),
 * algorithms/rl/{ddpg,td3,sac}/module.py `q.q.<last>`), the min of the two and the Bellman backup -- what sac.py:379-382,
 * td3.py:370-373 and ddpg.py:368-369 evaluate under no_grad as two [M,H] x [H,1] products, two bias adds, a min and five
 * element-wise launches.
 *   q_g[i]    = dot(h_g[i, :], w_g) + b_g[0]                            g < G (G = 2 when h1 is given)
 *   qmin[i]   = G == 2 ? min(q_0[i], q_1[i]) : q_0[i]
 *   backup[i] = reward[i] + gamma * (1 - done[i]) * (qmin[i] - alpha * logp[i])     (logp == NULL: no alpha term -- TD3, DDPG)
 * h_g [M,H] f32 is the output of the critic's last hidden activation; w_g [1,H] and b_g [1] are torch's parameters, read in place
 * on every call (the polyak update rewrites the target's after every minibatch, sac.py:354-359).  reward [M] f32, done [M] uint8
 * (ReplayBuffer.dones; non-zero = done), logp [M] f32.  Destinations, any of which may be NULL (no store), at least one given:
 * q0_out, q1_out, backup [M].  backup == NULL is the forward alone: reward, done and logp are not read.  backup needs reward and done.
 * h1 = w1 = b1 = q1_out = NULL runs one network; the second network needs h1, w1 and b1 together.
 * The sum over k has a fixed order that depends on H alone and there are no atomics: q_g[i] is a function of row i and the
 * parameters, not of M or of where the row sits in the call; a done row's backup is reward[i] exactly.  Inputs are taken to be
 * finite: the min is fminf in finite-math code, so a NaN in one critic's output does not propagate as torch.min's would.  Rows past
 * M are neither read nor written.  H a positive multiple of 64 up to MMS_Q_MAX_H (both weight rows are staged in LDS), h_g and w_g
 * 16-byte aligned, M >= 0 (M == 0 succeeds and writes nothing).  Bad arguments return non-zero with mms_last_error(NULL) and
 * write nothing. */
#define MMS_Q_MAX_H 4096
int mms_q_heads_backup(int device, int64_t M, int32_t H,
                       const float* h0, const float* w0, const float* b0, float* q0_out,
                       const float* h1, const float* w1, const float* b1, float* q1_out,      /* all NULL: one network */
                       const float* reward, const uint8_t* done, const float* logp, float gamma, float alpha,
                       float* backup, void* hip_stream);

/* The critics' loss heads WITH a gradient, forward and backward in one streaming pass: the last layer of one or two critics, the
 * loss and everything loss.backward() leaves behind that tail.  Replaces, in the reference's SAC update, compute_loss_q (sac.py:367-389:
 * both critics' Linear(H, 1), two squared-error means and autograd's mirror image) with mode 0, and the critic half of
 * compute_loss_pi (sac.py:392-403: both critics' Linear(H, 1), torch.min, the mean and their backward) with mode 1; one network and
 * mode 0 is TD3's / DDPG's critic loss.  d loss / d q is known the moment q is known, so each [M,H] block is read from memory once.
 *   q_g[i] = mms_q_heads_backup's value for that row, bit for bit (the order of the sum is a function of H alone)
 *   mode 0 (MSE; target [M] required):  e = (double)q_g[i] - (double)target[i]
 *       loss = fp32( sum_g (1/M) sum_i e^2 )                dq_g[i] = scale 2 e / M
 *   mode 1 (policy; target NULL, logp [M] or NULL):  m_i = min_g q_g[i]
 *       loss = fp32( (1/M) sum_i (alpha logp[i] - m_i) )    (logp NULL: no alpha term)
 *       dq_g[i] = -scale/M where q_g is the strict minimum, half of that on a tie (torch.min(a, b)'s rule), 0 otherwise; one network:
 *       dq = -scale/M
 *   dh_g[i,k] = fp32(dq_g[i]) w_g[k] in fp32 (mode 0: one rounding for dq, one for the product);  fp32( dq_g[i] (double)w_g[k] ) (mode 1)
 *   dw_g[k] = fp32( sum_i dq_g[i] (double)h_g[i,k] )        db_g = fp32( sum_i dq_g[i] )
 * dq is a double and stays one in the sums: dw and db carry their own final rounding and the order of the double sum, nothing else
 * (rounded to fp32 first, every term of mode 0 would carry a rounding of its own, and in mode 1 the representation error of 1/M
 * would enter dh, dw and db with one sign).
 * Sums over rows are accumulated in double: per-workgroup partials in the workspace over a partition that is a function of (M, H),
 * added in one finish pass in a fixed order and rounded once.  No atomics, no memset, at most two launches on hip_stream, no host
 * synchronisation: bit-identical run to run, and graph-capturable.  A row's q, dq and dh depend on that row, the parameters and the
 * scalars (M through the stated 1/M), not on where the row sits in the call.
 * Outputs: loss [1] (required); q0_out, q1_out [M]; dh0, dh1 [M,H]; dw_g [H] and db_g [1] as a pair.  Each of q*_out, dh* and the pair
 * may be NULL: not computed (frozen critics in the policy step pass dw = db = NULL), and the others keep their bits.
 * h1 = w1 = b1 = NULL (with q1_out, dh1, dw1, db1 NULL) runs one network.  H a positive multiple of 64 up to MMS_Q_LOSS_MAX_H (a row then
 * fits a quarter wave's registers), h_g, w_g and dh_g 16-byte aligned, 1 <= M <= 0x7fffffff (M == 0 is a bad argument: a mean of
 * nothing has no value).  Rows past M are neither read nor written.  Inputs are taken to be finite.
 * workspace / ws_bytes: mms_sac_heads_grad's convention (NULL stores the bytes needed and returns 0 -- of the arguments only M, H and
 * whether h1 is given are looked at, nothing is dereferenced; 256-byte aligned; a smaller one is an error; the CPU build needs 0 and
 * runs on any aligned non-NULL workspace).  The workspace needs no initialisation.
 * Bad arguments return non-zero with mms_last_error(NULL) and write nothing. */
#define MMS_Q_LOSS_MAX_H 1024
int mms_q_heads_loss(int device, int64_t M, int32_t H,
                     const float* h0, const float* w0, const float* b0,
                     const float* h1, const float* w1, const float* b1,     /* all NULL: one network */
                     int32_t mode, const float* target, const float* logp, float alpha, float scale,
                     float* loss, float* q0_out, float* q1_out,
                     float* dh0, float* dh1, float* dw0, float* db0, float* dw1, float* db1,
                     void* workspace, int64_t* ws_bytes, void* hip_stream);

/* One hidden layer of the PPO policy for BOTH networks in one launch (module.py:27-52: nn.Linear + activation, actor and
 * critic of the same shape): y_g = act(x_g @ w_g^T + b_g), g = 0, 1, on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact
 * fp32 products and sums) with bias and activation in the epilogue.  x [M,K], w [N,K] and b [N] in torch's Linear layout,
 * y [M,N], all f32 and contiguous; K a multiple of 4; act 0 = identity, 1 = ELU(alpha 1) (cfg/ppo/config.yaml:9),
 * 2 = ReLU (the DDPG / TD3 actor, rl/ddpg/module.py:37), 3 = tanh (its output layer, :18).
 * x1 = w1 = b1 = y1 = NULL runs a single problem.  x0 and x1 may be the same buffer (first layer). */
int mms_linear2_act(int device, int64_t M, int32_t N, int32_t K, const float* x0, const float* w0, const float* b0, float* y0,
                    const float* x1, const float* w1, const float* b1, float* y1, int32_t act, void* hip_stream);

/* ---- MAPPO / HAPPO policy inference: every layer of ALL agents' networks per launch ------------------------------------------
 * The reference's collect step (algorithms/marl/runner.py:186-216) calls, agent by agent, policy.get_actions -> Actor.forward
 * (algorithms/marl/actor_critic.py:43-69) and Critic.forward (:137-155): MLPBase (algorithms/utils/mlp.py:38-65) = LayerNorm of
 * the input, then layer_N + 1 blocks of Linear + ELU + LayerNorm (:5-36); ACTLayer / DiagGaussian (utils/act.py:75-81,
 * utils/distributions.py:94-117) = Linear mean head, std = sigmoid(log_std / std_x_coef) * std_y_coef, sample, summed
 * log-probability; v_out = Linear(hidden, 1).  The three operators below run one such stage for up to MMS_MAX_GROUPS networks
 * of the same shape at once (ten actors + ten critics of TenAnt's MAPPO: 20).  The pointer arguments are HOST arrays of
 * `groups` device pointers.  Recurrent policies (use_recurrent_policy: an RNNLayer between MLPBase and the head) take
 * mms_gru_group below between the last block and mms_marl_heads_act. */
#define MMS_MAX_GROUPS 32

/* y_g = act(x_g @ w_g^T + b_g), g < groups: mms_linear2_act for any number of networks (same kernel, same shapes rules).
 * The three ln_* arguments (all NULL: none) fold the LayerNorms on either side of the layer into it, so that the normalised
 * activations are never written (they need act = ELU and M and N multiples of 128):
 *   ln_part_out[g] [N/64, M, 2]: the epilogue also leaves per output row and per 64-column slot the sum and the sum of squares of
 *     the activations; mms_row_stats_group turns them into (mean, rstd) per row.  No atomics: the result does not depend on scheduling.
 *   ln_stat_in[g] [M, 2] + ln_s[g] [N]: x_g is the PRE-LayerNorm activation h and the layer W (LN(h) gamma + beta) + b is evaluated
 *     as rstd (W~ h - mean s) + c: the caller passes W~ = W diag(gamma) as w_g, s = W~ 1 as ln_s[g] and c = W beta + b as b_g.
 * act + 16 asks for blocked summation over k where the shapes take the generic kernel (M or N not a multiple of its tiles): every 32 k
 * are summed from zero and added to the running sum -- 16 + K / 32 roundings of partial sums per output instead of K / 2.  The
 * recurrent policies' layers ask for it (their state carries a layer's error from step to step); elsewhere, and on the tiled fast
 * paths and the LayerNorm folds, results are what they are without it.  The CPU build's dot products are blocked either way. */
int mms_linear_group_act(int device, int32_t groups, int64_t M, int32_t N, int32_t K, const float* const* x, const float* const* w,
                         const float* const* b, float* const* y, int32_t act, const float* const* ln_s, const float* const* ln_stat_in,
                         float* const* ln_part_out, void* hip_stream);

/* ---- MADDPG: the no-gradient tails of all agents' networks per launch --------------------------------------------------------
 * The last layer of up to MMS_MAX_GROUPS deterministic actors (algorithms/marl/maddpg/module.py:36-46, MLPActLayer.forward from the
 * last hidden activation on), the exploration noise of MADDPG_policy.act (:165-175) and the stores, in one launch:
 *   a_g[i,k] = act_limit[g] * tanh(dot(h_g[i,:], w_g[k,:]) + b_g[k])                        g < groups, k < A
 *   sigma > 0:  a_g[i,k] = clamp(a_g[i,k] + sigma * z, -act_limit[g], act_limit[g]),
 *               z ~ N(0,1): counter-based (seed, global row = row_offset + i, counters[i], (agent0 + g) * A + k), the stream of
 *               mms_ppo_act; counters[i] += 1 once per call (behind the draws, on the same stream)
 *   sigma == 0: nothing is drawn, no clamp, counters untouched (may be NULL)
 * h, w, b, act_out: HOST arrays of `groups` device pointers; h_g [M,H] f32 (the output of the last hidden activation), w_g [A,H] and
 * b_g [A] torch's Linear parameters, read in place on every call; act_limit: a HOST array of `groups` floats.  Destinations: act_out
 * (NULL, or per group NULL: no store) -- act_out[g] [M,A] at act_pitch floats per row, e.g. a ring row of agent g's replay buffer --
 * and joint_out (NULL: no store) at joint_pitch floats per row, where agent g's actions go to
 * joint_out[i * joint_pitch + (agent0 + g) * A + k]; every group needs at least one of the two.  agent0 >= 0 lets a caller with more
 * than MMS_MAX_GROUPS agents chunk the call, or refresh one agent's columns with groups = 1.  On the matrix cores
 * (v_mfma_f32_16x16x4_f32: exact fp32 products and sums); the order of the sum over k is a function of H and A alone and there are
 * no atomics: with sigma = 0, a_g[i,:] is a function of row i and network g's parameters only, not of M, groups, agent0, the pitches
 * or where the row sits.  H a positive multiple of 64, 1 <= A <= 128, h_g and w_g 16-byte aligned, act_pitch >= A (when act_out is
 * given), joint_pitch >= (agent0 + groups) * A (when joint_out is given), M >= 0 (M == 0 succeeds and touches nothing).  Rows past M
 * and columns past A are never written.  Bad arguments return non-zero with mms_last_error(NULL) and write nothing. */
int mms_det_heads_act_group(int device, int32_t groups, int64_t M, int32_t H, int32_t A, int32_t agent0,
                            const float* const* h, const float* const* w, const float* const* b, const float* act_limit,
                            float sigma, uint64_t seed, int64_t* counters, int64_t row_offset,
                            float* const* act_out, int64_t act_pitch, float* joint_out, int64_t joint_pitch, void* hip_stream);

/* The last layer of ONE deterministic actor (algorithms/rl/{ddpg,td3}/module.py MLPActor, from its last hidden activation on), with
 * what DDPG's and TD3's updates put behind it, in one launch plus at most one counter launch:
 *   t[i,k] = tanh(dot(h[i,:], w[k,:]) + b[k])                    h [M,H], w [A,H], b [A]: torch's parameters, read in place
 *   a[i,k] = act_limit * t[i,k]
 *   sigma > 0:  e = sigma * z,  z ~ N(0,1): counter-based (seed, global row = row_offset + i, counters[i], k), mms_ppo_act's stream
 *               noise_clip finite and >= 0:  e = min(max(e, -noise_clip), noise_clip)        (td3.py:362-364 target policy smoothing)
 *               a = min(max(a + e, -act_limit), act_limit);  counters[i] += 1 once per call (behind the draws, on the same stream)
 *   sigma == 0: nothing is drawn, no clamp, counters untouched (may be NULL)
 * noise_clip negative or +inf: no noise clip (MLPActorCritic.act's exploration noise).  Destinations, each optional, at least one:
 * act_out [M,A] at act_pitch floats per row (a pitch of W + A writes the action into the action columns of a [o | a] block), and
 * tanh_out [M,A] dense: t as computed BEFORE any noise -- what mms_det_heads_grad reads.
 * This is mms_det_heads_act_group's kernel with one group: with sigma == 0, or sigma > 0 without a noise clip, act_out holds bit for
 * bit what that entry gives with groups = 1, agent0 = 0; the order of the sum over k is a function of H and A alone, no atomics, and
 * a row's result depends on that row and the parameters only.  H a positive multiple of 64, 1 <= A <= 128, h and w 16-byte aligned,
 * act_pitch >= A (when act_out is given), M >= 0 (M == 0 succeeds and touches nothing).  Rows past M and columns past A are never
 * written.  Bad arguments return non-zero with mms_last_error(NULL) and write nothing. */
int mms_det_heads_act(int device, int64_t M, int32_t H, int32_t A, const float* h, const float* w, const float* b, float act_limit,
                      float sigma, float noise_clip, uint64_t seed, int64_t* counters, int64_t row_offset,
                      float* act_out, int64_t act_pitch, float* tanh_out, void* hip_stream);

/* The backward of that head's epilogue (csrc/det_head_kernels.hip), on mms_sac_heads_grad's pattern: the gradient with respect to the
 * OUTPUT of the actor's last Linear, and its bias gradient, from the forward's tanh_out.
 *   dy[i,k]  = (act_limit * g[i,k]) * (1 - t[i,k]^2)       g = d loss / d action, [N,A] at grad_pitch floats per row (>= A)
 *   dbias[k] = sum_i dy[i,k]                               dbias NULL: not computed
 * t [N,A] and dy [N,A] are dense.  grad_pitch lets g be the action columns of the critic's input gradient [N, W + A], read where they
 * lie.  The two products behind it (grad_hidden = dy @ W, grad_W = dy^T @ hidden) are left to the caller's GEMM library.
 * Every product and difference is rounded on its own (no contraction): dy has the same bits in the HIP and the CPU build.  A row of
 * dy depends on that row and act_limit alone.  dbias: per-workgroup partials in double in the workspace, then one pass that adds them
 * in a fixed order and rounds once -- no atomics, no memset, bit-identical run to run.  At most two launches on hip_stream, no host
 * synchronisation, graph-capturable.  16-byte accesses of t and dy where both are 16-byte aligned (any A), of g where in addition g is
 * 16-byte aligned and A and grad_pitch are multiples of 4; element by element otherwise, with the same results.
 * workspace / ws_bytes: mms_sac_heads_grad's convention (NULL stores the bytes needed and returns 0 -- nothing else is read; 256-byte
 * aligned; a smaller one is an error; the CPU build needs 0 and runs on any aligned non-NULL workspace).  No initialisation needed.
 * 0 <= N <= 0x7fffffff (N == 0 succeeds and writes nothing), 1 <= A <= 128.  Inputs are taken to be finite.  Bad arguments -- t, g
 * or dy NULL, grad_pitch below A, A or N out of range, a small or misaligned workspace -- return non-zero with mms_last_error(NULL)
 * and write nothing. */
int mms_det_heads_grad(int device, int64_t N, int32_t A, float act_limit, const float* t, const float* g, int64_t grad_pitch,
                       float* dy, float* dbias, void* workspace, int64_t* ws_bytes, void* hip_stream);

/* mms_q_heads_backup with ONE critic per group for up to MMS_MAX_GROUPS groups in one launch (cal_value_loss, module.py:218-219):
 *   q_g[i]      = dot(h_g[i,:], w_g) + b_g[0]
 *   backup_g[i] = reward_g[i] + gamma * (1 - done_g[i]) * q_g[i]
 * h, w, b, q_out, reward, done, backup: HOST arrays of `groups` device pointers (q_out, reward, done, backup may be NULL as a
 * whole); q_out[g] and backup[g] may be NULL per group with at least one destination overall; backup[g] needs reward[g] and done[g]
 * (uint8).  The limits of the ungrouped entry (H a positive multiple of 64 up to MMS_Q_MAX_H, h_g and w_g 16-byte aligned, M >= 0).
 * Per group the results are bit-identical to mms_q_heads_backup called for that network alone (one network, logp NULL). */
int mms_q_heads_backup_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* h, const float* const* w,
                             const float* const* b, float* const* q_out, const float* const* reward, const uint8_t* const* done,
                             float gamma, float* const* backup, void* hip_stream);

/* stat_g[r] = (mean, 1 / sqrt(var + eps)) of row r from the `slots` partial (sum, sum of squares) pairs of mms_linear_group_act's
 * ln_part_out (width = that layer's N; biased variance, as nn.LayerNorm). */
int mms_row_stats_group(int device, int32_t groups, int64_t M, int32_t slots, int32_t width, const float* const* part, float* const* stat,
                        float eps, void* hip_stream);

/* stat_g[r] = (mean, 1 / sqrt(var + eps)) of row r of x_g [M, K] (row pitch x_pitch floats, 0 = K; K <= 4096): the statistics of a
 * LayerNorm whose normalised output is never needed because the layer behind it takes them through ln_stat_in -- the feature
 * LayerNorm of the centralised observation, which every critic of an env shares. */
int mms_row_moments_group(int device, int32_t groups, int64_t M, int32_t K, int32_t x_pitch, const float* const* x, float* const* stat,
                          float eps, void* hip_stream);

/* nn.LayerNorm over the last dimension (biased variance, eps inside the root): y_g[r, 0:K] = LN(x_g[r, 0:K]) * gamma_g + beta_g,
 * y_g[r, K:Kp] = 0.  x rows have pitch x_pitch floats (0 = K; A * K reads one agent's rows of an [N, A, K] block where they lie),
 * y rows pitch Kp >= K (Kp > K pads a 46-wide observation to the multiple of 4 the layer kernel wants); y_g == x_g with
 * Kp == x_pitch == K is the in-place form.  K <= 4096 (the 100-ant swarm's centralised observation is 3808 wide). */
int mms_layernorm_group(int device, int32_t groups, int64_t M, int32_t K, int32_t Kp, int32_t x_pitch, const float* const* x,
                        const float* const* gamma, const float* const* beta, float* const* y, float eps, void* hip_stream);

/* (eps < 0: no LayerNorm -- the plain output layer on h_g; gamma / beta are not read by either build: the arrays, or
 *  entries of them, may be NULL.  eps >= 0: gamma[g] and beta[g] are [H] each and required.)
 * The last LayerNorm + the output layer (+ the Gaussian sample) of each network: out_g[r, j] = b_g[j] + sum_k w_g[j, k] *
 * LN(h_g[r])[k], j < A[g] <= 16, H <= 1024.  std[g] != NULL ([A[g]] standard deviations): out_g = that mean + std z with z ~ N(0,1)
 * from the counter-based stream keyed (seed + g, row_offset + r, counters[g][r], j) (counters[g][r] += 1; counters or counters[g]
 * NULL: counter 0), and logp[g][r, j] = log N(out_j | mean_j, std_j), PER DIMENSION, [M, A[g]] (FixedNormal.log_probs,
 * distributions.py:31-34, does not sum over the action dimensions).  std == NULL or
 * std[g] == NULL: out_g is the plain output (the critic's value; a deterministic action).  out_pitch[g] (NULL: A[g]) = floats
 * between consecutive rows of out_g and logp_g, so that agent k's actions land in an [N, agents, A] rollout slot directly.  The noise stream is this build's, not
 * torch's Philox: sampled actions differ from the reference's draw for the same torch seed, their distribution does not. */
int mms_marl_heads_act(int device, int32_t groups, int64_t M, int32_t H, const float* const* h, const float* const* gamma,
                       const float* const* beta, const float* const* w, const float* const* b, const int32_t* A, const float* const* std,
                       float* const* out, float* const* logp, const int32_t* out_pitch, int64_t* const* counters, uint64_t seed,
                       int64_t row_offset, float eps, void* hip_stream);

/* mms_marl_heads_act's front with the actions GIVEN: the tail of Actor.evaluate_actions (algorithms/utils/act.py evaluate_actions on
 * a Box space; FixedNormal.log_probs, distributions.py:31-34) and the product that the Runner's train() forms from two such passes per
 * agent (runner.py:282-313: factor *= prod_j exp(new_logp - old_logp)), in one launch for up to MMS_MAX_GROUPS networks.  h, gamma,
 * beta, eps, w, b, A as in mms_marl_heads_act (H <= 1024, A[g] <= 16; eps < 0: no LayerNorm, gamma / beta not read); std[g] [A[g]] and
 * act[g] [M, A[g]] (row pitch act_pitch[g] floats) are required.  With mean_j = b_g[j] + sum_k w_g[j, k] LN(h_g[r])[k]:
 *   logp_g[r, j]    = log N(act_g[r, j] | mean_j, std_g[j])                 PER DIMENSION, [M, A[g]] at pitch logp_pitch[g]; not summed.
 *                                                                            logp == NULL or logp[g] == NULL: not stored.
 *   factor_out_g[r] = factor_in_g[r] * exp(sum_j (logp_g[r, j] - old_logp_g[r, j]))
 *                                                                            where factor_out[g] != NULL; old_logp[g] ([M, A[g]] at pitch
 *                                                                            old_pitch[g]) is then required; factor_in == NULL or
 *                                                                            factor_in[g] == NULL stands for 1; factor_out[g] ==
 *                                                                            factor_in[g] is the in-place form.  [M] floats each.
 * Everything between the fp32 inputs and the two outputs is double (csrc/marl_eval_lane.h, one arithmetic for both builds): the
 * LayerNorm, the head's sums over H, the log-density -- logp is one rounding of it --, the sum over ascending j of the differences
 * between the fp32 values logp_g[r, j] that are (or would be) stored and old_logp_g[r, j], and the exp, with one rounding to fp32 at
 * the product: the factor's bits do not depend on whether logp is stored, and with old_logp written by this entry from parameters that
 * have not moved since, factor_out is factor_in bit for bit.  A pitch array that is NULL stands for A[g].  No atomics; a row's results are a function of that row and network g's
 * parameters only, not of M, groups or where the row sits.  logp[g] must not be act[g] or old_logp[g].  M >= 0 (M == 0 succeeds and
 * touches nothing); groups 1..MMS_MAX_GROUPS.  One launch on hip_stream, no host synchronisation.  Bad arguments (A[g] > 16, H > 1024,
 * groups out of range, a required pointer NULL, a pitch below A[g], factor_out without old_logp) return non-zero with
 * mms_last_error(NULL) and write nothing. */
int mms_marl_heads_eval(int device, int32_t groups, int64_t M, int32_t H, const float* const* h, const float* const* gamma,
                        const float* const* beta, const float* const* w, const float* const* b, const int32_t* A, const float* const* std,
                        const float* const* act, const int32_t* act_pitch, float* const* logp, const int32_t* logp_pitch,
                        const float* const* old_logp, const int32_t* old_pitch, const float* const* factor_in, float* const* factor_out,
                        float eps, void* hip_stream);

/* One GRU cell step for up to MMS_MAX_GROUPS networks in one launch: one layer of the reference's RNNLayer in its single-step
 * branch (algorithms/utils/rnn.py:25-29: nn.GRU on hxs * masks; built into every recurrent actor and critic at
 * algorithms/marl/actor_critic.py:35-36, 64-65, 139-140, 164-165 and run agent by agent from runner.py:205-217).  With torch's
 * parameters as they lie (gate order r, z, n): w_ih [3H, K], w_hh [3H, H], b_ih [3H], b_hh [3H], for g < groups and i < M:
 *   hm = mask_g[i] * h_g[i, :]                            (mask == NULL: hm = h_g[i, :])
 *   r  = sigmoid(x W_ir^T + b_ir + hm W_hr^T + b_hr)
 *   z  = sigmoid(x W_iz^T + b_iz + hm W_hz^T + b_hz)
 *   n  = tanh   (x W_in^T + b_in + r * (hm W_hn^T + b_hn))
 *   h' = (1 - z) * n + z * hm
 * x, h, mask, w_ih, w_hh, b_ih, b_hh, h_out, y: HOST arrays of `groups` device pointers; pitches in floats.  x_g [M, K] at x_pitch;
 * h_g [M, H] at h_pitch, so that layer l of an [M, recurrent_N, H] state slot (or of agent k's part of an [N, agents, recurrent_N,
 * H] slot) is read where it lies; mask_g [M] at mask_pitch (NULL as a whole: no mask); h_out_g [M, H] at h_out_pitch receives h',
 * e.g. in the next step's slot; y (NULL as a whole, or per group) is a second, dense [M, H] destination of the same h' -- the next
 * GRU layer's x and the head's input.  The mask multiplies h as the reference does it (0 * NaN = NaN); a row with mask 0 is bit for
 * bit the row of a zero state.
 * On the matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products and sums); the [M, 3H] pre-activations stay in accumulators.  The
 * order of every sum over k is a function of K and H alone and there are no atomics: h'_g[i, :] is a function of row i and network
 * g's parameters only, not of M, groups, the pitches or where the row sits, and runs are bit-identical.
 * K and H positive multiples of 4, H <= 1024; x_pitch >= K, h_pitch >= H, h_out_pitch >= H, each a multiple of 4; mask_pitch >= 1;
 * x_g, h_g, w_ih_g, w_hh_g, h_out_g, y_g 16-byte aligned; M >= 0 (M == 0 succeeds and touches nothing).  No destination may be one
 * of the sources (other workgroups still read those rows): h_out_g == h_q or x_q, y_g == h_q, x_q or h_out_q, or two groups with one
 * destination are refused.  Rows past M and columns past H are never written.  Bad arguments return non-zero with
 * mms_last_error(NULL) and write nothing. */
int mms_gru_group(int device, int32_t groups, int64_t M, int32_t K, int32_t H, const float* const* x, int64_t x_pitch,
                  const float* const* h, int64_t h_pitch, const float* const* mask, int64_t mask_pitch, const float* const* w_ih,
                  const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, float* const* h_out,
                  int64_t h_out_pitch, float* const* y, void* hip_stream);

/* The gate arithmetic of the same cell step on pre-activations that layer launches left in memory: the unfused form of mms_gru_group,
 * for callers that run the two products x W_ih^T and h W_hh^T on another kernel (GroupedPolicyInference's rnn_format="f16x2" runs them
 * on mms_linear_group_act_split16, N = 3H, identity activation, out_mode 0).  For g < groups, i < M, j < H, gate order r, z, n:
 *   gi_g [M, 3H] at g_pitch = x W_ih^T + b_ih, the bias already added; gh_g [M, 3H] at g_pitch = h W_hh^T of the UNMASKED state, no bias
 *   hm  = mask_g[i] * h_g[i, j]                                  (mask == NULL: hm = h)
 *   a_* = mask_g[i] * gh_g[i, * H + j] + b_hh_g[* H + j]         ((m h) W^T = m (h W^T) for a per-row 0 / 1 mask)
 *   r = sigmoid(gi_r + a_r);  z = sigmoid(gi_z + a_z);  n = tanh(gi_n + r * a_n);  h' = (1 - z) * n + z * hm
 * h' goes to h_out_g[i, j] (at h_out_pitch) and, where given, to y_g[i, j] (dense [M, H]; y NULL as a whole or per group).  gi, gh, h,
 * mask, b_hh, h_out, y: HOST arrays of `groups` device pointers; pitches in floats.  Both products of the mask are followed by + 0, so a
 * row with mask 0 is bit for bit the row of a zero state with zero gh.  A streaming kernel without atomics: h'_g[i, :] is a function of
 * row i and the group's b_hh only, not of M, groups, the pitches or where the row sits, and runs are bit-identical.
 * H a positive multiple of 4 up to 1024; g_pitch >= 3H, h_pitch >= H, h_out_pitch >= H, each a multiple of 4; mask_pitch >= 1; gi_g,
 * gh_g, h_g, b_hh_g, h_out_g, y_g 16-byte aligned; M >= 0 (M == 0 succeeds and touches nothing); groups 1..MMS_MAX_GROUPS.  No
 * destination may be one of the sources: h_out_g == h_q, gi_q or gh_q, y_g == h_q, gi_q, gh_q or h_out_q, or two groups with one
 * destination are refused.  Rows past M, columns past H and whatever lies between pitched rows are never written.  Bad arguments return
 * non-zero with mms_last_error(NULL) and write nothing. */
int mms_gru_gates_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* gi, const float* const* gh, int64_t g_pitch,
                        const float* const* h, int64_t h_pitch, const float* const* mask, int64_t mask_pitch,
                        const float* const* b_hh, float* const* h_out, int64_t h_out_pitch, float* const* y, void* hip_stream);

/* The backward of mms_gru_gates_group for up to MMS_MAX_GROUPS networks per call (csrc/gru_grad_kernels.hip): what a GRU's backward
 * through time does per step besides its matrix products, which stay with the caller's library (algorithms/marl/rnn_seq.py runs the
 * actor and the critic of one agent as the two groups).  gi, gh (g_pitch), h (h_pitch), mask (mask_pitch), b_hh: the forward's inputs
 * with the forward's meaning; r, z, n are recomputed by the forward's statements and are bit for bit the forward's.  dh_out_g [M, H] at
 * dh_out_pitch is d loss / d h'; dy_g [M, H] at dy_pitch (NULL as a whole or per group) a second gradient of the same h' (the forward's
 * y); G = dh_out + dy, one fp32 addition (dy NULL: G = dh_out).  For g < groups, i < M, j < H, with m = mask_g[i] (NULL: 1):
 *   hm = m h;  a_* = m gh_* + b_hh_*;  r, z, n as in mms_gru_gates_group
 *   dpn = G (1 - z) (1 - n^2)          dpz = G (hm - n) z (1 - z)          dpr = dpn a_n r (1 - r)
 *   dgi_g[i] = [dpr | dpz | dpn]       dgh_g[i] = m [dpr | dpz | r dpn] + 0          (each [M, 3H] at dg_pitch)
 *   dh_g[i]  = m (G z) + 0             ([M, H] at dh_pitch: the direct path only)
 *   dbias_g  = the column sums over the M rows of [dpr | dpz | dpn | r dpn], NOT multiplied by m    ([4H]; NULL as a whole or per group:
 *              not computed)
 * The caller completes the step: dh_{t-1} = dh + dgh W_hh, db_ih = dbias[0:3H], db_hh = dbias[0:2H] | dbias[3H:4H].  The + 0 makes a
 * row with mask 0 have dgh and dh of +0 bit for bit, and mask == NULL a mask of ones bit for bit.
 * dgi, dgh and dh of row i are a function of row i and the group's b_hh alone.  dbias: per-workgroup partials in double in the
 * workspace over a partition of the rows that is a function of (M, H), one finish pass in a fixed order, rounded once, no atomics --
 * bit-identical run to run and independent of `groups`.
 * Workspace as for mms_ppo_loss: workspace == NULL stores the bytes needed (a function of groups, M and H; the CPU build: 0) in
 * *ws_bytes and returns 0 without reading anything else; otherwise 256-byte aligned with *ws_bytes at least that.  At most two launches
 * on hip_stream, no host synchronisation; the pointer tables travel in the kernel arguments.
 * H, M, groups, pitches (dg_pitch as g_pitch; dh_out_pitch, dy_pitch, dh_pitch as h_pitch) and alignments (dgi_g, dgh_g, dh_g, dh_out_g,
 * dy_g 16 bytes; dbias_g 4): the rules of mms_gru_gates_group.  No destination (dgi_g, dgh_g, dh_g, dbias_g) may be a source (gi_q,
 * gh_q, h_q, mask_q, b_hh_q, dh_out_q, dy_q) or another destination of any group: refused -- callers ping-pong two dh buffers.  Rows
 * past M, columns past the views and whatever lies between pitched rows are never written; M == 0 succeeds and writes nothing.  Bad
 * arguments return non-zero with mms_last_error(NULL) and write nothing. */
int mms_gru_gates_grad_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* gi, const float* const* gh, int64_t g_pitch,
                             const float* const* h, int64_t h_pitch, const float* const* mask, int64_t mask_pitch,
                             const float* const* b_hh, const float* const* dh_out, int64_t dh_out_pitch, const float* const* dy,
                             int64_t dy_pitch, float* const* dgi, float* const* dgh, int64_t dg_pitch, float* const* dh, int64_t dh_pitch,
                             float* const* dbias, void* workspace, int64_t* ws_bytes, void* hip_stream);

/* ---- the `Linear + ELU + LayerNorm` blocks of the MAPPO / HAPPO networks in an update (csrc/elu_ln_kernels.hip) --------------------
 * What one block of MLPLayer (agents/algorithms/utils/mlp.py:19-27) does behind its matrix product, for up to MMS_MAX_GROUPS networks
 * of one width per call (algorithms/marl/blocks.py runs the actor and the critic of one agent as the two groups); the products stay with
 * the caller's library.  z_g [M, H] at z_pitch is the bias-free product x W^T.  For g < groups, i < M, j < H (csrc/elu_ln_lane.h):
 *   u = z_g[i, j] + bias_g[j];  a = u > 0 ? u : expm1f(u)                                (ELU, alpha = 1; fp32, as torch holds them)
 *   mean = sum_j(a) / H;  var = sum_j((a - mean)^2) / H  (two-pass, biased, as nn.LayerNorm);  rstd = 1 / sqrt(var + eps)
 *   y_g[i, j] = (a - mean) rstd gamma_g[j] + beta_g[j]   ([M, H] at y_pitch);   stat_g[i] = (mean, rstd)   ([M, 2], dense)
 * What is stored (mean, rstd, y) is fp32; what lies between two stored values (the sums, var, (a - mean) rstd) is formed in double from
 * the fp32 values and rounded once; var and y use the stored, rounded mean and rstd, which is what the backward reads.
 * z, bias, gamma, beta, y, stat: HOST arrays of `groups` device pointers; pitches in floats.  A streaming kernel without atomics; the
 * order of a row's sums is a function of H alone, so y_g[i, :] and stat_g[i] are a function of row i and the group's parameters only,
 * not of M, groups, the pitches or where the row sits, and runs are bit-identical.
 * H a positive multiple of 4 up to 1024; z_pitch, y_pitch >= H and multiples of 4; z_g, bias_g, gamma_g, beta_g, y_g 16-byte aligned,
 * stat_g 8; eps >= 0; M >= 0 (M == 0 succeeds and touches nothing); groups 1..MMS_MAX_GROUPS.  No destination (y_g, stat_g) may be a
 * source or another destination of any group.  Rows past M, columns past H and whatever lies between pitched rows are never written.
 * One launch on hip_stream, no host synchronisation.  Bad arguments return non-zero with mms_last_error(NULL) and write nothing. */
int mms_elu_ln_group(int device, int32_t groups, int64_t M, int32_t H, float eps, const float* const* z, int64_t z_pitch,
                     const float* const* bias, const float* const* gamma, const float* const* beta, float* const* y, int64_t y_pitch,
                     float* const* stat, void* hip_stream);

/* mms_elu_ln_group that leaves y_g in both forms: as fp32 (what the backward's library products read) and as the H32 operand planes of
 * mms_linear_group_act_split16 (below), which then multiplies the next block without a pass that re-reads and re-writes [M, H].
 * z .. stat: exactly mms_elu_ln_group's arguments, and y_g, stat_g are bit for bit what it writes.  planes, scale, inv: HOST arrays of
 * `groups` device pointers; planes_g receives the H32 split of y_g [M, H] (MMS_H32_BYTES(M, H) bytes, the columns from H to the next
 * multiple of 32 written as zero), scale_g [M] the rows' powers of two (from the row's own largest |y|; an all-zero row keeps 1) and
 * inv_g [M] their inverses (entries of these two arrays may be NULL).  All three are byte for byte what
 *   mms_split_planes16_group(device, groups, M, H, y_pitch, y, planes, scale, inv, 0, 0, NULL, NULL, NULL, NULL, eps, stream)
 * writes when it is run on that y.  The kernel is mms_elu_ln_group's with one more reduction over the row (a maximum: exact in any
 * order) while a thread still holds its four y: no further read of [M, H], 4 more bytes written per element and 8 per row.
 * H, pitches, alignments, M, groups: mms_elu_ln_group's rules; planes_g 16-byte aligned, scale_g and inv_g 4.  No destination (y_g,
 * stat_g, planes_g, scale_g, inv_g) may be a source or another destination of any group.  Rows past M are never written; M == 0
 * succeeds and touches nothing.  One launch on hip_stream, no atomics, no host synchronisation, the pointer tables in the kernel
 * arguments; a row's outputs are a function of that row and the group's parameters alone.  Bad arguments return non-zero with
 * mms_last_error(NULL) and write nothing. */
int mms_elu_ln_planes16_group(int device, int32_t groups, int64_t M, int32_t H, float eps, const float* const* z, int64_t z_pitch,
                              const float* const* bias, const float* const* gamma, const float* const* beta, float* const* y, int64_t y_pitch,
                              float* const* stat, void* const* planes, float* const* scale, float* const* inv, void* hip_stream);

/* The backward of mms_elu_ln_group.  z (z_pitch), bias, gamma: the forward's inputs; stat: the forward's output; u, a and
 * xhat = (a - mean) rstd are recomputed from them by the forward's statements and are bit for bit the forward's.  dy_g [M, H] at
 * dy_pitch is d loss / d y.  For g < groups, i < M, j < H:
 *   q = dy gamma;  c1 = sum_j(q) / H;  c2 = sum_j(q xhat) / H                          (in double, as xhat)
 *   da = rstd (q - c1 - xhat c2);  dz_g[i, j] = da (u > 0 ? 1 : a + 1), rounded once     ([M, H] at dz_pitch)
 *   dparams_g = the column sums over the M rows of [dz | dy xhat | dy] = [dbias | dgamma | dbeta]   ([3H]; NULL as a whole or per
 *               group: not computed)
 * The caller completes the block: dW = dz^T x, dx = dz W.  dz_g[i, :] is a function of row i and the group's parameters alone.
 * dparams: per-workgroup partials in double in the workspace over a partition of the rows that is a function of (M, H), one finish
 * pass in a fixed order, rounded once, no atomics -- bit-identical run to run and independent of `groups`.  M == 0 succeeds and
 * writes zeros into every dparams_g, nothing else.
 * Workspace as for mms_gru_gates_grad_group: workspace == NULL stores the bytes needed (a function of groups, M and H; the CPU build:
 * 0) in *ws_bytes and returns 0 without reading anything else; otherwise 256-byte aligned with *ws_bytes at least that.  At most two
 * launches on hip_stream, no memset, no host synchronisation; the pointer tables travel in the kernel arguments.
 * H, M, groups, pitches and alignments: the rules of mms_elu_ln_group (dy_g, dz_g 16 bytes, dparams_g 4).  No destination (dz_g,
 * dparams_g) may be a source (z_q, bias_q, gamma_q, stat_q, dy_q) or another destination of any group.  Rows past M, columns past H
 * and whatever lies between pitched rows are never written.  Bad arguments return non-zero with mms_last_error(NULL) and write
 * nothing. */
int mms_elu_ln_grad_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* z, int64_t z_pitch,
                          const float* const* bias, const float* const* gamma, const float* const* stat, const float* const* dy,
                          int64_t dy_pitch, float* const* dz, int64_t dz_pitch, float* const* dparams, void* workspace,
                          int64_t* ws_bytes, void* hip_stream);

/* ---- the output heads of the MAPPO / HAPPO networks in an update, forward and backward (csrc/marl_heads_grad_kernels.hip) ----------
 * DiagGaussian.fc_mean = Linear(H, A) with std = sigmoid(log_std / std_x_coef) std_y_coef (agents/algorithms/utils/distributions.py)
 * and Critic.v_out = Linear(H, 1), for up to MMS_MAX_GROUPS networks per call (algorithms/marl/heads.py).  Network g is
 * (f_g [M, H] at f_pitch, w_g [A[g], H], b_g [A[g]]) with A[g] in 1..16; a critic is the A = 1 case.  For g < groups, r < M, j < A[g]:
 *   out_g[r, j] = b_g[j] + sum_k w_g[j, k] f_g[r, k]                                     ([M, A[g]], dense)
 *   std_g[j] = sigmoid(log_std_g[j] / x_coef) y_coef                                     (where log_std_g != NULL; [A[g]])
 * Arithmetic (csrc/marl_heads_grad_lane.h): every product is formed in double from the fp32 values (exact), every sum is accumulated
 * in double and rounded to fp32 once, behind the bias; std in double, rounded once.  The order of a row's sum is a function of H
 * alone, so out_g[r, :] is a function of row r and of network g's parameters only, not of M, groups or where the row sits.
 * f, w, b, log_std, out, std: HOST arrays of `groups` device pointers (log_std and std may be NULL as a whole, log_std per entry);
 * A: HOST array; pitches in floats.  H a positive multiple of 4 up to 1024; f_pitch >= H and a multiple of 4; f_g, w_g 16-byte
 * aligned; M >= 0 (M == 0 writes std only); groups 1..MMS_MAX_GROUPS.  No destination (out_g, std_g) may be a source or another
 * destination of any group.  One launch on hip_stream, no atomics, no host synchronisation, the pointer tables in the kernel
 * arguments.  Bad arguments return non-zero with mms_last_error(NULL) and write nothing. */
int mms_marl_heads_fwd_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* f, int64_t f_pitch,
                             const float* const* w, const float* const* b, const int32_t* A, const float* const* log_std, float x_coef,
                             float y_coef, float* const* out, float* const* std, void* hip_stream);

/* The backward of mms_marl_heads_fwd_group.  dout_g [M, A[g]] (dense) is d loss / d out_g, dstd_g [A[g]] is d loss / d std_g:
 *   df_g[r, k] = sum_j dout_g[r, j] w_g[j, k], j ascending                                ([M, H] at df_pitch)
 *   dw_g[j, k] = sum_r dout_g[r, j] f_g[r, k];   db_g[j] = sum_r dout_g[r, j]             ([A[g], H], [A[g]])
 *   dlog_std_g[j] = dstd_g[j] y_coef s (1 - s) / x_coef,  s = sigmoid(log_std_g[j] / x_coef)
 * with the forward's arithmetic: products and sums in double, one rounding.  df, dw with db, and dlog_std may each be NULL as a whole
 * or per group (dw_g and db_g together): what is NULL is not computed and the other outputs keep their bits.  df_g[r, :] is a function
 * of row r and w_g alone.  dw, db: per-workgroup partials in double in the workspace over a partition of the rows that is a function
 * of (M, H), one finish pass in a fixed order, rounded once, no atomics -- bit-identical run to run and independent of `groups`: group
 * g's outputs are bit for bit those of a call with groups = 1 on its arguments.  M == 0 succeeds and writes zeros into dw_g and db_g
 * (and dlog_std_g), nothing else.
 * Workspace as for mms_elu_ln_grad_group: workspace == NULL stores the bytes needed (a function of groups, M, H and A; the CPU build:
 * 0) in *ws_bytes and returns 0 without reading anything but A; otherwise 256-byte aligned with *ws_bytes at least that.  At most two
 * launches on hip_stream, no memset, no host synchronisation; the pointer tables travel in the kernel arguments.
 * H, M, groups, A, f_pitch: the forward's rules; df_pitch >= H and a multiple of 4; f_g, w_g, df_g 16-byte aligned.  No destination
 * (df_g, dw_g, db_g, dlog_std_g) may be a source (f_q, w_q, dout_q, log_std_q, dstd_q) or another destination of any group.  Rows past
 * M and whatever lies between pitched rows are never written.  Bad arguments return non-zero with mms_last_error(NULL) and write
 * nothing. */
int mms_marl_heads_grad_group(int device, int32_t groups, int64_t M, int32_t H, const float* const* f, int64_t f_pitch,
                              const float* const* w, const int32_t* A, const float* const* dout, const float* const* log_std,
                              const float* const* dstd, float x_coef, float y_coef, float* const* df, int64_t df_pitch,
                              float* const* dw, float* const* db, float* const* dlog_std, void* workspace, int64_t* ws_bytes,
                              void* hip_stream);

/* ---- the same layers on the bf16 matrix pipe with fp32 operands carried as three bf16 planes (csrc/split_kernels.hip) -----------
 * An fp32 number is exactly a0 + a1 + a2 with a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1); the product is formed as the six
 * bf16 MFMA products a0 b0 + a0 b1 + a1 b0 + a1 b1 + a0 b2 + a2 b0 with fp32 accumulation (the dropped terms are < 2^-25 |a b|): the fp32
 * product of module.py:27-52 at 16 / 6 of the fp32 MFMA rate, with an error against the float64 product that is not larger than the
 * exact-fp32 MFMA kernel's (tests/test_gpu_parity.py measures both on the same inputs).
 * Plane format "P32": bf16 [rows, KC, 3, 32], KC = ceil(K / 32): per row and per 32 consecutive k the three planes, 192 contiguous bytes;
 * columns past K are zero.  MMS_P32_BYTES(rows, K) bytes. */
#define MMS_P32_BYTES(rows, K) ((size_t)(rows) * (size_t)(((K) + 31) / 32) * 192)

/* planes <- split(x): x [rows, K] f32 with row pitch x_pitch floats (0 = K; rows 16-byte aligned).  Weights once per optimizer step,
 * the observation once per env step; hidden activations are left in P32 by the layer that produces them (out_planes below). */
int mms_split_planes(int device, int64_t rows, int32_t K, int32_t x_pitch, const float* x, void* planes, void* hip_stream);

/* The same for `groups` matrices of one shape in one launch (x and planes: HOST arrays of device pointers).  Rows need not be 16-byte
 * aligned here (agent k's rows of an [M, agents, 46] observation block): unaligned sources take scalar loads. */
int mms_split_planes_group(int device, int32_t groups, int64_t rows, int32_t K, int32_t x_pitch, const float* const* x, void* const* planes,
                           void* hip_stream);

/* y_g = act(x_g @ w_g^T + b_g), g < groups, as mms_linear_group_act, with x_g [M, K] and w_g [N, K] given as P32 planes and b_g [N] f32.
 * M and N multiples of 128.  out_mode 0: y_g [M, N] f32; 1: y_g left as P32 planes of [M, N] (the next split layer's x); 2: no y_g --
 * only the output head's partial dot products (below).
 * LayerNorm folds (ln_s, ln_stat_in, ln_part_out: all NULL or all given; act must be ELU): as mms_linear_group_act's, except that
 *   ln_part_out[g] [N/64, M, 2] receives per row and 64-column slot (sum, sum of squared deviations FROM THE SLOT'S OWN MEAN) -- the
 *   two-pass form, free of E[x^2] - mean^2 cancellation; mms_row_stats_chan_group combines the slots (Chan's formula).
 * out_mode 2 (needs the folds): head_w[g] [head_dims[g], N] f32 = the output head's weight with the last LayerNorm's gamma folded in,
 *   head_dims[g] <= 16 (host array, one entry per network: an actor's action count, 1 for a critic); head_part[g] [N/64, M, stride_g],
 *   stride_g = head_dims[g] rounded up to 4, receives sum over the slot's columns of y[r, n] head_w[j, n]: the head of every network is
 *   finished by mms_marl_heads_finish (whose A[g] = head_dims[g]) without the activations ever being written.  head_dims may be NULL in
 *   the other output modes. */
int mms_linear_group_act_split(int device, int32_t groups, int64_t M, int32_t N, int32_t K, const void* const* x, const void* const* w,
                               const float* const* b, void* const* y, int32_t act, int32_t out_mode, const float* const* ln_s,
                               const float* const* ln_stat_in, float* const* ln_part_out, const float* const* head_w, float* const* head_part,
                               const int32_t* head_dims, void* hip_stream);

/* ---- ... and with two scaled fp16 planes per operand (csrc/split16_kernels.hip): the default of the policy modules -----------------
 * x s = hi + lo 2^-11 with s a power of two per ROW, hi = f16(x s), lo = f16((x s - hi) 2^11): the operand is kept to 2^-22 |x| (worst
 * case; 4e-8 rms) instead of exactly, in 4 bytes instead of 6, and the product is THREE f16 MFMA products (hi hi, hi lo, lo hi) with fp32
 * accumulation -- the layers are bound by the operand stream into LDS, so the k-loop takes two thirds of the three-plane kernel's time,
 * and three LDS stages fit.  Error against the float64 product: 0.39-0.46 x the exact-fp32 MFMA kernel's on the PPO policy's layers,
 * below it down to K = 32 (tests/test_gpu_parity.py::test_split16_layers_error).  What the two missing bits cost: behind a folded
 * LayerNorm the operand error is amplified by |mean| / std of the row like the rounding of the activations themselves (x 4 against the
 * fp32 passes at |mean| / std = 1000, tests/test_marl_policy.py); the three-plane entry points above have exact operands.
 * Scales: a plane row's scale puts a bound of the row's magnitudes at 2^14 (fp16 ends at 65504).  Inputs (observations, weight rows): the
 * row's own largest magnitude, found by the split.  Hidden activations: a-priori, |act(W x + b)| <= (largest row 1-norm of W) max|x| +
 * max|b| (ELU, ReLU, tanh, identity: |act(y)| <= |y|), evaluated per row by the split of the network's input (`chain`); behind a
 * LayerNorm the bound does not depend on the data (|W~ xhat + c| <= |W~ row|_2 sqrt(K) + |c|) and the caller passes constant scales.
 * Plane format "H32": f16 [rows, KC, 2, 32], KC = ceil(K / 32): hi and lo of 32 consecutive k of a row, 128 contiguous bytes; columns
 * past K are zero.  MMS_H32_BYTES(rows, K) bytes. */
#define MMS_H32_BYTES(rows, K) ((size_t)(rows) * (size_t)(((K) + 31) / 32) * 128)

/* planes_g <- split(x_g) for `groups` matrices [rows, K] f32 (row pitch x_pitch floats, 0 = K; unaligned rows take scalar loads), with
 * scale[g][r] = the row's power of two and inv[g][r] = 1 / scale (f32 [rows]; entries of the two arrays may be NULL).
 * nchains > 0: chain[g] = f32 [nchains, L, 2] of (mult, add) per layer; for each chain c and layer l < L the bound
 * b_{l+1} = (mult_l b_l + add_l) 1.001, b_0 = the row's largest magnitude, gives chain_scale[g][c, l, r] = 2^(14 - e), b_{l+1} <= 2^e, and
 * chain_inv = its inverse (f32 [nchains, L, rows] each): the y_scale / next x_inv of the layers below.
 * stat != NULL: stat[g] f32 [rows, 2] receives (mean, 1 / sqrt(var + eps)) of every row -- the statistics of an nn.LayerNorm over the
 * rows (two-pass form), which the grouped MARL inference folds into its first layers: the split reads the rows anyway. */
int mms_split_planes16_group(int device, int32_t groups, int64_t rows, int32_t K, int32_t x_pitch, const float* const* x, void* const* planes,
                             float* const* scale, float* const* inv, int32_t nchains, int32_t L, const float* const* chain,
                             float* const* chain_scale, float* const* chain_inv, float* const* stat, float eps, void* hip_stream);

/* mms_split_planes16_group with groups = 1 and stat = NULL on the row-wise concatenation [x0[r, 0:K0] | x1[r, 0:K1]], K = K0 + K1, which
 * is never written: the input of an off-policy critic, cat(obs, act) (algorithms/rl/{ddpg,td3,sac}/module.py), read where its halves
 * lie -- a replay ring's observation rows and the actor's freshly written actions.  planes (H32 of [rows, K], zero columns past K),
 * scale and inv (f32 [rows], either may be NULL), chain_scale and chain_inv (f32 [nchains, L, rows]) are bit-identical to that call on
 * the materialised concatenation: the row's bound is the largest magnitude over both sources, an all-zero row keeps scale 1.
 * pitch0 / pitch1: floats between consecutive rows of x0 / x1 (0 = the source's own K, otherwise >= it: a row may be a slice of a wider
 * block).  K0, K1 >= 1; sources 4-byte aligned (a source whose rows are not all 16-byte aligned takes scalar loads), planes 16-byte
 * aligned.  rows == 0 succeeds and writes nothing.  Bad arguments return non-zero with mms_last_error(NULL) and write nothing. */
int mms_split_planes16_cat(int device, int64_t rows, int32_t K0, int32_t pitch0, const float* x0, int32_t K1, int32_t pitch1, const float* x1,
                           void* planes, float* scale, float* inv, int32_t nchains, int32_t L, const float* chain, float* chain_scale,
                           float* chain_inv, void* hip_stream);

/* The weights' side of the same layers, refreshed ON THE DEVICE after every parameter update (no host synchronisation, every output at
 * the caller's address: the two calls may sit at the head of a captured hipGraph of a rollout, so that a replay after an optimizer step
 * computes with the updated parameters -- ActorCritic.refresh(), algorithms/rl/ppo/module.py; the reference re-reads its nn.Linear
 * parameters in every forward, agents/algorithms/rl/ppo/module.py:73-87):
 * mms_weight_planes16_group: planes_g / scale_g / inv_g <- split of w_g [N[g], K[g]] f32 (contiguous; N, K: HOST arrays, the shapes may
 *   differ from group to group: all hidden layers of both networks in ONE launch) exactly as mms_split_planes16_group, and
 *   l1[g][n] = sum_k |w_g[n, k]| (f32 [N[g]]; l1 or l1[g] NULL: not written);
 * mms_chain_refresh16: entry e = c L + l of the bound chain, chain[e] = (max_i l1[e][i], max_i |bias[e][i]|), i < n[e] (bias or bias[e]
 *   NULL: 0) -- `chain` [nchains, L, 2] is what mms_split_planes16_group takes; l1, bias, n: HOST arrays of nchains * L <= MMS_MAX_GROUPS
 *   entries.  rows > 0: also the chain's scales for rows whose input bound is the CONSTANT bound0 (observation rows clamped to clip_obs
 *   whose planes the step kernel wrote, mms_bind_obs_planes16: bound0 = 2^14 / scale): chain_scale / chain_inv [nchains, L, rows] as
 *   mms_split_planes16_group would leave them for a row whose largest magnitude is bound0. */
int mms_weight_planes16_group(int device, int32_t groups, const int64_t* N, const int32_t* K, const float* const* w, void* const* planes,
                              float* const* scale, float* const* inv, float* const* l1, void* hip_stream);
int mms_chain_refresh16(int device, int32_t nchains, int32_t L, const float* const* l1, const float* const* bias, const int32_t* n,
                        float* chain, float bound0, int64_t rows, float* chain_scale, float* chain_inv, void* hip_stream);

/* mms_linear_group_act_split with x_g, w_g (and, out_mode 1, y_g) in the H32 format.  x_inv[g] f32 [M] and w_inv[g] f32 [N] (16-byte
 * aligned) are the inverse row scales of the operands; y_scale[g] f32 [M] (out_mode 1) is the scale the output rows are stored with --
 * it must put a bound of the row's activations at or below 2^14; the next layer's x_inv is its inverse.  Everything else (out_mode, the
 * LayerNorm folds, the output-head partials) as mms_linear_group_act_split. */
int mms_linear_group_act_split16(int device, int32_t groups, int64_t M, int32_t N, int32_t K, const void* const* x, const void* const* w,
                                 const float* const* b, void* const* y, const float* const* x_inv, const float* const* w_inv,
                                 const float* const* y_scale, int32_t act, int32_t out_mode, const float* const* ln_s,
                                 const float* const* ln_stat_in, float* const* ln_part_out, const float* const* head_w, float* const* head_part,
                                 const int32_t* head_dims, void* hip_stream);

/* The weights' side of a layer BEHIND A FOLDED LayerNorm, refreshed on the device after every update (GroupedPolicyInference.refresh():
 * no host synchronisation, every output at the caller's address; the reference re-reads its parameters in every forward,
 * agents/algorithms/utils/mlp.py:19-27,44-60).  For g < groups and row n of w_g [N[g], K[g]] (f32, contiguous; N, K: HOST arrays, the
 * shapes may differ from group to group):
 *   W~[n, k] = w[n, k] gamma_g[k] (gamma or gamma[g] NULL: w itself) -> planes_g (H32) with inv_g[n] = 1 / its row scale (planes or
 *   planes[g] NULL: no planes), wt[g] = W~ as f32 [N, K] (NULL: not stored), s[g][n] = sum_k W~[n, k], c[g][n] = sum_k w[n, k] beta_g[k] +
 *   bias_g[n] (NULL: without that term), rb[g][n] = |W~ row|_2 sqrt(K) + |c[n]|: the row's bound of W~ xhat + c over normalised inputs.
 * mms_fold_scales16_group: scale_g = 2^(14 - e) with 1.001 max_{i < n[g]} rb[g][i] <= 2^e -> scale1[g][0] (f32 [1], optional) and
 *   ysc[g][0..M) = scale_g, yinv[g][0..M) = 1 / scale_g (f32 [M] each, optional): the y_scale / next x_inv rows of
 *   mms_linear_group_act_split16 for a layer whose output bound does not depend on the data.  A zero network (largest rb[g][i] zero or
 *   at most 1e-30, or n[g] = 0) gets scale_g = 2^100 and 1 / scale_g = 2^-100, not 1: the bound is floored at 1e-30 and the shift clamped. */
int mms_fold_planes16_group(int device, int32_t groups, const int64_t* N, const int32_t* K, const float* const* w, const float* const* gamma,
                            const float* const* beta, const float* const* bias, void* const* planes, float* const* inv, float* const* s,
                            float* const* c, float* const* rb, float* const* wt, void* hip_stream);
int mms_fold_scales16_group(int device, int32_t groups, const float* const* rb, const int32_t* n, int64_t M, float* const* scale1,
                            float* const* ysc, float* const* yinv, void* hip_stream);

/* stat_g[r] = (mean, 1 / sqrt(var + eps)) of row r from mms_linear_group_act_split's ln_part_out (`slots` = N / 64 slots of 64). */
int mms_row_stats_chan_group(int device, int32_t groups, int64_t M, int32_t slots, const float* const* part, float* const* stat, float eps,
                             void* hip_stream);

/* The output heads behind an out_mode-2 layer: mean_gj[r] = rstd_r (sum_slots head_part[g][slot, r, j] - mean_r hs[g][j]) + hc[g][j] with
 * (mean_r, rstd_r) from part[g] (the last hidden layer's ln_part_out), hs = head_w 1 and hc = w beta + b (both [A[g]]); then exactly
 * mms_marl_heads_act's sampling: std / out / logp / out_pitch / counters / seed / row_offset have the same meaning. */
int mms_marl_heads_finish(int device, int32_t groups, int64_t M, int32_t slots, const float* const* part, const float* const* head_part,
                          const float* const* hs, const float* const* hc, const int32_t* A, const float* const* std, float* const* out,
                          float* const* logp, const int32_t* out_pitch, int64_t* const* counters, uint64_t seed, int64_t row_offset, float eps,
                          void* hip_stream);

/* ---- TRPO curvature products: backward and R-op of an ELU MLP (csrc/trpo_kernels.hip) ----------------------------------------------
 * The network: L = layers >= 2 Linear layers, ELU (alpha 1) after every one but the last; dims[0..L] the widths (dims[0] = input,
 * dims[L] = output), W_l [dims[l], dims[l-1]] in torch's Linear layout; x [M, dims[0]] and the hidden activations h[l-1] = h_l
 * [M, dims[l]], l = 1..L-1, as the forward left them; all f32, contiguous; 1 <= M <= 2097024.  ELU's derivatives are read from h: f' = f'' = h + 1 where
 * h <= 0, f' = 1 and f'' = 0 where h > 0.  Every product runs on the split-operand GEMM core (fp32 operands as three bf16 planes,
 * fp32 accumulation; P32 above), weight gradients as deterministic row-split sums (no atomics: results are bit-identical run to run).
 * workspace: caller-owned device memory, 256-byte aligned; workspace == NULL stores the bytes needed in *ws_bytes and returns 0
 * (the CPU build needs none: 0, and runs on any non-NULL workspace).  Otherwise *ws_bytes is the size given and a smaller one is an
 * error.
 *
 * mms_mlp_grad: J^T g of mu = MLP(x) for g [M, dims[L]]: d_L = g, dW_l = d_l^T h_{l-1}, db_l = sum over rows of d_l,
 *   e_{l-1} = d_l W_l, d_{l-1} = e_{l-1} f'(h_{l-1}).  dw[l-1] [dims[l], dims[l-1]], db[l-1] [dims[l]].  d_out / e_out (NULL: not kept)
 *   receive d_l and e_l [M, dims[l]] for l = 1..L-1 at index l-1: what mms_mlp_grad_rop reads. */
int mms_mlp_grad(int device, int32_t layers, int64_t M, const int32_t* dims, const float* x, const float* const* h, const float* const* w,
                 const float* g, float* const* dw, float* const* db, float* const* d_out, float* const* e_out, void* workspace,
                 int64_t* ws_bytes, void* hip_stream);

/* mms_mlp_grad_rop: the directional derivative (Pearlmutter's R-op) of mms_mlp_grad along the parameters' direction (V_l, c_l)
 * (v[l-1], c[l-1] shaped like W_l, b_l) with g held fixed: rmu [M, dims[L]] = J v = R{mu}, and rdw[l-1] / rdb[l-1] = R{dW_l} / R{db_l}
 * = sum over rows of g . (d2 mu / d theta2) v, the curvature term of a Hessian-vector product (the Gauss-Newton term is the caller's:
 * J^T of the loss curvature times rmu).  d, e: mms_mlp_grad's d_out / e_out for the same g.
 *   Ra_l = Rh_{l-1} W_l^T + h_{l-1} V_l^T + c_l, Rh_l = f'(h_l) Ra_l (Rh_0 = 0); Rd_L = 0,
 *   R{dW_l} = Rd_l^T h_{l-1} + d_l^T Rh_{l-1}, R{db_l} = sum Rd_l, Rd_{l-1} = (Rd_l W_l + d_l V_l) f'(h_{l-1}) + e_{l-1} f''(h_{l-1}) Ra_{l-1} */
int mms_mlp_grad_rop(int device, int32_t layers, int64_t M, const int32_t* dims, const float* x, const float* const* h, const float* const* w,
                     const float* const* v, const float* const* c, const float* g, const float* const* d, const float* const* e, float* rmu,
                     float* const* rdw, float* const* rdb, void* workspace, int64_t* ws_bytes, void* hip_stream);

/* ---- HATRPO's Fisher-vector product: J^T g and J v of a LayerNorm-ELU MLP (csrc/ln_mlp_kernels.hip) ------------------------------------
 * The network is the MARL actor's mean (agents/algorithms/utils/mlp.py:6-66 and fc_mean), L = blocks >= 1 hidden blocks:
 *   u_0 = LN(x; g_0, t_0)                                    (feature_norm)
 *   a_l = u_{l-1} W_l^T + b_l, h_l = ELU(a_l), u_l = LN(h_l; g_l, t_l)        l = 1..L
 *   mu  = u_L W_m^T + b_m
 * dims[0..L+1]: the input width, the L hidden widths and A.  LN(v; g, t) = g (v - mean) rstd + t with the biased variance and eps
 * inside the root; one eps serves every level.  Index conventions: ln_g / ln_t [L+1] hold g_l, t_l of level l = 0..L ([dims[l]]);
 * w [L+1] holds W_1..W_L and W_m at index L (torch's Linear layout, w[l-1] is [dims[l], dims[l-1]]); h [L] holds h_l [M, dims[l]] at
 * index l-1, the ELU outputs BEFORE their LayerNorm, as the forward left them; x [M, dims[0]].  All f32 and contiguous.  xhat_l, u_l and
 * ELU's f' = h + 1 (h <= 0) | 1 are re-derived from x and h_l: no a_l, u_l or normalised copy is an input, and the biases are not read.
 * Row statistics are RECOMPUTED by every call in the two-pass form (mean, then the mean of squared deviations, over the true width);
 * there is no caller-supplied statistics argument.
 * The GEMMs run on the split-operand core of the TRPO section (fp32 operands as three bf16 planes, fp32 accumulation); sums of two
 * products are concatenated along k; u_{l-1} is evaluated by the operand split from h_{l-1}; weight gradients are deterministic
 * row-split sums, the bias and affine gradients per-block column sums in double added in block order: no atomics, results are
 * bit-identical run to run.  Rows past M and columns past a width are neither read from caller memory nor written to it.
 * Limits: 1 <= blocks <= MMS_LN_MLP_MAX_BLOCKS, widths dims[0..L] in 1..MMS_LN_MLP_MAX_WIDTH, A = dims[L+1] in 1..MMS_LN_MLP_MAX_A,
 * 1 <= M <= 2097024, eps >= 0.
 * workspace / ws_bytes: mms_mlp_grad's convention (NULL stores the bytes needed and returns 0 -- nothing else is read; 256-byte aligned;
 * a smaller one is an error).  The CPU build keeps its row statistics there ((L + 1) M 16 bytes, rounded up to 256).  The workspace
 * needs no initialisation.  Bad arguments return non-zero with mms_last_error(NULL) and write nothing.
 *
 * mms_ln_mlp_grad: J^T g for g [M, A] -- the gradient of sum(g . mu) with respect to every parameter but the biases' own trivial part:
 *   dW_m = g^T u_L, db_m = sum_rows g, du_L = g W_m;  for l = L..0:  dg_l = sum_rows du_l xhat_l, dt_l = sum_rows du_l, q = du_l g_l,
 *   dh_l = rstd_l (q - mean(q) - xhat_l mean(q xhat_l)), da_l = dh_l f'(h_l), dW_l = da_l^T u_{l-1}, db_l = sum_rows da_l,
 *   du_{l-1} = da_l W_l  (level 0 ends with dg_0, dt_0: the input has no gradient output).
 *   dln_g / dln_t [L+1] receive dg_l, dt_l; dw / db [L+1] receive dW_l, db_l at index l-1 and dW_m, db_m at index L. */
#define MMS_LN_MLP_MAX_BLOCKS 7
#define MMS_LN_MLP_MAX_WIDTH 4096
#define MMS_LN_MLP_MAX_A 128
int mms_ln_mlp_grad(int device, int32_t blocks, int64_t M, const int32_t* dims, float eps, const float* x, const float* const* h,
                    const float* const* ln_g, const float* const* ln_t, const float* const* w, const float* g, float* const* dln_g,
                    float* const* dln_t, float* const* dw, float* const* db, void* workspace, int64_t* ws_bytes, void* hip_stream);

/* mms_ln_mlp_jvp: J v, the directional derivative of mu along a direction with one tensor per parameter: vg / vt [L+1] = (G_l, T_l)
 * shaped like g_l, t_l; vw / vc [L+1] = (V_l, c_l) shaped like W_l, b_l, with (V_m, c_m) at index L:
 *   Ru_0 = G_0 xhat_0 + T_0;  Ra_l = Ru_{l-1} W_l^T + u_{l-1} V_l^T + c_l, Rh_l = f'(h_l) Ra_l,
 *   Ru_l = g_l rstd_l (Rh_l - mean(Rh_l) - xhat_l mean(Rh_l xhat_l)) + G_l xhat_l + T_l;  rmu = Ru_L W_m^T + u_L V_m^T + c_m
 * rmu [M, A].  col_scale [A] (or NULL) multiplies column j of rmu on the way out: with 1 / (M std_j^2) there, a Fisher-vector product
 * of the Gaussian policy's KL is this call followed by mms_ln_mlp_grad with g = rmu. */
int mms_ln_mlp_jvp(int device, int32_t blocks, int64_t M, const int32_t* dims, float eps, const float* x, const float* const* h,
                   const float* const* ln_g, const float* const* ln_t, const float* const* w, const float* const* vg, const float* const* vt,
                   const float* const* vw, const float* const* vc, const float* col_scale, float* rmu, void* workspace, int64_t* ws_bytes,
                   void* hip_stream);

/* ---- The PPO update's loss head and its gradients in one call (csrc/ppo_loss_kernels.hip) ------------------------------------------
 * What agents/algorithms/rl/ppo/ppo.py:270-302 evaluates per minibatch behind ActorCritic.evaluate, as seven advanced-index gathers and
 * a few dozen element-wise launches forward and again in backward(): the KL of the adaptive schedule, the clipped surrogate, the
 * (clipped) value loss, the entropy term, and the gradients of the loss with respect to the networks' outputs.
 * Dense inputs, the networks' outputs for the minibatch: mu [M, A], log_std [A] (l below), value [M].  Stored inputs, read in place as
 * row indices[i] of their base (row i when indices == NULL): actions [*, A], old_logp [*], adv [*], returns [*], target_values [*],
 * old_mu [*, A], old_sigma [*, A] (what the reference stores as "sigma": log_std rows).  All f32 and contiguous, indices int64.
 *   z_ij    = (a_ij - mu_ij) exp(-2 l_j)
 *   logp_i  = sum_j (-0.5 z_ij^2 - 2 l_j - 0.5 log 2pi)          scale_tril = diag(sigma^2), as module.py:76-77 and ActorCritic.evaluate
 *   entropy = sum_j (0.5 + 0.5 log 2pi + 2 l_j)
 *   kl      = mean_i sum_j (l_j - os_ij + (exp(os_ij)^2 + (om_ij - mu_ij)^2) / (2 exp(l_j)^2) - 0.5)       (no gradient, ppo.py:273-275)
 *   r_i     = exp(logp_i - old_logp_i)
 *   surrogate  = mean_i max(-adv_i r_i, -adv_i clamp(r_i, 1 - clip, 1 + clip))
 *   value_loss = clipped_value ? mean_i max((v_i - ret_i)^2, (vc_i - ret_i)^2), vc_i = tv_i + clamp(v_i - tv_i, -clip, clip)
 *                              : mean_i (ret_i - v_i)^2
 *   loss    = surrogate + value_coef value_loss - entropy_coef entropy
 * out [5] = {loss, surrogate, value_loss, entropy, kl}.  dmu [M, A], dlog_std [A], dvalue [M] = d loss / d (mu, log_std, value), all
 * three or none (none: the five terms only) -- torch autograd's result, including how maximum and clamp split ties:
 *   g_i        = -adv_i r_i / M  where 1 - clip <= r_i <= 1 + clip or -adv_i r_i > -adv_i clamp(r_i), else 0
 *   dmu_ij     = g_i z_ij exp(-2 l_j)            dlog_std_j = sum_i g_i (2 z_ij^2 - 2) - 2 entropy_coef
 *   dvalue_i   = value_coef 2 (v_i - ret_i) / M  where clipped_value is off, |v_i - tv_i| <= clip or (v_i - ret_i)^2 > (vc_i - ret_i)^2, else 0
 * (one measure-zero difference: outside the clip range with exactly equal squares torch gives half the gradient, this gives none).
 * Sums over rows are per-block partials in double, added in a fixed order and rounded once: no atomics, results bit-identical run to
 * run; a row's dmu and dvalue depend on that row, M and the scalars alone.  At most two launches on hip_stream, no host synchronisation.
 * The entry cannot see the values of indices: every one must be a valid row of all seven stored inputs.
 * workspace / ws_bytes: mms_mlp_grad's convention (NULL stores the bytes needed and returns 0 -- nothing else is read; 256-byte aligned;
 * a smaller one is an error; the CPU build needs 0 and runs on any aligned non-NULL workspace).  The workspace needs no initialisation.
 * 1 <= M <= 0x7fffffff, 1 <= A <= MMS_PPO_LOSS_MAX_A.  Inputs are taken to be finite (finite-math device code).  Bad arguments return
 * non-zero with mms_last_error(NULL) and write nothing. */
#define MMS_PPO_LOSS_MAX_A 128
int mms_ppo_loss(int device, int64_t M, int32_t A, const float* mu, const float* log_std, const float* value, const int64_t* indices,
                 const float* actions, const float* old_logp, const float* adv, const float* returns, const float* target_values,
                 const float* old_mu, const float* old_sigma, float clip, float value_coef, float entropy_coef, int32_t clipped_value,
                 float* out, float* dmu, float* dlog_std, float* dvalue, void* workspace, int64_t* ws_bytes, void* hip_stream);

/* ---- The head of TRPO's policy step in one call (csrc/trpo_loss_kernels.hip) --------------------------------------------------------
 * What agents/algorithms/rl/trpo/trpo.py evaluates behind ActorCritic.evaluate per minibatch -- the surrogate and the KL (:287-298), the
 * output side of the KL's Hessian-vector product (:417-435) and the line search's evaluation (:464-478) -- as a dozen element-wise
 * launches forward and again backward each time.  trpo.py takes its step with respect to actor.parameters() only: log_std gets no
 * gradient anywhere in TRPO.update, so every derivative here is with respect to mu.
 * Dense inputs: mu [M, A], log_std [A] (l below), rmu [M, A] (optional).  Stored inputs, read in place as row indices[i] of their base
 * (row i when indices == NULL): actions [*, A], adv [*], old_mu [*, A], old_sigma [*, A] (what the reference stores as "sigma": log_std
 * rows).  old_logp: stored [*] and read through indices, or, with old_logp_dense != 0, a dense [M] vector read at row i (the reference's
 * line search measures every trial against the PREVIOUS evaluation's log-probabilities, trpo.py:409).  All f32 and contiguous, indices
 * int64.
 *   z_ij    = (a_ij - mu_ij) exp(-2 l_j)
 *   logp_i  = sum_j (-0.5 z_ij^2 - 2 l_j - 0.5 log 2pi)        mms_ppo_loss's, ActorCritic.evaluate's
 *   r_i     = exp(logp_i - old_logp_i)
 *   a_loss  = mean_i (-adv_i r_i)                               trpo.py:287-288, 475-476
 *   kl      = mean_i sum_j (l_j - os_ij + (exp(os_ij)^2 + (om_ij - mu_ij)^2) / (2 exp(l_j)^2) - 0.5)        trpo.py:294-298
 *   gsur_ij = (-adv_i r_i / M) z_ij exp(-2 l_j)                 = d a_loss / d mu
 *   gkl_ij  = (mu_ij - om_ij) / (exp(l_j)^2 M)                  = d kl / d mu
 *   gn_ij   = rmu_ij / (exp(l_j)^2 M)                           = (d2 kl / d mu2) rmu: the KL's Hessian in mu is diagonal and constant
 * With J = d mu / d theta the exact Hessian-vector product of the KL over the actor's parameters is
 *   H v = J^T ((J v) / (exp(l)^2 M)) + sum_rows gkl . (d2 mu / d theta2) v:
 * mms_mlp_grad_rop along v with g = gkl gives J v (its rmu) and the second term; this entry turns J v into gn; mms_mlp_grad(gn) is the
 * first term.
 * Outputs, each optional, at least one: out [2] = {a_loss, kl}, logp [M], gsur [M, A], gkl [M, A], gn [M, A].  What a call must be
 * given follows from what it asks for, and nothing else is read: log_std always; mu for out, logp, gsur, gkl; actions for out, logp,
 * gsur; old_logp and adv for out, gsur; old_mu for out, gkl; old_sigma for out; rmu for gn.  out + logp is the line search's
 * evaluation; gn alone reads log_std and rmu and nothing stored.
 * Each output has the same bits whichever others are asked for.  A row's outputs depend on that row, M and log_std alone.  The two sums
 * are per-block partials in double, added in a fixed order, divided by M and rounded once: no atomics, no memset, bit-identical run to
 * run.  At most two launches on hip_stream (one without out), no host synchronisation, graph-capturable.  16-byte accesses where A is a
 * multiple of 4 and every [*, A] base given is 16-byte aligned; element by element otherwise, with the same bits.  gkl and gn have the
 * same bits in the HIP and the CPU build (csrc/trpo_loss_lane.h says why the others agree to rounding only); on one build a_loss, kl
 * and gsur have the bits of mms_ppo_loss's surrogate (with a clip range that holds every ratio), kl and dmu.
 * The entry cannot see the values of indices: every one must be a valid row of the stored inputs in use.
 * workspace / ws_bytes: mms_mlp_grad's convention (NULL stores the bytes needed and returns 0 -- nothing else is read; 256-byte aligned;
 * a smaller one is an error; the CPU build needs 0 and runs on any aligned non-NULL workspace).  The workspace needs no initialisation.
 * 1 <= M <= 0x7fffffff, 1 <= A <= MMS_PPO_LOSS_MAX_A.  Inputs are taken to be finite.  Bad arguments -- a pointer the requested outputs
 * need is NULL (gn without rmu among them), no output at all, A or M out of range, a small or misaligned workspace -- return non-zero
 * with mms_last_error(NULL) and write nothing. */
int mms_trpo_heads(int device, int64_t M, int32_t A, const float* mu, const float* log_std, const float* rmu, const int64_t* indices,
                   const float* actions, const float* adv, const float* old_mu, const float* old_sigma, const float* old_logp,
                   int32_t old_logp_dense, float* out, float* logp, float* gsur, float* gkl, float* gn, void* workspace, int64_t* ws_bytes,
                   void* hip_stream);

/* ---- The MAPPO / HAPPO update's loss head and its gradients in one call (csrc/marl_loss_kernels.hip) --------------------------------
 * What agents/algorithms/marl/mappo_trainer.py:63-179 and happo_trainer.py:48-170 evaluate per minibatch behind
 * ACTLayer.evaluate_actions (utils/act.py:154-165, FixedNormal.log_probs, util.py:23-29) for a Box action space: the per-dimension
 * Gaussian log-density, the clipped surrogate (with HAPPO's factor), the entropy term, the PopArt-normalised, clipped, Huber or
 * squared value loss, the active masks, and the gradients of the objective with respect to the networks' outputs.
 * Dense inputs, the networks' outputs for the minibatch: mu [M, A], std [A] (sigmoid(log_std / std_x_coef) std_y_coef, formed by the
 * caller), value [M].  Stored inputs, read in place: field F's row for minibatch row i is F.base + indices[i] * F.pitch (row i when
 * indices == NULL), pitch in floats -- a SeparatedReplayBuffer's tensors (pitch A or 1) as well as one agent's view of a shared
 * [T, N, agents, A] or [T+1, N, agents] block (pitch agents * A or agents).  actions and old_logp hold A floats per row (pitch >= A),
 * adv, value_preds, returns, active_masks and factor one (pitch >= 1).  A [T+1, N, .] field is read through its first T N rows, so
 * one flat index t N + n serves every field.  active_masks.base is required only with a mask flag and not read otherwise;
 * factor.base NULL means f = 1.  All f32, indices int64.
 *   logp_ij = -(a_ij - mu_ij)^2 / (2 std_j^2) - log std_j - 0.5 log 2pi                  per dimension, not summed (as stored)
 *   r_i     = exp(sum_j (logp_ij - old_logp_ij))
 *   s_i     = f_i min(r_i adv_i, clamp(r_i, 1 - clip, 1 + clip) adv_i)
 *   w_i     = m_i / sum_k m_k where the respective mask flag (policy_masks / value_masks) is on, else 1 / M
 *   policy_loss  = -sum_i w_i s_i
 *   dist_entropy = sum_j (0.5 + 0.5 log 2pi + log std_j) * (policy_masks ? 1 : 1 / A)    (act.py:161 against act.py:163)
 *   t_i     = use_norm ? (ret_i - norm_mean) / sqrt(norm_var) : ret_i                    norm_mean, norm_var: device scalars [1]
 *   vc_i    = vp_i + clamp(v_i - vp_i, -clip, clip);  e_o = t_i - v_i;  e_c = t_i - vc_i
 *   h(e)    = use_huber ? (|e| <= d: e^2 / 2;  e > d: d (|e| - d / 2);  e < -d: 0) : e^2 / 2    (util.py:23-26: b = (e > d))
 *   vl_i    = clipped_value ? max(h(e_o), h(e_c)) : h(e_o);   value_loss = sum_i w_i vl_i
 *   objective = policy_loss - entropy_coef dist_entropy + value_loss_coef value_loss
 * out [5] = {objective, policy_loss, value_loss, dist_entropy, ratio_mean = mean_i r_i}.  dmu [M, A], dstd [A], dvalue [M] =
 * d objective / d (mu, std, value), all three or none (none: the terms only) -- torch autograd's result, including how min, max and
 * clamp split ties:
 *   g_i      = -f_i adv_i r_i w_i   where 1 - clip <= r_i <= 1 + clip or adv_i r_i < adv_i clamp(r_i), else 0
 *   dmu_ij   = g_i (a_ij - mu_ij) / std_j^2
 *   dstd_j   = sum_i g_i ((a_ij - mu_ij)^2 / std_j^3 - 1 / std_j) - entropy_coef (policy_masks ? 1 : 1 / A) / std_j
 *   h'(e)    = use_huber ? (|e| <= d: e;  e > d: d;  e < -d: 0) : e
 *   dvalue_i = -value_loss_coef w_i h'(e_o)  where clipped_value is off, h(e_o) > h(e_c) or |v_i - vp_i| <= clip, else 0
 * (one measure-zero difference: outside the clip range with exactly equal non-zero losses torch gives half the gradient, this none).
 * row_logp [M] = sum_j logp_ij, or NULL: what HAPPO's factor update evaluates before and after an agent's update.
 * Sums over rows are per-block partials in double, added in a fixed order and rounded once: no atomics, no memset, results
 * bit-identical run to run; the lane roles and every sum's order depend on A alone.  Two launches on hip_stream, three with a mask
 * flag (sum_k m_k first), no host synchronisation.  A mask sum of zero is the caller's error, as in the reference (0 / 0).
 * The entry cannot see the values of indices: every one must be a valid row of every stored field.
 * workspace / ws_bytes: mms_mlp_grad's convention (NULL stores the bytes needed and returns 0 -- nothing else is read; 256-byte aligned;
 * a smaller one is an error; the CPU build needs 0 and runs on any aligned non-NULL workspace).  The workspace needs no initialisation.
 * 1 <= M <= 0x7fffffff, 1 <= A <= MMS_MARL_LOSS_MAX_A.  Inputs are taken to be finite (finite-math device code).  Bad arguments return
 * non-zero with mms_last_error(NULL) and write nothing. */
#define MMS_MARL_LOSS_MAX_A 128
typedef struct {
    const float* base;
    int64_t pitch;          /* floats from one row to the next */
} mms_rows;
typedef struct {
    mms_rows actions, old_logp, adv, value_preds, returns, active_masks, factor;
} mms_marl_loss_fields;
int mms_marl_ppo_loss(int device, int64_t M, int32_t A, const float* mu, const float* std, const float* value, const int64_t* indices,
                      const mms_marl_loss_fields* fields, float clip, float value_loss_coef, float entropy_coef, float huber_delta,
                      int32_t use_huber, int32_t clipped_value, int32_t policy_masks, int32_t value_masks, int32_t use_norm,
                      const float* norm_mean, const float* norm_var, float* out, float* dmu, float* dstd, float* dvalue, float* row_logp,
                      void* workspace, int64_t* ws_bytes, void* hip_stream);

/* mms_marl_ppo_loss for up to MMS_MAX_GROUPS agents in one call: the loss heads of a MAPPO run's agents, whose updates do not depend
 * on each other.  M, A, the four scalars and the five flags are shared; `table` is a HOST array of `groups` structs with what
 * mms_marl_ppo_loss takes per call: indices may be NULL per group, dmu / dstd / dvalue are all three or none per group, row_logp may
 * be NULL per group, norm_mean / norm_var are read only with use_norm, the fields as in the single entry (per-group bases and pitches:
 * separate buffers as well as the agents' views of one [T, N, agents, A] block).
 * Group g's outputs are bit-identical to mms_marl_ppo_loss called with group g's arguments (the rule of mms_q_heads_backup_group), on
 * both builds: the same lane roles, the same order of every sum, the mask sum over group g's masks alone, per-block partials in
 * double added in the single entry's order and rounded once.  No atomics, no memset, bit-identical run to run.
 * Launches: three on hip_stream whatever `groups` is, the group on the grid's second dimension; no host synchronisation, no copy:
 * the call is stream-ordered and can be captured in a graph.  How the table travels: one struct per group (18 pointers and 7
 * pitches, 200 bytes) is 6.4 KB for 32 groups, and as arrays per member the rows pass alone reads 16 pointers and 7 pitches per
 * group (5.9 KB), more than the 4 KB of kernel arguments.  So every pass carries in its own kernel arguments the per-group arrays
 * it can (as mms_marl_heads_eval and mms_gru_group carry theirs: 2.8 KB for the rows pass, 0.8 KB for the finish pass), and the 12
 * words per group that do not fit beside the rows pass's (std, norm_mean, norm_var, the bases of active_masks and factor, the seven
 * pitches: 3 KB) travel in the arguments of the FIRST launch, which stores them at the head of the workspace, where the rows pass
 * reads them; with a mask flag that first launch is the mask-sum pass, without one it does only this.  (A host-to-device copy of
 * the table would read a host buffer that a captured graph outlives.)  Two launches without a mask flag would need the rows pass to
 * hold all 23 words per group.
 * workspace / ws_bytes: mms_mlp_grad's convention for this groups, M and A (NULL stores the bytes needed and returns 0 -- nothing
 * else is read, not even table; 256-byte aligned; a smaller one is an error; the CPU build needs 0 and runs on any aligned non-NULL
 * workspace).  No initialisation needed.  Errors: the single entry's per group, groups outside 1..MMS_MAX_GROUPS, table NULL; any
 * error returns non-zero with mms_last_error(NULL) and writes nothing for any group. */
typedef struct {
    const float *mu, *std, *value;
    const int64_t* indices;
    mms_marl_loss_fields fields;
    const float *norm_mean, *norm_var;
    float *out, *dmu, *dstd, *dvalue, *row_logp;
} mms_marl_loss_group;
int mms_marl_ppo_loss_group(int device, int32_t groups, int64_t M, int32_t A, const mms_marl_loss_group* table, float clip,
                            float value_loss_coef, float entropy_coef, float huber_delta, int32_t use_huber, int32_t clipped_value,
                            int32_t policy_masks, int32_t value_masks, int32_t use_norm, void* workspace, int64_t* ws_bytes,
                            void* hip_stream);

/* ---- the parameter step: gradient-norm clip + Adam + polyak in two launches ---------------------------------------------------
 * What every learner ends a minibatch with -- nn.utils.clip_grad_norm_, torch.optim.Adam.step() and, off-policy, the per-parameter
 * polyak loop (algorithms/rl/sac/sac.py:325-349, rl/ppo/ppo.py's update, marl/mappo_trainer.py, marl/maddpg/module.py:280-292) -- for
 * up to MMS_PARAM_MAX_TENSORS tensors per call.  numel, param, grad, exp_avg, exp_avg_sq, target: HOST arrays of `tensors` entries
 * (element counts / device pointers, all f32); a pointer array may be NULL as a whole (= every entry NULL), and per tensor:
 *   grad[t]    NULL: no Adam for this tensor (torch skips p.grad is None) and no share in the norm
 *   param[t]   NULL with grad[t] given: the tensor takes part in the norm ONLY (the reference's SAC clips over
 *              actor_critic.parameters() while it steps only the Q or only the pi parameters)
 *   exp_avg[t], exp_avg_sq[t]: Adam's moments, both or neither; required where param[t] and grad[t] are given
 *   target[t]  NULL: no polyak; given (it needs param[t]): averaged towards the NEW parameter, also where grad[t] is NULL
 * Norm:   total = sqrt(sum over tensors with a grad of sum g^2); coef = min(1, max_norm / (total + 1e-6)), or 1 with max_norm <= 0:
 *         clip_grad_norm_ with the L2 norm.  norm_out (a device float, or NULL: not stored) receives total, the UNCLIPPED norm, as
 *         clip_grad_norm_ / get_gard_norm return it.  The gradients are NOT rewritten in place: grad is only read.
 * Adam:   torch.optim.Adam's default rule (no amsgrad, no maximize), with g' = coef g + weight_decay p (weight_decay == 0: coef g):
 *           m += (g' - m) (1 - beta1);   v = beta2 v + (1 - beta2) g'^2
 *           p -= (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *         step >= 1 is the step number AFTER this call, by value (a captured graph would replay the same number); the bias
 *         corrections and 1 - beta are formed in double on the host and rounded once, as torch does with its Python scalars.
 * Polyak: target = target polyak + (1 - polyak) p_new, rounded as the reference's two statements round --
 *         fl(fl(t (float)polyak) + fl(c p)), c = (float)(1.0 - polyak), no fused multiply-add: bit-identical to
 *         p_targ.mul_(polyak); p_targ.add_((1 - polyak) * p).
 * The hyperparameters are doubles because the reference holds them as Python floats: (float)(1.0 - 0.995) is not 1.f - 0.995f.
 * Arithmetic: IEEE fp32 division and square root, no contraction, no finite-math assumption -- a non-finite gradient reaches the
 * norm and the parameters exactly as it does through torch (an inf makes total inf, coef 0 and that element NaN).  Device code
 * flushes subnormals to zero (an exp_avg_sq below 1.2e-38 becomes 0).
 * Two launches on hip_stream, no atomics, no grid-wide wait, no host synchronisation, no table copy (the tensor table travels in
 * the kernel arguments).  Each tensor is cut into chunks of MMS_PARAM_CHUNK elements, one workgroup per chunk.  Launch 1 leaves one
 * double per chunk of every tensor with a grad in `partials` (fixed order inside the workgroup); launch 2's workgroups each add ALL
 * partials in one fixed order -- every workgroup forms the same coef -- and stream their chunk: read p, g, m, v, target, write p, m,
 * v, target.  Results are bit-identical run to run; with max_norm <= 0 a tensor's results do not depend on the other tensors of
 * the call.  Launch 1 is skipped when no norm is asked for (max_norm <= 0 and norm_out == NULL); partials may then be NULL.
 * (The CPU build walks the same chunk tables; it adds a chunk's squares one after another where the device adds per thread and then
 * across the workgroup, so the two builds' norms can differ in the last bit; the element rule is the same source.)
 * partials: a device workspace of mms_param_step_partials(tensors, numel) doubles = sum over t of ceil(numel[t] / MMS_PARAM_CHUNK)
 * (at least 1), 8-byte aligned, no initialisation needed.
 * Any 4-byte-aligned pointer is taken (parameters are often views into larger storages): where a tensor's pointers share their
 * offset within 16 bytes the chunk is streamed in 16-byte accesses behind a scalar head and in front of a scalar tail, otherwise
 * element by element.  Elements past numel[t] are never touched.  The arrays of one call must not overlap one another.
 * numel[t] == 0 and tensors == 0 succeed and touch nothing.  flags: reserved, must be 0.
 * Non-zero with mms_last_error(NULL), and nothing written, for: tensors outside 0..MMS_PARAM_MAX_TENSORS, step < 1, a beta outside
 * [0, 1), negative or non-finite lr / eps / weight_decay, flags != 0, negative numel, more than 2^31 - 1 chunks, exp_avg[t] without
 * exp_avg_sq[t] or the reverse, param[t] and grad[t] without moments, target[t] without param[t], a pointer that is not 4-byte
 * aligned, and a norm asked for with partials NULL or not 8-byte aligned. */
#define MMS_PARAM_MAX_TENSORS 48
#define MMS_PARAM_CHUNK 4096
int64_t mms_param_step_partials(int32_t tensors, const int64_t* numel);
int mms_param_step(int device, int32_t tensors, const int64_t* numel, float* const* param, const float* const* grad, float* const* exp_avg,
                   float* const* exp_avg_sq, float* const* target, double lr, double beta1, double beta2, double eps, double weight_decay,
                   int64_t step, double max_norm, double polyak, int32_t flags, double* partials, float* norm_out, void* hip_stream);

const char* mms_last_error(mms_handle h);   /* h may be NULL: error of the last failed mms_create */
int mms_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MMS_H */
