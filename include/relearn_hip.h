/* relearn_hip.h — C ABI of the MI355X-native batched rollout-and-update engine.
 *
 * This is the drop-in boundary for ONE hot path of edlanglois/relearn (v0.3.1):
 *   vectorised env step -> MLP policy/critic forward -> GAE/return scan -> TRPO + critic update.
 * The reference has no FFI of its own (it is 100 % Rust over tch/libtorch); the boundary it offers
 * is its trait surface.  Every entry point below names the reference interface it stands in for
 * (paths relative to the reference tree), and INTEGRATION.md shows the `extern "C"` block a Rust
 * maintainer adds to bind them behind `Environment` / `Actor` / `Agent` / `BatchUpdate`.
 *
 * Conventions
 *   - every function returns int32_t: 0 = RL_OK, otherwise an rl_status code; no exception or abort
 *     crosses the boundary; `rl_last_error(engine)` returns a static-lifetime-until-next-call message;
 *   - handles are opaque, created/destroyed by the library; device memory is library-owned;
 *   - host buffers are caller-owned and only borrowed for the duration of a call;
 *   - a handle is NOT thread-safe: one engine per GPU, driven by one host thread;
 *   - calls enqueue work on the engine's HIP stream; functions that return data to the host
 *     synchronise that stream, the others may return before the GPU has finished
 *     (`rl_engine_sync` waits);
 *   - there is NO CPU fallback: without a visible gfx950 device `rl_engine_create` fails with
 *     RL_ERR_NO_DEVICE.
 *
 * Data layout in HBM: one env per lane, struct-of-arrays, time-major trajectories
 *   obs[d][t][lane] f32, action[t][lane] u8, reward[t][lane] f32, flag[t][lane] u8 (successor code).
 * The flat sample index used by the update kernels is b = t * n_lanes + lane.
 */
#ifndef RELEARN_HIP_H
#define RELEARN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Incremented whenever an entry point is removed, an argument list or a struct layout changes, or a status code is
 * renumbered: a binding checks rl_abi_version() against the value it was generated from.  Purely additive entry
 * points (new symbols, new structs; nothing existing changes) keep the number: a binding finds them by symbol lookup.
 * 6 (round 6): covers rl_actor_critic_update_begin / _finish; the step summaries (rl_summary_*) came later under it. */
#define RL_ABI_VERSION 6

/* ---------------------------------------------------------------------------------------------
 * Status codes.  The non-generic ones mirror the reference's error enums:
 *   BuildAgentError              src/agents/mod.rs:219-226
 *   BuildEnvError                src/envs/builders.rs:62-66
 *   WriteExperienceError::Full   src/agents/buffers/mod.rs:225-228
 *   PackingError                 src/torch/packed.rs:18-23
 *   OptimizerStepError           src/torch/optimizers/mod.rs:80-94 (reported in *_stats.status;
 *                                NaN variants additionally make the call return RL_ERR_OPT_NAN because
 *                                the reference panics on them, src/torch/agents/policies/trpo.rs:154-162)
 */
typedef enum {
  RL_OK = 0,
  RL_ERR_INVALID_ARGUMENT = 1,
  RL_ERR_HIP = 2,
  RL_ERR_NO_DEVICE = 3,
  RL_ERR_BUILD_AGENT = 4,
  RL_ERR_BUILD_ENV = 5,
  RL_ERR_BUFFER_FULL = 6,
  RL_ERR_PACKING = 7,
  RL_ERR_COMM = 8,
  RL_ERR_OPT_NAN = 9,
  RL_ERR_UNSUPPORTED = 10
} rl_status;

/* Successor codes stored in `flag` (src/envs/mod.rs:257-269) */
enum { RL_SUCC_CONTINUE = 0, RL_SUCC_TERMINATE = 1, RL_SUCC_INTERRUPT = 2 };
/* OptimizerStepError as an integer (src/torch/optimizers/mod.rs:80-94) */
enum { RL_OPT_OK = 0, RL_OPT_LOSS_NOT_IMPROVING = 1, RL_OPT_CONSTRAINT_VIOLATED = 2, RL_OPT_NAN_LOSS = 3,
       RL_OPT_NAN_CONSTRAINT = 4 };
/* env kinds / step-limit wrappers (src/envs/cartpole.rs, chain.rs, wrappers/step_limit.rs:13,97) */
enum { RL_ENV_CARTPOLE = 0, RL_ENV_CHAIN = 1, RL_ENV_MEMORY = 2, RL_ENV_BANDIT = 3,
       RL_ENV_META_BANDIT = 4 /* rl_env_create_meta_bandit only (src/envs/meta.rs) */,
       RL_ENV_TABULAR_MDP = 5 /* rl_env_create_tabular_mdp only (src/envs/mdps.rs) */,
       RL_ENV_META_MDP = 6 /* rl_env_create_meta_mdp only (src/envs/meta.rs over src/envs/mdps.rs) */,
       RL_ENV_PARTITION = 7 /* rl_env_create_partition only (src/envs/partition.rs) */ };
/* bandit distributions of a meta-bandit env (src/envs/bandits.rs:128-243, src/envs/testing.rs:108-160) */
enum { RL_BANDITS_UNIFORM_BERNOULLI = 0, RL_BANDITS_ONE_HOT = 1, RL_BANDITS_ROUND_ROBIN = 2 };
enum { RL_LIMIT_NONE = 0, RL_LIMIT_LATENT = 1, RL_LIMIT_VISIBLE = 2 };

typedef struct rl_engine rl_engine;
typedef struct rl_env rl_env;
typedef struct rl_mlp rl_mlp;
typedef struct rl_traj rl_traj;
typedef struct rl_adam rl_adam;
typedef struct rl_dqn rl_dqn;
typedef struct rl_summary rl_summary;

/* ---------------------------------------------------------------------------------------------
 * Engine (one per GPU).  Stands in for `Device::cuda_if_available()` + the libtorch runtime the
 * reference configures in ActorCriticConfig.device (src/torch/agents/actor_critic.rs:20-45). */
int32_t rl_abi_version(void);
int32_t rl_device_count(int32_t *count);
int32_t rl_engine_create(int32_t device_ordinal, rl_engine **out);
int32_t rl_engine_destroy(rl_engine *engine);
int32_t rl_engine_sync(rl_engine *engine);
const char *rl_last_error(const rl_engine *engine);
/* name of the device, gcnArchName (must start with "gfx950"), CU count */
int32_t rl_engine_info(const rl_engine *engine, char *name_out, size_t name_cap, char *arch_out, size_t arch_cap,
                       int32_t *compute_units);
/* Kernel selection: 0 (default) = best kernels for the shape (fused matrix-pipe update kernels at hidden 128,
 * obs_dim 5); 1 = the v1 kernels only (what other shapes fall back to; kept selectable as an in-library cross-check:
 * same results within the tolerances stated in tests/test_gpu_parity.py). */
int32_t rl_engine_set_kernel_variant(rl_engine *engine, int32_t variant);
/* Numeric range of the fused kernels (variant 0 at hidden 128, obs_dim 5: rl_trpo_update, rl_ppo_update,
 * rl_reinforce_update, rl_critic_update / rl_values_opt_update / rl_actor_critic_update, rl_policy_gradient / _fvp /
 * _loss_kl, rl_critic_gradient, rl_dqn_update).  The reference's forward is plain f32 (Mlp::forward,
 * src/torch/modules/ff/mlp.rs:139-151) and has no bound beyond f32's own.  The fused kernels compute every product of
 * layer 1 exactly on the bf16 matrix pipe with the weights scaled by 2^96 and read relu' off the scaled accumulator, which
 * is exact — bit-for-bit the mask of the f32 pre-activation's sign — when, for every hidden unit j,
 *     sum_k |W1[j][k]| * max|obs| + |b1[j]|  <  2^31      (the scaled accumulator stays finite),
 *     sum_k |W1[j][k]|  <  2^31                           (the scaled weights themselves stay finite), and
 *     max(max_k |W1[j][k]| * min{|obs| : obs != 0}, |b1[j]|)  >=  2^-46   unless the unit's weights and bias are all zero
 *                                                         (a non-zero pre-activation cannot fall below 2^-96),
 * and every observation is finite.  With Glorot-initialised 5-128 layers (|w| <= 0.22) that is |obs| < 1.9e9 whatever the
 * small end when the biases are non-zero, and |obs| >= 7e-14 when they are zero.  Observation pieces below 2^-126 (bf16
 * subnormals: |obs| < 2^-110) may be flushed by the matrix pipe; inside the range above their contribution is below the
 * f32 rounding of the terms that carry the pre-activation.  "The f32 pre-activation" is an f32 evaluation of it: where the
 * exact value is below 2^-46 of its terms (f64 sees a sign, f32 sees 0) the mask is 0, never a fraction.
 * The mask is exact; the OUTPUTS are not the plain-f32 ones.  relu(x) is formed as (x + |x|) / 2 with the two halves summed
 * over the hidden units separately in f32, so a value or a logit carries roundings of 2^-24 of sum_j |W2[.][j] pre_j| over
 * ALL hidden units, those that are off included, where a plain f32 forward carries them of the active units' sum only:
 * measured 0.30 x 2^-24 of that sum with b1 = -1000 on 96 of 128 units (1.9e-4 absolute on values of order 0.1, where kernel
 * variant 1 is within 1e-7); with biases of the weights' own size the two sums are of one size.
 * The library checks the condition in the first fused launch of each module of every call (the later launches of the
 * same call start from parameters that call produced itself, in steps bounded by the learning rate or the KL constraint),
 * from the weights the launch has just loaded and the magnitude range of the trajectory's observation planes (measured
 * once per rollout / rl_traj_write; for DQN the collecting rollout folds the observations it writes to the replay
 * store into the same range words).  Outside the range the call returns RL_ERR_UNSUPPORTED
 * — never a silently wrong mask; its outputs are then not valid, and an update is refused WHOLE: the launch that finds the
 * violation sets a veto word on the device, which every optimiser and line-search kernel behind it reads, so parameters,
 * Adam moments and step count are what they were at entry (rl_dqn_update: put back from a snapshot).  The policy chain
 * and the critic chain have a word each: under rl_actor_critic_update[_begin] a violation of one chain refuses that
 * chain, the error names it, and the other chain's step stands (like the NaN policy step above).
 * Kernel variant 1 is plain f32 and takes any magnitudes.  tests/test_gpu_numeric_range.py; at the bounds themselves,
 * at relu'(0) = 0 and for the forward bound: tests/test_gpu_relu_edges.py. */
/* HIP-event timing of everything enqueued between begin and end on the engine stream (milliseconds) */
int32_t rl_timer_begin(rl_engine *engine);
int32_t rl_timer_end(rl_engine *engine, float *elapsed_ms);
/* Per-kernel-class accumulated device time since the last reset, measured with HIP events around each
 * launch when profiling is on (off by default: events add host overhead).  classes: see rl_kernel_class. */
typedef enum {
  RL_K_ENV_STEP = 0, RL_K_ROLLOUT = 1, RL_K_VALUES = 2, RL_K_GAE = 3, RL_K_POLICY_PASS = 4, RL_K_BACKWARD = 5,
  RL_K_REDUCE = 6, RL_K_SMALL = 7, RL_K_CRITIC_FWD = 8, RL_K_ALLREDUCE = 9, RL_K_CRITIC_FUSED = 10,
  RL_K_POLICY_FUSED = 11, RL_K_POLICY_FVP = 12 /* Fisher-vector launches of the fused policy kernel */,
  RL_K_CLASS_COUNT = 13
} rl_kernel_class;
int32_t rl_profile_enable(rl_engine *engine, int32_t on);
int32_t rl_profile_read(rl_engine *engine, double *total_ms_out /*[RL_K_CLASS_COUNT]*/,
                        uint64_t *launches_out /*[RL_K_CLASS_COUNT]*/, int32_t reset);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU: env lanes are sharded over ranks; the only exchange is an RCCL all-reduce (sum, f32)
 * of the <= 4 KiB reduced gradient / Hessian-vector / scalar vectors.  The reference has no
 * collective at all (threads + shared memory, src/simulation/train.rs:98-180); this replaces the
 * `Vec<buffer>` hand-off of train.rs:180.  `unique_id` is the 128-byte ncclUniqueId produced on
 * rank 0 and distributed by the caller (bench.py uses torch.distributed for that). */
/* RL_OK when the collective library can be bound in this process (dlopen of the librccl next to the HIP runtime in
 * use), RL_ERR_COMM otherwise.  Touches no GPU: every rank of a job calls it and the job agrees on the answer BEFORE
 * any rank enters the collective rl_comm_init (a rank that cannot load RCCL must not leave its peers blocked there). */
int32_t rl_comm_available(void);
/* Which shared objects the collective runs on: the librccl this library bound (empty before it is bound) and the
 * libamdhip64 this library is linked to — they must sit in the same directory (a host program may map a second copy of
 * the ROCm libraries; a communicator of the other copy's RCCL cannot use this runtime's streams). */
int32_t rl_comm_library_paths(char *rccl_out, size_t rccl_cap, char *hip_out, size_t hip_cap);
int32_t rl_comm_unique_id(uint8_t id_out[128]);
int32_t rl_comm_init(rl_engine *engine, int32_t rank, int32_t n_ranks, const uint8_t unique_id[128]);
int32_t rl_comm_destroy(rl_engine *engine);
/* Peer-mailbox transport for the same all-reduce (ranks = processes of ONE node): every rank owns a mailbox in its HBM,
 * exports it (rl_comm_ipc_handle: a 64-byte hipIpcMemHandle; n_ranks <= 16), the caller gathers the handles of all ranks
 * in rank order and hands them to rl_comm_init_ipc, which maps the peers' mailboxes.  An all-reduce is then ONE kernel
 * per rank: publish into every peer's mailbox, wait for every peer's sequence number (bounded), add the rows in rank
 * order — bit-identical replicas, no broadcast.  Vectors of <= 2048 floats (the feed-forward updates; recurrent modules
 * keep RCCL).  A peer that never arrives makes the next synchronising call return RL_ERR_COMM.  Undone by
 * rl_comm_destroy (all ranks, after a barrier of their own). */
int32_t rl_comm_ipc_handle(rl_engine *engine, int32_t n_ranks, uint8_t handle_out[64]);
int32_t rl_comm_init_ipc(rl_engine *engine, int32_t rank, int32_t n_ranks, const uint8_t *handles /* [n_ranks][64] */);
/* Three all-reduces of known vectors through whatever collective is installed; RL_ERR_COMM when a sum is wrong or a
 * peer does not arrive.  Collective: every rank calls it.  Lets a job agree that a transport works before relying on it. */
int32_t rl_comm_selftest(rl_engine *engine);
/* Host-staged collective for machines (or tests) without a usable RCCL communicator: for every all-reduce the library
 * copies the vector to the host, calls `fn(ctx, buf, count)` — which must sum `buf` element-wise over all ranks in place
 * (a gloo / MPI all-reduce, for instance) and return 0 — and copies the result back.  Same arithmetic contract as
 * rl_comm_init (sample-weighted means over all ranks, identical redundant updates); two PCIe hops and one host
 * collective per call, so it is a fallback, not the fast path.  Undone by rl_comm_destroy. */
typedef int32_t (*rl_host_allreduce_fn)(void *ctx, float *buf, uint64_t count);
int32_t rl_comm_init_host(rl_engine *engine, int32_t rank, int32_t n_ranks, rl_host_allreduce_fn fn, void *ctx);

/* ---------------------------------------------------------------------------------------------
 * Environments.  Mirrors `Environment::{initial_state, observe, step}` (src/envs/mod.rs:76-127) for N
 * lanes at once; state is explicit and owned by the handle. */
typedef struct {
  /* PhysicalConstants (src/envs/cartpole.rs:157-191) */
  double gravity, mass_cart, mass_pole, length_half_pole, friction_cart, friction_pole, time_step;
  /* EnvironmentParams (src/envs/cartpole.rs:194-216) */
  double action_force, max_pos, max_angle, discount_factor;
} rl_cartpole_params;
/* CartPole::default() */
int32_t rl_cartpole_params_default(rl_cartpole_params *p);

typedef struct {
  int32_t kind;          /* RL_ENV_CARTPOLE | RL_ENV_CHAIN (Chain::default, src/envs/chain.rs:38-45: obs = one-hot(5)) |
                          * RL_ENV_MEMORY (MemoryGame, src/envs/memory.rs:24-115: obs = one-hot(num_actions + history_len)) */
  int32_t limit_kind;    /* RL_LIMIT_* : `env.wrap(VisibleStepLimit::new(max_steps))` */
  uint64_t max_steps;    /* max_steps_per_episode (< 2^32) */
  uint64_t n_lanes;      /* lanes resident on THIS engine */
  uint64_t lane_offset;  /* global id of lane 0 (random streams are keyed by global lane id) */
  uint64_t seed_env;     /* env stream seed   (the `rng_env` of Steps, src/simulation/steps.rs:15-28) */
  uint64_t seed_actor;   /* actor stream seed (the `rng_actor` of Steps) */
  rl_cartpole_params cartpole;
  uint64_t chain_size;   /* RL_ENV_CHAIN: number of states (Chain::default: 5; the kernels are built for 5); 0 = 5 */
  /* RL_ENV_MEMORY: MemoryGame { num_actions, history_len } (memory.rs:24-40): any num_actions >= 2 and history_len >= 1
   * with num_actions + history_len >= 4 whose observation — one-hot(num_actions + history_len), + 1 feature under a
   * VisibleStepLimit — fits the trajectory's 8 features; other sizes, among them MemoryGame::default() = (2, 1) with its
   * three features, -> RL_ERR_BUILD_ENV (the scalar host env takes any).  0 / 0 = (2, 3), the size the fused
   * rollouts are built for; every other size steps through the standalone env kernels (feed-forward policies of
   * out_dim = num_actions: rl_mlp_create_layers).  Episodes last history_len + 1 steps; the only random draw is
   * `gen_range(0..num_actions)` in initial_state, taken sequentially from the lane's env stream. */
  uint64_t memory_num_actions, memory_history_len;
  /* RL_ENV_BANDIT: DeterministicBandit::from_values([v0, v1]) (src/envs/bandits.rs:109-116; Bandit::step :66-77): one
   * state, reward = the chosen arm's value, every step terminates, discount factor 1, no step limit.  The singleton
   * observation is presented as one-hot(5) of state 0 (its one constant feature padded to the kernels' five inputs). */
  double bandit_values[2];
} rl_env_config;

int32_t rl_env_create(rl_engine *engine, const rl_env_config *cfg, rl_env **out);
/* DeterministicBandit::from_values(values) (src/envs/bandits.rs:109-116) for `n_arms` in 2..8 — rl_env_config's
 * bandit_values holds two.  `cfg`: kind RL_ENV_BANDIT, no step limit; it supplies the lanes, the lane offset and the
 * seeds, its bandit_values are not read.  Action space IndexSpace::new(n_arms); observation and termination as in the
 * two-armed lanes (one-hot(5) of the single state, every step terminates, reward = values[action] as f32).  Anything
 * else -> RL_ERR_BUILD_ENV. */
int32_t rl_env_create_bandit(rl_engine *engine, const rl_env_config *cfg, const double *values, uint32_t n_arms,
                             rl_env **out);
/* Meta-RL bandit lanes: `MetaEnv::new(D).wrap(TrialEpisodeLimit::new(episodes_per_trial))` (src/envs/meta.rs:128-203,
 * 541-617) over Bandit<_> (src/envs/bandits.rs:58-78) — the env of relearn_experiments/src/bin/rl2-bandits.rs.  Every
 * trial draws a new bandit from D; an inner episode is one arm pull (Bandit::step always terminates), the step after a
 * pull ignores its action and starts the next inner episode (reward 0), and the pull that ends the trial's last inner
 * episode is an Interrupt: a trial of E episodes is 2 E - 1 steps.  Observation (MetaObservationSpace, meta.rs:357-363),
 * n_arms + 4 features: [inner observation is None] [prev_step is None] [one-hot(prev action)] [prev reward]
 * [episode_done].  `distribution`:
 *   RL_BANDITS_UNIFORM_BERNOULLI  UniformBernoulliBandits (bandits.rs:96-106, 170-181): n_arms means, each
 *                                 Uniform::new_inclusive(0, 1); a pull is Bernoulli::new(mean).sample
 *   RL_BANDITS_ONE_HOT            OneHotBandits (bandits.rs:229-243): reward 1 on the arm gen_range(0..n_arms), else 0
 *   RL_BANDITS_ROUND_ROBIN        RoundRobinDeterministicBandits (src/envs/testing.rs:108-160): reward 1 on arm j mod
 *                                 n_arms in a lane's j-th trial (every lane counts its own trials), no draw
 * All draws are taken sequentially from the lane's env stream.  Discount factor 1 (bandits.rs:52-54). */
typedef struct {
  uint32_t n_arms;             /* 2..4: the observation has n_arms + 4 features, a trajectory at most 8 */
  int32_t distribution;        /* RL_BANDITS_* */
  uint64_t episodes_per_trial; /* TrialEpisodeLimit::new: > 0 (and < 2^32) */
} rl_meta_bandit_config;
/* UniformBernoulliBandits::default (bandits.rs:140-144) under TrialEpisodeLimit::default (meta.rs:557-564): 2 arms,
 * RL_BANDITS_UNIFORM_BERNOULLI, 10 episodes per trial */
int32_t rl_meta_bandit_config_default(rl_meta_bandit_config *meta);
/* `cfg` supplies the lanes, the lane offset and the seeds, as in rl_env_create_bandit; its kind is not read.
 * RL_ERR_BUILD_ENV: n_arms outside 2..4, episodes_per_trial == 0 (TrialEpisodeLimit::new asserts, meta.rs:548-553) or
 * >= 2^32, an unknown distribution, a step limit in `cfg` (the trial limit is this env's limit).  rl_env_dims returns
 * (n_arms + 4, n_arms).  Feed-forward policies of n_arms outputs roll out on it; recurrent chains on two arms (more ->
 * RL_ERR_UNSUPPORTED from rl_rollout).  Not built, RL_ERR_UNSUPPORTED by name: rl_env_get_state / rl_env_set_state,
 * rl_dqn_create, rl_actor_to_cbor.  An episode of rl_summary_push is a trial. */
int32_t rl_env_create_meta_bandit(rl_engine *engine, const rl_env_config *cfg, const rl_meta_bandit_config *meta,
                                  rl_env **out);
/* The same lanes at n_arms 2..12 (6..16 observation features): the range of the reference's rl2-bandits experiment, whose
 * default is ten arms.  n_arms 2..4: rl_env_create_meta_bandit, the same handle.  RL_ERR_BUILD_ENV: n_arms outside 2..12
 * and everything rl_env_create_meta_bandit refuses.  Above four arms the lanes serve rl_env_reset / _observe / _step,
 * rl_rollout under a recurrent chain of rl_rnn_chain_create_wide (in one launch; kernel variant 1: a launch sequence per
 * step) with every update on what it collected, rl_bandit_agent_* and rl_summary_push; trajectories take up to 16
 * observation features.  Feed-forward modules have at most eight inputs and do not build for them; rl_dqn_create*,
 * rl_env_get_state / rl_env_set_state and rl_actor_to_cbor refuse every meta lane by name. */
int32_t rl_env_create_meta_bandit_wide(rl_engine *engine, const rl_env_config *cfg, const rl_meta_bandit_config *meta,
                                       rl_env **out);
/* Tabular MDP lanes: `TabularMdp<_, Normal<f64>>` (src/envs/mdps.rs:12-85), any finite MDP of 2..8 states and 2..8
 * actions given as tables; ONE MDP shared by all lanes.  `cfg` supplies the lanes, the lane offset, the seeds and the step
 * limit, as in rl_env_create_bandit; its kind is not read.  The handle's kind is RL_ENV_TABULAR_MDP.
 *   transitions   [S][A][S] f32, transitions[s][a][j] = P(s' = j | s, a); every row sums to 1
 *   reward_mean   [S][A] f64;  reward_stddev [S][A] f64, NULL: 1.0 everywhere (DirichletRandomMdps, mdps.rs:163)
 * Semantics.  initial_state is state 0 and draws nothing; the observation is the one-hot of the state, then `remaining`
 * under a VisibleStepLimit: n_states [+ 1] features, at most 8 — the lanes end at 8, so the reference's default
 * 10 x 5 does not build.  rl_env_dims returns (n_states [+ 1], n_actions).  A step in state s with action a takes its
 * draws sequentially from the lane's env stream at the even word position env_pos (as MemoryGame and meta lanes do):
 *   1. successor: one u64 at env_pos (env_pos += 2; always drawn), u = the low word as rl_u32_to_unit_f32 makes it,
 *      s' = #{ j < S - 1 : cum[s][a][j] <= u } with cum the f32 running sum of the row in index order, formed once on the
 *      host (from the row's last successor of positive probability on, the entries are exactly 1: no draw reaches 1, so
 *      the rounding of a running sum opens no bucket behind it); u == cum[j] goes to the bucket after j, a
 *      zero-probability successor is never reached
 *   2. reward: stddev[s][a] == 0: the mean, no draw; otherwise the polar normal z of include/rl_normal.h from env_pos
 *      (4 words per attempt); reward = (float)(mean + stddev * z), formed in f64
 *   3. always Successor::Continue, then the step-limit tail of the index lanes: an Interrupt at 0 remaining steps, the
 *      successor observation is written, then a reset.  RL_LIMIT_NONE: episodes never end, as on Chain lanes.
 * Lane state, in the columns MemoryGame uses: rl_env_get_state / rl_env_set_state work, state4[0] the state index,
 * state4[2] env_pos, plus steps_remaining and reset_count.
 * RL_ERR_BUILD_ENV: n_states or n_actions outside 2..8; n_states + 1 > 8 under a VisibleStepLimit; a probability that is
 * negative or not finite; a row whose f32 running sum differs from 1 by more than 1e-5; a mean that is not finite; a
 * stddev that is negative or not finite; what every env refuses of `cfg` (lanes, step limit).  A NULL pointer other than
 * reward_stddev: RL_ERR_INVALID_ARGUMENT.
 * Agents: rl_rollout with feed-forward modules of (obs_dim -> n_actions) and recurrent chains of rl_rnn_chain_create, a
 * launch sequence per step (a two-output module of the five older constructors on more than two actions ->
 * RL_ERR_UNSUPPORTED, as on every env of another width than its own); every update on what
 * it collected; rl_summary_*; the sharding over ranks (streams are keyed by global lane).  DQN: rl_dqn_create_finite with
 * a feed-forward action-value module on the per-layer kernels, at every n_actions 2..8 (step-wise collection); a module of
 * the fused shape (4 or 5 inputs, one ReLU layer of at most 128 units, two outputs, biases), a recurrent module,
 * rl_dqn_create and rl_dqn_create_recurrent -> RL_ERR_UNSUPPORTED by name.  rl_actor_to_cbor writes the form MemoryGame
 * lanes use: IndexSpace observation of n_states and action of n_actions, with the step-limit wrapper as there. */
typedef struct {
  uint32_t n_states, n_actions;
  double discount_factor;
} rl_tabular_mdp_config;
int32_t rl_env_create_tabular_mdp(rl_engine *engine, const rl_env_config *cfg, const rl_tabular_mdp_config *mdp,
                                  const float *transitions, const double *reward_mean, const double *reward_stddev,
                                  rl_env **out);
/* `DirichletRandomMdps` (mdps.rs:87-171), the distribution of the second task of the RL^2 paper, and its
 * sample_environment on the host: no engine, no device.  num_states, num_actions 1..64; alpha > 0; stddev >= 0; every
 * field finite; anything else -> RL_ERR_INVALID_ARGUMENT.  Consumes ONE stream, ChaCha8Rng::seed_from_u64(seed) with
 * set_stream(stream), sequentially, in the reference's order, row-major over (s, a): the S Gamma(alpha, 1) draws of the
 * row's Dirichlet sample (include/rl_normal.h), normalised in f64 and each cast to f32 -> transitions[s][a][.]; then the
 * row's reward mean, reward_prior_mean + reward_prior_stddev * z -> reward_mean[s][a].  The reward stddev of the sampled
 * MDP is 1 everywhere (mdps.rs:163). */
typedef struct {
  uint64_t num_states, num_actions;
  double transition_prior_dirichlet_alpha, reward_prior_mean, reward_prior_stddev, discount_factor;
} rl_random_mdps_config;
/* DirichletRandomMdps::default (mdps.rs:111-122): 10, 5, 1, 1, 1, 1 */
int32_t rl_random_mdps_config_default(rl_random_mdps_config *cfg);
int32_t rl_random_mdps_sample(const rl_random_mdps_config *cfg, uint64_t seed, uint64_t stream, float *transitions,
                              double *reward_mean);
/* Meta-RL random-MDP lanes, the second task of the RL^2 paper:
 * `MetaEnv::new(DirichletRandomMdps{..}.wrap(LatentStepLimit::new(L))).wrap(TrialEpisodeLimit::new(E))`
 * (src/envs/meta.rs:128-203, 541-617; src/envs/mdps.rs:12-171; src/envs/wrappers/mod.rs:104-123,
 * wrappers/step_limit.rs:13-89).  Every lane draws ITS OWN MDP of S = n_states and A = n_actions on the device at each
 * trial's start and keeps its tables in device memory.  S and A 2..8 with S + A + 4 <= 16; L = max_inner_steps and
 * E = episodes_per_trial positive and < 2^32.  The handle's kind is RL_ENV_META_MDP; rl_env_dims returns (S + A + 4, A).
 * Observation, S + A + 4 features in the derived product space's field order (MetaObservationSpace, meta.rs:357-363):
 *   [inner is None] [one-hot(inner state), S] [prev is None] [one-hot(prev action), A] [prev reward] [episode_done]
 * TabularMdp never terminates: an inner episode ends only by the limit's Interrupt(state), whose state is kept, so
 * feature 0 is always 0, and on the step after an inner episode's last step the state's one-hot is still there and
 * episode_done is 1.  The A + 1 entries behind a prev-None marker are zero; prev reward is the step's f32 reward.
 * Step, inner episode done: the action is ignored; inner state <- 0, inner steps remaining <- L, prev <- None; reward 0,
 *   Continue, nothing drawn.
 * Step, inner episode live: TabularMdp::step on the lane's own tables as rl_env_create_tabular_mdp states it — one u64
 *   for the successor, always; then the polar normal of include/rl_normal.h unless reward_stddev is 0;
 *   reward = (float)(mean + reward_stddev z).  prev <- Some(action, reward).  The inner steps remaining drop by 1; at 0
 *   the inner episode is done and the trial has one episode less; when none is left the step is an Interrupt, the
 *   successor observation is written, then the lane is reset.  A trial is E (L + 1) - 1 steps.
 * Reset (trial start): sample_environment from the lane's env stream at the lane's word position env_pos, in
 *   rl_random_mdps_sample's order, row-major over (s, a): the row's S Gamma(alpha, 1) variates, normalised in f64 and each
 *   cast to f32 (rl_dirichlet_row_normalise), the f32 running sums (rl_mdp_row_cumulative: from the last successor of
 *   positive probability on exactly 1), then the row's mean, reward_prior_mean + reward_prior_stddev z (always drawn).
 *   The inner initial_state (state 0) draws nothing.  Lanes are keyed by seed_from_u64(seed_env) and stream = global lane,
 *   so at env_pos 0 lane g's first trial is rl_random_mdps_sample(.., seed_env, stream = g) bit for bit.
 * reward_stddev is one launch-uniform value, the stddev of every sampled MDP's rewards (mdps.rs:163: 1.0); 0 draws nothing
 * per step. */
typedef struct {
  uint32_t n_states, n_actions;
  double alpha;               /* transition_prior_dirichlet_alpha: positive and finite */
  double reward_prior_mean, reward_prior_stddev;
  double reward_stddev;       /* of the sampled MDP's rewards: >= 0 */
  double discount_factor;
  uint64_t max_inner_steps;   /* LatentStepLimit::new(L) of an inner episode */
  uint64_t episodes_per_trial; /* TrialEpisodeLimit::new(E) */
} rl_meta_mdp_config;
/* 5 states, 5 actions, alpha 1, prior N(1, 1), reward stddev 1, discount 1, L = 10, E = 10.  Five states and not
 * DirichletRandomMdps::default's ten: 10 x 5 has 19 observation features and rl_env_create_meta_mdp ends at 16
 * (rl_env_create_meta_mdp_wide takes it). */
int32_t rl_meta_mdp_config_default(rl_meta_mdp_config *meta);
/* `cfg` supplies the lanes, the lane offset and the seeds, as in rl_env_create_meta_bandit; its kind is not read.
 * RL_ERR_BUILD_ENV: sizes outside the ranges above, L or E zero or >= 2^32, alpha not positive and finite, a stddev
 * negative or not finite, a mean or discount not finite, a step limit in `cfg`.  The lanes serve rl_env_reset / _observe /
 * _step, rl_rollout under a recurrent chain of rl_rnn_chain_create_wide (one launch at (S, A) in (2,2), (3,2), (4,3),
 * (5,5), (8,4), (4,8) unless the kernel variant is 1; a launch sequence per step otherwise) or, at 2 x 2, a feed-forward
 * module of eight inputs, every update on what was collected, and rl_summary_push (an episode is a trial).  Not built,
 * RL_ERR_UNSUPPORTED by name: rl_env_get_state / rl_env_set_state, rl_dqn_create*, rl_actor_to_cbor, rl_bandit_agent_*. */
int32_t rl_env_create_meta_mdp(rl_engine *engine, const rl_env_config *cfg, const rl_meta_mdp_config *meta, rl_env **out);
/* The same lanes at n_states 2..10 and n_actions 2..8 with n_states + n_actions + 4 <= 20 observation features: the size
 * of DirichletRandomMdps::default and of the RL^2 paper's tabular-MDP task, 10 x 5 (19 features), is in this range.
 * Wherever rl_env_create_meta_mdp builds, this is that constructor and that handle.  RL_ERR_BUILD_ENV, in this entry
 * point's name: sizes outside these ranges (tested first), then everything rl_env_create_meta_mdp refuses.  At nine and
 * ten states a lane's row of running sums is sixteen floats in device memory; rl_env_meta_mdp_read_tables returns `cum`
 * at the logical width S whatever the padded row is.  Above 16 features the lanes serve rl_env_reset / _observe / _step,
 * rl_rollout under a recurrent chain of rl_rnn_chain_create_wide20 into a trajectory of rl_traj_create_wide (one launch
 * at 10 x 5 unless the kernel variant is 1; a launch sequence per step otherwise), every update on what was collected,
 * and rl_summary_push.  Feed-forward modules (at most eight inputs) do not build for them; rl_dqn_create*,
 * rl_env_get_state / rl_env_set_state, rl_actor_to_cbor and rl_bandit_agent_* refuse every meta-MDP lane by name. */
int32_t rl_env_create_meta_mdp_wide(rl_engine *engine, const rl_env_config *cfg, const rl_meta_mdp_config *meta,
                                    rl_env **out);
/* PartitionGame lanes (src/envs/partition.rs:86-130) under the index lanes' step limit: `cfg` supplies the lanes, the lane
 * offset, the seeds and the limit (RL_LIMIT_NONE, RL_LIMIT_LATENT or RL_LIMIT_VISIBLE with max_steps; the experiment's
 * partition-game.rs wraps VisibleStepLimit::new(1000)); its kind is not read.  The handle's kind is RL_ENV_PARTITION;
 * rl_env_dims returns (23, 2), (24, 2) under a visible limit; PartitionGame::discount_factor is 0.999.
 * A lane: a supervisor axis 0..9, an element of ten booleans, the feedback Option<(previous element, its label)>.
 * Reset: gen_range(0..10) over usize picks the axis, then ten gen::<bool>() in index order the element; feedback None.
 * Step: label = element[axis] (Right when set); reward +1.0f when the action index (ClassifyLeft 0, ClassifyRight 1)
 * equals the label index, else -1.0f; feedback = Some((element, label)); ten gen::<bool>() draw the next element.  The env
 * never terminates itself; the step-limit tail is the index lanes'.  Every draw is taken sequentially from the lane's env
 * stream (ChaCha8 of seed_env, stream = global lane); gen::<bool>() is one next_u32 whose sign bit is the value.
 * Features: [element, 10] [feedback is None] [previous element, 10] [one-hot label: Left, Right] [+ remaining]; the 12
 * entries behind a None marker are zero.
 * The lanes serve rl_env_reset / _observe / _step, rl_rollout under a recurrent chain of rl_rnn_chain_create_wide24 into
 * a trajectory of rl_traj_create_wide24 (one launch at 24 features unless the kernel variant is 1; a launch sequence per
 * step otherwise), every update on what was collected, and rl_summary_push.  RL_ERR_UNSUPPORTED by name: feed-forward
 * modules in rl_rollout (they have at most eight inputs), rl_dqn_create*, rl_env_get_state / rl_env_set_state,
 * rl_actor_to_cbor, rl_bandit_agent_*. */
int32_t rl_env_create_partition(rl_engine *engine, const rl_env_config *cfg, rl_env **out);
/* The current trial's tables of lanes first_lane .. first_lane + n - 1 (local lanes) as the lanes read them; read-only.
 * cum_out [n][S*A][S] f32 running sums, mean_out [n][S*A] f64; either may be NULL. */
int32_t rl_env_meta_mdp_read_tables(rl_env *env, uint64_t first_lane, uint64_t n, float *cum_out, double *mean_out);
int32_t rl_env_destroy(rl_env *env);
/* number of observation features (CartPole 4, +1 `remaining` under VisibleStepLimit) and actions */
int32_t rl_env_dims(const rl_env *env, uint32_t *obs_dim, uint32_t *n_actions);
/* Environment::initial_state for every lane (a new episode in every lane) */
int32_t rl_env_reset(rl_env *env);
/* Environment::observe -> feature vectors, SoA [obs_dim][n_lanes] f32 (host buffer) */
int32_t rl_env_observe(rl_env *env, float *obs_out);
/* Environment::step for every lane with host-side actions (u8 indices below the env's action count, anything else ->
 * RL_ERR_INVALID_ARGUMENT; rl_env_upload_actions checks the same); lanes whose episode ends start a new one.  Outputs (host, may be NULL): reward[n] f32, flag[n] u8, next observation features
 * [obs_dim][n] (of the NEW episode when the lane was reset), interrupt successor features [obs_dim][n]
 * (valid where flag == RL_SUCC_INTERRUPT). */
int32_t rl_env_step(rl_env *env, const uint8_t *actions, float *reward_out, uint8_t *flag_out, float *obs_out,
                    float *term_obs_out);
/* Same step with everything device-resident (no PCIe): actions from / results to the env's own HBM
 * staging buffers.  `rl_env_upload_actions` fills the action buffer once; used by bench.py. */
int32_t rl_env_upload_actions(rl_env *env, const uint8_t *actions);
int32_t rl_env_step_resident(rl_env *env);
/* raw lane state for parity tests: state4 [4][n] f64 (x, xdot, theta, thetadot), nv_pos[n] i32 (cached sign),
 * steps_remaining[n] u64, reset_count[n] u64.  RL_ENV_CHAIN / RL_ENV_MEMORY: state4[0][lane] holds the state index (exact
 * in f64); RL_ENV_MEMORY: state4[1] the episode's initial state, state4[2] the word position of the lane's env stream;
 * the other state4 rows and nv_pos are unused */
int32_t rl_env_get_state(rl_env *env, double *state4, int32_t *nv_pos, uint64_t *steps_remaining,
                         uint64_t *reset_count);
int32_t rl_env_set_state(rl_env *env, const double *state4, const int32_t *nv_pos, const uint64_t *steps_remaining,
                         const uint64_t *reset_count);

/* Test hook for the random streams (Prng = ChaCha8Rng used as a counter-based generator, src/lib.rs:68):
 * `n_words` consecutive 32-bit words, starting at word `first_word`, of ChaCha8Rng::seed_from_u64(seed) with
 * set_stream(stream), computed ON THE DEVICE by the block function the rollouts, resets and env steps draw from
 * (include/rl_chacha.h as compiled for gfx950).  tests/test_gpu_chacha_independent.py compares them with a from-scratch
 * implementation (RFC 7539 quarter round, 8 rounds; rand_core's PCG32 seed expansion) that shares no code with the
 * library or the oracle. */
int32_t rl_debug_stream_words(rl_engine *engine, uint64_t seed, uint64_t stream, uint64_t first_word, uint32_t n_words,
                              uint32_t *words_out);
/* Test hook for the handles' device memory: bytes and allocations of device memory that the child handles of this
 * process (envs, modules, optimisers, trajectories, DQN agents, summaries) and the scoped temporaries of the entry
 * points hold at this moment.  Process-wide, so it takes no engine; either pointer may be NULL.  Whatever is created
 * and destroyed between two reads leaves both numbers as they were (tests/test_gpu_device_memory.py). */
int32_t rl_debug_device_memory(uint64_t *live_bytes, uint64_t *live_allocations);

/* ---------------------------------------------------------------------------------------------
 * Modules.  `MlpConfig::build_module` with one hidden layer, ReLU, identity output
 * (src/torch/modules/ff/mlp.rs:25-69); parameters are exchanged in the reference's flat order
 * (kernel [out][in] then bias per layer: ff/linear.rs:108-110, torch/utils.rs:10-22). */
int32_t rl_mlp_create(rl_engine *engine, uint32_t in_dim, uint32_t hidden, uint32_t out_dim, rl_mlp **out);
/* Activation (src/torch/modules/ff/activation.rs:11-20,85-92): the unit variants of the reference's enum, in its
 * declaration order.  Sigmoid and tanh are the engine's deterministic ones (include/rl_detmath.h, within 2.5 ulp of
 * libm), shared with the oracle like every transcendental of the bit-exact paths. */
typedef enum {
  RL_ACT_IDENTITY = 0,
  RL_ACT_RELU = 1,
  RL_ACT_SIGMOID = 2,
  RL_ACT_TANH = 3
} rl_activation;
/* MlpConfig { hidden_sizes, activation, output_activation, .. } (src/torch/modules/ff/mlp.rs:13-34,139-151): in_dim ->
 * hidden_sizes[0] -> ... -> out_dim with `activation` after every hidden layer and `output_activation` on the output;
 * parameters flat as [W, b] per layer in layer order.  `n_hidden` in [0, 4], every width in [1, 256], in_dim in [1, 8]
 * (the envs of this library have 4 or 5 features: other widths work on host-made histories, rl_traj_write),
 * out_dim in [1, 8], activations from rl_activation; anything else -> RL_ERR_BUILD_AGENT.  out_dim > 2 is a categorical
 * policy over IndexSpace::new(out_dim) (spaces/index.rs:19-22): rollouts, rl_policy_gradient / _fvp / _loss_kl, TRPO, PPO,
 * REINFORCE and the actor-critic update take it on envs and trajectories of that many actions (a mismatch ->
 * RL_ERR_INVALID_ARGUMENT); DQN over more than two actions -> RL_ERR_UNSUPPORTED.  One hidden layer of at most
 * 128 units with the reference's defaults (Relu, Identity) and at most two outputs is rl_mlp_create — the fused kernels every BASELINE
 * configuration runs on, which are built for exactly that; any other shape or activation runs per-layer kernels
 * (relearn_amd/csrc/kernels_general.hip: the general path, not the fast one) behind the same entry points — rollouts,
 * GAE, TRPO / PPO / REINFORCE and critic updates, DQN (collection one launch sequence per step), row-wise forward,
 * actor serialisation. */
int32_t rl_mlp_create_layers(rl_engine *engine, uint32_t in_dim, const uint32_t *hidden_sizes, uint32_t n_hidden,
                             uint32_t out_dim, int32_t activation, int32_t output_activation, rl_mlp **out);
/* The same with MlpConfig::linear_config's choice of bias vectors (LinearConfig { kernel_init, bias_init: Option<..> },
 * ff/linear.rs:13-33,54-68): bias = 0 builds every layer WITHOUT a bias vector (bias_init = None) — the flat parameter
 * vector then holds the kernels only (trainable_variables of such a Linear: the kernel, linear.rs:104-117), actor
 * documents carry `bias: null`, rl_mlp_init draws the kernels only and rl_mlp_init_with takes bias_init = NULL.  Such
 * modules run the per-layer kernels (also the 1 x <= 128 Relu shape the fused kernels would otherwise take). */
int32_t rl_mlp_create_config(rl_engine *engine, uint32_t in_dim, const uint32_t *hidden_sizes, uint32_t n_hidden,
                             uint32_t out_dim, int32_t activation, int32_t output_activation, int32_t bias, rl_mlp **out);
int32_t rl_mlp_destroy(rl_mlp *mlp);
int32_t rl_mlp_num_params(const rl_mlp *mlp, uint64_t *n);
/* Linear::new Glorot-uniform init (ff/linear.rs:54-68) from the engine-defined stream ChaCha8(seed) */
int32_t rl_mlp_init(rl_mlp *mlp, uint64_t seed);
/* LinearConfig { kernel_init, bias_init } (src/torch/modules/ff/linear.rs:13-33) with the reference's `Initializer`
 * (src/torch/initializers.rs:8-64,152-176,328-364): Zeros; Constant(value); Uniform(scale): U(+-sqrt(3 var));
 * Normal(scale): N(0, var); Orthogonal: QR of a normal [rows, cols] matrix (transposed when rows < cols), columns
 * multiplied by the sign of R's diagonal.  var = VarianceScale::variance: Constant(value) | 1 / fan_in | 1 / fan_out |
 * 2 / (fan_in + fan_out) with Linear::new's fan_in = in_dim + 1 for kernel AND bias and fan_out from the tensor's
 * shape.  Feed-forward modules only; every layer uses the same pair, as MlpConfig::linear_config does.  The draws come
 * from the engine's stream ChaCha8(seed), stream 0, in flat parameter order: one f32 per uniform element, Box-Muller
 * on consecutive pairs for normal ones (libtorch's generator is never seeded by the reference).
 * `bias_init` NULL <=> the module was built without bias vectors (rl_mlp_create_config(..., bias = 0):
 * LinearConfig::bias_init = None); a mismatch -> RL_ERR_INVALID_ARGUMENT.  rl_mlp_init(m, seed) = both Uniform(FanAvg),
 * the default. */
typedef enum { RL_INIT_ZEROS = 0, RL_INIT_CONSTANT = 1, RL_INIT_UNIFORM = 2, RL_INIT_NORMAL = 3, RL_INIT_ORTHOGONAL = 4 } rl_init_kind;
typedef enum { RL_SCALE_CONSTANT = 0, RL_SCALE_FAN_IN = 1, RL_SCALE_FAN_OUT = 2, RL_SCALE_FAN_AVG = 3 } rl_variance_scale;
typedef struct {
  int32_t kind;   /* rl_init_kind */
  int32_t scale;  /* rl_variance_scale, read by Uniform and Normal */
  double value;   /* Constant(value); VarianceScale::Constant(value) */
} rl_initializer;
int32_t rl_mlp_init_with(rl_mlp *mlp, uint64_t seed, const rl_initializer *kernel_init, const rl_initializer *bias_init);
/* The same for a recurrent chain: RnnBaseConfig { input_weights_init, hidden_weights_init, bias_init }
 * (seq/rnn/mod.rs:20-45; RnnWeights::new, :223-257: per layer W_ih from input_weights_init, W_hh from
 * hidden_weights_init, b_ih and b_hh from bias_init — 1-D tensors: fan_in 1, fan_out = gate rows) and the chain's
 * MlpConfig::linear_config { kernel_init, bias_init } (fan_in = in + 1), layer after layer from the same stream.
 * rl_mlp_init(m, seed) on a recurrent chain = (Uniform(FanAvg), Orthogonal, Zeros; Uniform(FanAvg) x 2), the defaults.
 * On a chain with a Linear tail (rl_rnn_linear_create) the last pair is that Linear's LinearConfig.
 * bias_init NULL <=> the module was built without recurrent bias vectors (rl_rnn_mlp_create_config, bias = 0:
 * RnnBaseConfig::bias_init = None); a mismatch -> RL_ERR_INVALID_ARGUMENT; mlp_bias_init NULL -> RL_ERR_UNSUPPORTED (the
 * chain's MLP is built with bias vectors); Orthogonal on a bias -> RL_ERR_INVALID_ARGUMENT (init_orthogonal asserts two
 * dimensions, initializers.rs:331-334). */
int32_t rl_rnn_mlp_init_with(rl_mlp *module, uint64_t seed, const rl_initializer *input_weights_init,
                             const rl_initializer *hidden_weights_init, const rl_initializer *bias_init,
                             const rl_initializer *mlp_kernel_init, const rl_initializer *mlp_bias_init);
int32_t rl_params_get(rl_mlp *mlp, float *host, uint64_t n);
int32_t rl_params_set(rl_mlp *mlp, const float *host, uint64_t n);
/* Forward::forward on host rows [n_rows][in_dim] -> [n_rows][out_dim] (test/utility path) */
int32_t rl_mlp_forward(rl_mlp *mlp, const float *rows, uint64_t n_rows, float *out);

/* Recurrent module `GruMlpConfig = ChainConfig<GruConfig, MlpConfig>` (src/torch/modules/mod.rs:14;
 * chain.rs:12-56; seq/rnn/mod.rs:20-45,223-257; seq/rnn/gru.rs:20-98): in_dim -> GRU(gru_hidden) -> ReLU ->
 * Linear(gru_hidden, mlp_hidden) -> ReLU -> Linear(mlp_hidden, out_dim).  The handle type is shared with the MLP:
 * every entry point that takes a module dispatches on its kind.  Flat parameter order = trainable_variables():
 * W_ih [3H, in] (gate rows r, z, n), W_hh [3H, H], b_ih [3H], b_hh [3H], then the MLP's kernel/bias pairs.
 * The kernels are built for gru_hidden = mlp_hidden = 128, in_dim = 5; narrower chains — in_dim 1..5, gru_hidden
 * 1..128, mlp_hidden 1..128 (RnnBaseConfig::hidden_size / ChainConfig::hidden_dim, MlpConfig::hidden_sizes = [h]; e.g.
 * the GRU(3 -> 4) of the reference's benches/rnn.rs) — run on the same kernels embedded with zero padding: padded
 * units stay exactly 0 and every real dot product only gains terms fma(0, 0, acc), so outputs, gradients and
 * Fisher-vector products are those of the narrow chain (forward bit-identical to the oracle's, tests/test_gpu_gru.py).
 * out_dim in {1, 2}; lanes in multiples of 32; trajectories of obs_dim = in_dim (rollouts need an env with five
 * observation features; narrower inputs come from rl_traj_write).  in_dim 6..8, widths 129..256 and stacked layers
 * (RnnBaseConfig::num_layers 2..4, rl_rnn_mlp_create) run the lane-per-thread kernels instead: see there.
 * rl_mlp_init: Glorot-uniform W_ih, orthogonal W_hh, zero biases (RnnBaseConfig::default), Linear::new for the MLP. */
int32_t rl_gru_mlp_create(rl_engine *engine, uint32_t in_dim, uint32_t gru_hidden, uint32_t mlp_hidden,
                          uint32_t out_dim, rl_mlp **out);
/* The same chain with the LSTM cell: `ChainConfig<LstmConfig, MlpConfig>` (Lstm = RnnBase<LstmImpl>,
 * src/torch/modules/seq/rnn/lstm.rs:12-51; note that the reference's alias `LstmMlpConfig` names the GRU chain,
 * modules/mod.rs:15).  Gate rows [i; f; g; o]: W_ih [4H, in], W_hh [4H, H], b_ih [4H], b_hh [4H]; the episode state
 * is (h, c), both zero at the start of an episode (lstm.rs:22-31); c' = f * c + i * g, h' = o * tanh(c').  Same
 * shapes, initialisation rule and entry points as the GRU chain (rollout, GAE, TRPO, PPO, REINFORCE, critic update,
 * serialisation). */
int32_t rl_lstm_mlp_create(rl_engine *engine, uint32_t in_dim, uint32_t lstm_hidden, uint32_t mlp_hidden,
                           uint32_t out_dim, rl_mlp **out);
/* Both chains with RnnBaseConfig's fields spelled out (seq/rnn/mod.rs:20-45: hidden_size, num_layers; the initializers
 * are RnnBaseConfig::default's): cell = RL_CELL_GRU | RL_CELL_LSTM; in_dim 1..8, hidden_size and mlp_hidden 1..256.
 * num_layers 1..4 (0 -> RL_ERR_BUILD_AGENT, > 4 -> RL_ERR_UNSUPPORTED).  Stacked layers (num_layers > 1): flat order
 * per layer [W_ih, W_hh, b_ih, b_hh] (RnnWeights::new, seq/rnn/mod.rs:223-257) — layer 0 reads the in_dim features,
 * layer l > 0 the hidden output of layer l - 1 of the same step (Tensor::gru / ::lstm with num_layers, gru.rs:41-66),
 * no dropout — then the MLP's kernel/bias pairs; rl_mlp_init draws layer after layer from one stream; the actor
 * document holds 4 tensors per layer.  Stacked chains, chains of in_dim 6..8 and widths above 128 run general lane-per-thread kernels
 * at the module's own widths (kernels_seq_stack.hip: any lane count, one launch sequence per rollout step; the path for
 * shapes the fused 5 -> 128 -> 128 tile kernels do not cover, not a fast one).  Every entry point of the single-layer
 * chains applies: rl_rollout (two-action policies on either lane family), rl_seq_forward, rl_gae, rl_trpo_update,
 * rl_ppo_update, rl_policy_gradient / _fvp / _loss_kl, rl_values_opt_update, rl_critic_update, serialisation.  Forward
 * bit-identical to the C restatement; gradients and Fisher-vector products to f32 tolerance against the f64
 * restatement, both pinned by PyTorch vectors (tests/test_gpu_stacked.py, tests/test_oracle_stacked.py). */
enum { RL_CELL_GRU = 0, RL_CELL_LSTM = 1 };
int32_t rl_rnn_mlp_create(rl_engine *engine, int32_t cell, uint32_t in_dim, uint32_t hidden_size, uint32_t num_layers,
                          uint32_t mlp_hidden, uint32_t out_dim, rl_mlp **out);
/* The same with RnnBaseConfig::bias_init's choice of bias vectors (Option<Initializer>, seq/rnn/mod.rs:20-45,246-251):
 * bias = 0 builds the recurrent layers WITHOUT b_ih / b_hh (RnnWeights::has_biases = false) — flat order per layer
 * [W_ih, W_hh], then the MLP's kernel/bias pairs (the chain's MLP keeps its own LinearConfig); actor documents carry
 * `has_biases: false` and two tensors per layer; rl_mlp_init draws the weights only; rl_rnn_mlp_init_with takes
 * bias_init = NULL.  Such a module runs the lane-per-thread kernels (the gate rows start from zeros kept behind the
 * parameters); outputs are bit-identical to those of the same module with zero bias vectors, gradients are that module's
 * without the bias entries. */
int32_t rl_rnn_mlp_create_config(rl_engine *engine, int32_t cell, uint32_t in_dim, uint32_t hidden_size,
                                 uint32_t num_layers, int32_t bias, uint32_t mlp_hidden, uint32_t out_dim, rl_mlp **out);
/* ChainConfig<GruConfig | LstmConfig, LinearConfig> (modules/chain.rs:12-54, ff/linear.rs:13-68):
 * in_dim -> num_layers x RNN(hidden_size) -> ReLU -> Linear(hidden_size, out_dim) — the model of the reference's
 * rl2-bandits experiment (relearn_experiments/src/bin/rl2-bandits.rs:349,379-394: `type Model = Chain<Gru, Linear>`,
 * hidden_dim 128, policy and critic alike).  in_dim 1..8, hidden_size 1..256, num_layers 1..4 (0 -> RL_ERR_BUILD_AGENT,
 * > 4 -> RL_ERR_UNSUPPORTED), out_dim in {1, 2}, rnn_bias 0 | 1 (0: the layers of rl_rnn_mlp_create_config(...,
 * bias = 0, ...)); anything else -> RL_ERR_BUILD_AGENT.  Flat order = trainable_variables(): per layer
 * [W_ih, W_hh, b_ih, b_hh] (or [W_ih, W_hh]), then kernel [out_dim, hidden_size], then bias [out_dim]; a Linear
 * without a bias vector is not built.  rl_mlp_init draws the layers and then the Linear (Linear::new, fan_in =
 * hidden_size + 1) from the one stream with RnnBaseConfig::default's and LinearConfig::default's initializers; in
 * rl_rnn_mlp_init_with the last two arguments are the Linear's pair.  The module runs the lane-per-thread kernels at
 * every shape (5 -> 128 included: the fused tile kernels are built around the MLP tail's hidden layer), instantiated
 * without the head's hidden layer; every entry
 * point of the MLP-tail chains applies, rl_actor_critic_update with one module of each tail included.  Actor documents
 * hold `second: Linear { kernel, bias }`; a document of the other tail than the module's is refused with
 * RL_ERR_INVALID_ARGUMENT.  Outputs are bit-identical to the C restatement of the MLP-tail chain with mlp_hidden =
 * hidden_size, W1 = I, b1 = 0 (tests/test_gpu_chain_linear.py). */
int32_t rl_rnn_linear_create(rl_engine *engine, int32_t cell, uint32_t in_dim, uint32_t hidden_size,
                             uint32_t num_layers, int32_t rnn_bias, uint32_t out_dim, rl_mlp **out);
/* ChainConfig<GruConfig | LstmConfig, MlpConfig | LinearConfig> in one statement (modules/chain.rs:12-56,
 * seq/rnn/mod.rs:20-45,223-281) — and the one constructor of recurrent chains with MORE THAN TWO outputs: a categorical
 * policy over IndexSpace::new(3..8), what MetaEnv<UniformBernoulliBandits(3 | 4)>, OneHotBandits::new(3)
 * (src/agents/meta.rs:239) and MemoryGame::new(k >= 3, h) need.  The five constructors above remain the two-action
 * shorthand (out_dim in {1, 2}); for out_dim <= 2 this one builds exactly what the matching one of them builds (same
 * parameter count, same kernels, the fused 5 -> 128 -> 128 tile kernels and their padded twin included).
 *   cell RL_CELL_GRU | RL_CELL_LSTM; in_dim 1..8; hidden 1..256; num_layers 1..4 (0 -> RL_ERR_BUILD_AGENT, > 4 ->
 *   RL_ERR_UNSUPPORTED); rnn_bias 0 | 1; mlp_hidden 0..256, 0: the second module is one Linear(hidden, out_dim), else
 *   Mlp([mlp_hidden]); out_dim 1..8 (0 or 9 -> RL_ERR_BUILD_AGENT).  A NULL `out` or `cfg`: RL_ERR_INVALID_ARGUMENT.
 * out_dim >= 3 always runs the lane-per-thread kernels (kernels_seq_stack.hip) at the module's own widths, never a twin:
 * the head's outputs are computed in passes of four rows, each the forward's contract chain (acc = bias[q]; acc =
 * fma(x_k, w[q][k], acc), k ascending), so rl_seq_forward stays bit-identical to the C restatement.  Flat order, the
 * initialisation stream (the head is drawn at its real out_dim) and the actor document (head tensors [out_dim, .]) are
 * those of the two-action chains.  Every entry point of those chains applies: rl_rollout (out_dim must equal the env's
 * action count; meta-bandit lanes of 2..4 arms in one launch, every other env one launch sequence per step),
 * rl_seq_forward, rl_policy_gradient / _fvp / _loss_kl, rl_trpo_update, rl_ppo_update, rl_reinforce_update,
 * rl_actor_critic_update and its begin / finish pair, rl_params_get / _set, rl_mlp_init, rl_rnn_mlp_init_with,
 * rl_actor_to_cbor / rl_module_from_cbor.  Not an action-value module: rl_dqn_create refuses it. */
typedef struct {
  int32_t cell;        /* RL_CELL_GRU | RL_CELL_LSTM */
  uint32_t in_dim;     /* observation features */
  uint32_t hidden;     /* RnnBaseConfig::hidden_size */
  uint32_t num_layers; /* RnnBaseConfig::num_layers */
  int32_t rnn_bias;    /* RnnBaseConfig::bias_init is Some */
  uint32_t mlp_hidden; /* MlpConfig::hidden_sizes = [mlp_hidden]; 0: a Linear tail */
  uint32_t out_dim;    /* outputs: 1 (a critic) or the action count 2..8 */
} rl_rnn_chain_config;
/* RnnBaseConfig::default / ChainConfig::default over MlpConfig::default: 5 -> 128 -> [128] -> 2, one layer, bias vectors */
int32_t rl_rnn_chain_config_default(int32_t cell, rl_rnn_chain_config *cfg);
int32_t rl_rnn_chain_create(rl_engine *engine, const rl_rnn_chain_config *cfg, rl_mlp **out);
/* The same chain at in_dim 1..16 and out_dim 1..12: policy (k + 4 -> k) and critic (k + 4 -> 1) of the rl2-bandits
 * experiment on up to 12 arms.  in_dim <= 8 and out_dim <= 8: rl_rnn_chain_create, the same handle.  Beyond, the module
 * always runs the lane-per-thread kernels (the head's outputs in up to three passes of four rows), never a twin.  out_dim
 * 0 or 13, in_dim 0 or 17 -> RL_ERR_BUILD_AGENT; everything else as rl_rnn_chain_create.  Not an action-value module, and
 * no actor document on the lanes wide enough to need it. */
int32_t rl_rnn_chain_create_wide(rl_engine *engine, const rl_rnn_chain_config *cfg, rl_mlp **out);
/* The same chain at in_dim 1..20 and out_dim 1..12: the model of the RL^2 MDP experiment on 10 x 5 lanes (19 inputs; five
 * outputs for the policy, one for the critic).  "wide20" names the bound: rl_rnn_chain_create_wide keeps ending at 16.
 * in_dim <= 16: rl_rnn_chain_create_wide, the same handle and the same refusals.  in_dim 0 or 21, out_dim 0 or 13 ->
 * RL_ERR_BUILD_AGENT; everything else as rl_rnn_chain_create.  Serves trajectories of rl_traj_create_wide. */
int32_t rl_rnn_chain_create_wide20(rl_engine *engine, const rl_rnn_chain_config *cfg, rl_mlp **out);
/* The same chain at in_dim 1..24: the model of the partition-game experiment (24 inputs under the visible limit; two
 * outputs for the policy, one for the critic).  in_dim <= 20: rl_rnn_chain_create_wide20, the same handle and the same
 * refusals.  in_dim 0 or 25, out_dim 0 or 13 -> RL_ERR_BUILD_AGENT; everything else as rl_rnn_chain_create.  Serves
 * trajectories of rl_traj_create_wide24. */
int32_t rl_rnn_chain_create_wide24(rl_engine *engine, const rl_rnn_chain_config *cfg, rl_mlp **out);

/* ---------------------------------------------------------------------------------------------
 * Trajectory store (replaces VecBuffer + LazyHistoryFeatures: src/agents/buffers/vec.rs:15-143,
 * src/torch/agents/features.rs:48-213 — trajectories are born in HBM, no H2D per update). */
typedef enum {
  RL_TRAJ_OBS = 0,       /* f32 [obs_dim][T+1][n] (slot T = observation after the last step) */
  RL_TRAJ_ACTION = 1,    /* u8  [T][n] */
  RL_TRAJ_REWARD = 2,    /* f32 [T][n] */
  RL_TRAJ_FLAG = 3,      /* u8  [T][n] successor code */
  RL_TRAJ_TERM_OBS = 4,  /* f32 [obs_dim][T][n], valid where flag == INTERRUPT */
  RL_TRAJ_VALUES = 5,    /* f32 [T+1][n] critic values of OBS (after rl_gae, or a OneStepTd rl_values_opt_update); slot T
                          * is V(obs[T]) of every lane for a feed-forward critic, whatever ended step T-1.  A recurrent
                          * critic has no fresh-state value of obs[T] behind an episode end: there slot T holds what step
                          * T-1 bootstrapped from — 0 after Terminate, V(successor observation) otherwise */
  RL_TRAJ_ADVANTAGES = 6,/* f32 [T][n] */
  RL_TRAJ_RETURNS = 7,   /* f32 [T][n] discounted reward-to-go */
  RL_TRAJ_TARGETS = 8    /* f32 [T][n] value targets of the last rl_values_opt_update (StepValueTarget::targets) */
} rl_traj_field;

/* obs_dim in 1..8 (feed-forward modules take 4 or 5; the others serve recurrent chains of that in_dim, written through
 * rl_traj_write: the envs of this library have 4 or 5 features) */
int32_t rl_traj_create(rl_engine *engine, uint64_t n_lanes, uint64_t horizon, uint32_t obs_dim, rl_traj **out);
/* The same store with up to 20 observation planes (the lanes of rl_env_create_meta_mdp_wide).  Up to the width
 * rl_traj_create takes it is rl_traj_create.  Whatever reads a trajectory checks its own width against the planes'. */
int32_t rl_traj_create_wide(rl_engine *engine, uint64_t n_lanes, uint64_t horizon, uint32_t obs_dim, rl_traj **out);
/* ... with up to 24 observation planes (the lanes of rl_env_create_partition).  Up to 20 it is rl_traj_create_wide. */
int32_t rl_traj_create_wide24(rl_engine *engine, uint64_t n_lanes, uint64_t horizon, uint32_t obs_dim, rl_traj **out);
int32_t rl_traj_destroy(rl_traj *traj);
int32_t rl_traj_field_bytes(const rl_traj *traj, int32_t field, uint64_t *bytes);
int32_t rl_traj_read(rl_traj *traj, int32_t field, void *host, uint64_t bytes);
/* upload (tests: feed oracle-generated trajectories / advantages to the update kernels) */
int32_t rl_traj_write(rl_traj *traj, int32_t field, const void *host, uint64_t bytes);

/* HOT LOOP A: `horizon` calls of Steps::step per lane (src/simulation/steps.rs:113-167) with
 * PolicyActor::act (src/torch/agents/policies/actor.rs:42-55) fused in: one persistent kernel. */
int32_t rl_rollout(rl_env *env, const rl_mlp *policy, rl_traj *traj);

/* critic.advantages + reward_to_go (src/torch/agents/critics/mod.rs:101-199; opt.rs:95-104).
 * gamma = min(max_discount_factor, env discount) as f32 (opt.rs:73), lambda f32 (critics/mod.rs:78). */
int32_t rl_gae(rl_traj *traj, const rl_mlp *critic, float gamma, float lambda);
/* SeqPacked::seq_packed of a recurrent module on a trajectory (modules/chain.rs:151-161): outputs for every step,
 * host [out_dim][T][n]; succ_out (may be NULL): outputs at the successor observation of every cut episode
 * (Interrupt / horizon), 0 elsewhere.  The recurrent state restarts at t = 0 and after every episode end. */
int32_t rl_seq_forward(rl_mlp *module, rl_traj *traj, float *out, float *succ_out);

/* ---------------------------------------------------------------------------------------------
 * TRPO policy update: Trpo::update (src/torch/agents/policies/trpo.rs:97-164) =
 * ConjugateGradientOptimizer::trust_region_backward_step + backtracking_line_search
 * (src/torch/optimizers/conjugate_gradient.rs:115-255). */
typedef struct {
  uint64_t iterations;      /* 10 */
  uint64_t max_backtracks;  /* 15 */
  double backtrack_ratio;   /* 0.8 */
  double hpv_reg_coeff;     /* 1e-5 */
  double max_policy_step_kl;/* 0.01 (TrpoConfig, trpo.rs:38) */
  int32_t accept_violation; /* false */
} rl_trpo_config;
int32_t rl_trpo_config_default(rl_trpo_config *cfg);

/* logged scalars, named as the reference logs them under `policy/` (conjugate_gradient.rs:164,200,219-226;
 * trpo.rs:119) */
typedef struct {
  double entropy, step_size, loss_initial, loss_final, constraint_val_final, step_scale;
  int64_t num_backtracks; /* -1: line search exhausted */
  int32_t status;         /* RL_OPT_* */
  int32_t cg_iterations;
} rl_trpo_stats;

/* Device memory: with the fused kernels (variant 0, a 5 -> 128 -> 2 policy) the first rl_trpo_update /
 * rl_actor_critic_update / rl_policy_fvp on a trajectory allocates 20 bytes per sample of it (168 MB at 65,536 lanes x
 * 128 steps) beside its update workspace: the gradient pass keeps its relu' masks (16 B per sample) and the Fisher weight
 * p0 p1 (4 B) for the Fisher-vector products of the same call.  The memory is freed with the trajectory; what it holds is
 * never read by a later call. */
int32_t rl_trpo_update(rl_mlp *policy, rl_traj *traj, const rl_trpo_config *cfg, rl_trpo_stats *stats);
/* pieces of the update exposed for parity tests (host vectors in flat parameter order) */
int32_t rl_policy_gradient(rl_mlp *policy, rl_traj *traj, float *grad_out, float *loss_out, float *entropy_out);
int32_t rl_policy_fvp(rl_mlp *policy, rl_traj *traj, const float *v, float reg, float *out);
int32_t rl_policy_loss_kl(rl_mlp *policy, rl_traj *traj, const float *params0, float *loss_out, float *kl_out);

/* ---------------------------------------------------------------------------------------------
 * Critic update: ValuesOpt::update (src/torch/agents/critics/opt.rs:100-126) = n_backward_steps
 * (src/torch/agents/mod.rs:35-72) of full-batch MSE with COptimizer Adam (optimizers/coptimizer.rs:13-26,
 * 136-167; libtorch default eps 1e-8, amsgrad off). */
typedef struct {
  double learning_rate, beta1, beta2, weight_decay; /* AdamConfig (coptimizer.rs:136-156) */
  double eps;                                       /* libtorch default 1e-8 (not a field in the reference) */
} rl_adam_config;
int32_t rl_adam_config_default(rl_adam_config *cfg);
int32_t rl_adam_create(rl_mlp *module, const rl_adam_config *cfg, rl_adam **out);
int32_t rl_adam_destroy(rl_adam *opt);
/* one optimizer step from a host gradient (parity tests) */
int32_t rl_adam_step_host(rl_adam *opt, const float *grad);

/* The other first-order rules.  Every first-order update of the reference is generic over its optimiser configuration
 * (`optimizer_config: OC` in ValuesOptConfig, PpoConfig, ReinforceConfig, DqnConfig), and OC is one of the four COptimizer
 * configurations of src/torch/optimizers/coptimizer.rs: SgdConfig (:49-87), RmsPropConfig (:89-132), AdamConfig
 * (:134-168), AdamWConfig (:170-205).  The handle type stays rl_adam: an optimiser built here with any rule is passed
 * unchanged wherever the prototypes take `rl_adam *` (critic, values-opt, actor-critic, PPO, REINFORCE and DQN updates),
 * and is freed by the destroy call above.  Arithmetic is f32 in the operation order of libtorch 1.12's C++ optimisers
 * (what tch 0.8 binds; the reference passes its fields straight through, coptimizer.rs:76-86,120-131,158-167,195-204);
 * with g the gradient entry, p the parameter, k the 1-based count of applied steps:
 *   SGD      wd != 0: g = g + wd*p;  momentum != 0: buf = (k == 1) ? g : buf*momentum + (1-dampening)*g,
 *            g = nesterov ? g + momentum*buf : buf;  p = p + (-lr)*g
 *   RMSProp  wd != 0: g = g + wd*p;  sq = sq*alpha + ((1-alpha)*g)*g;  centered: ga = ga*alpha + (1-alpha)*g,
 *            avg = sqrt(sq - ga*ga) + eps, otherwise avg = sqrt(sq) + eps;  momentum > 0: buf = buf*momentum + g/avg,
 *            p = p + (-lr)*buf, otherwise p = p + (-lr)*(g/avg)
 *   AdamW    p = p*(1 - lr*wd), then Adam's moments and step without wd*p in the gradient (eps 1e-8, amsgrad off)
 * A refused step (range guard, failed exchange) changes nothing: parameters, every state slot and the step count stay,
 * so SGD's first-step rule applies to the first step that IS applied.
 * With several ranks on the peer-mailbox transport (EXPERIMENTAL, rl_comm_init_ipc above) the exchange fused into the
 * reduction launch is built for Adam only; the other rules take the two-launch route there (reduce, stand-alone exchange,
 * step kernel).
 * tests/test_gpu_optimizers.py, tests/optim_ref.py. */
enum { RL_OPTIMIZER_ADAM = 0, RL_OPTIMIZER_ADAMW = 1, RL_OPTIMIZER_SGD = 2, RL_OPTIMIZER_RMSPROP = 3 };
typedef struct {
  int32_t kind;               /* RL_OPTIMIZER_* */
  int32_t nesterov;           /* SgdConfig */
  int32_t centered;           /* RmsPropConfig */
  int32_t reserved;           /* 0 */
  double learning_rate, weight_decay;
  double beta1, beta2;        /* AdamConfig, AdamWConfig */
  double eps;                 /* Adam, AdamW (libtorch default 1e-8, not a field in the reference), RmsPropConfig */
  double momentum, dampening; /* SgdConfig; momentum also RmsPropConfig */
  double alpha;               /* RmsPropConfig */
} rl_optimizer_config;
/* the reference's Default impls: SGD lr 1e-2, momentum 0, dampening 0, wd 0, nesterov false (coptimizer.rs:64-74);
 * RMSProp lr 1e-2, momentum 0, alpha 0.99, eps 1e-8, centered false, wd 0 (:107-118); Adam and AdamW lr 1e-3, betas
 * 0.9 / 0.999, wd 0 (:147-156, :184-193; AdamW's 0 is the reference's default, not libtorch's 1e-2) */
int32_t rl_optimizer_config_default(int32_t kind, rl_optimizer_config *cfg);
/* RL_ERR_INVALID_ARGUMENT, naming the field, for what libtorch rejects: negative learning_rate, momentum, weight_decay,
 * eps or alpha; a beta outside [0, 1); nesterov with momentum <= 0 or dampening != 0; an unknown kind.  The configuration
 * is checked before the module is looked at.  Kind RL_OPTIMIZER_ADAM builds what the Adam create call above builds. */
int32_t rl_optimizer_create(rl_mlp *module, const rl_optimizer_config *cfg, rl_adam **out);
/* one optimizer step of the handle's rule from a host gradient */
int32_t rl_optimizer_step_host(rl_adam *opt, const float *grad);
/* state slot 0..2 of the rule -> host[0..n), n = the module's parameter count (Adam / AdamW: m, v; SGD: momentum buffer;
 * RMSProp: square average, momentum buffer, gradient average), and the device's step count (either may be NULL; without `host`,
 * `slot` and `n` are not looked at).  A slot the configuration does not have (it is not allocated) ->
 * RL_ERR_INVALID_ARGUMENT. */
int32_t rl_optimizer_state_read(rl_adam *opt, int32_t slot, float *host, uint64_t n, uint64_t *step_out);

typedef struct {
  double loss_first, loss_last; /* loss before the first / last optimisation step */
  uint64_t steps;
} rl_critic_stats;
/* targets = RL_TRAJ_RETURNS (StepValueTarget::RewardToGo, critics/mod.rs:203-229); `losses_out` (host,
 * may be NULL) receives the loss before each of the opt_steps steps */
int32_t rl_critic_update(rl_mlp *critic, rl_adam *opt, rl_traj *traj, uint64_t opt_steps, rl_critic_stats *stats,
                         float *losses_out);
int32_t rl_critic_gradient(rl_mlp *critic, rl_traj *traj, float *grad_out, float *loss_out);

/* ValuesOpt::update with its configuration (src/torch/agents/critics/opt.rs:13-37,100-126): the targets are computed
 * once, under no-grad, from the critic as it stands when the call begins — StepValueTarget::targets
 * (critics/mod.rs:203-229):
 *   RewardToGo  discounted_cumsum_from_end of the rewards                         (reward_to_go, critics/mod.rs:101-105)
 *   OneStepTd   r_t + discount_factor * V(successor of step t)                    (one_step_values, critics/mod.rs:139-150)
 *               with the masked extended values of eval_extended_state_values (:116-131): 0 after Terminate,
 *               V(successor observation) after Interrupt (and at the horizon cut); `scalar * tensor` then
 *               `tensor + tensor`, two f32 roundings
 * — then opt_steps_per_update x {mse_loss(V(obs), targets, Mean); backward; Adam}.  The targets stay readable as
 * RL_TRAJ_TARGETS; OneStepTd also refreshes RL_TRAJ_VALUES.  rl_critic_update above is the RewardToGo case on the
 * returns rl_gae left in RL_TRAJ_RETURNS. */
enum { RL_VALUE_TARGET_REWARD_TO_GO = 0, RL_VALUE_TARGET_ONE_STEP_TD = 1 }; /* StepValueTarget, critics/mod.rs:203-214 */
typedef struct {
  uint64_t opt_steps_per_update; /* 80 (opt.rs:46) */
  int32_t target;                /* RL_VALUE_TARGET_* ; default RewardToGo (critics/mod.rs:211-215) */
  float discount_factor;         /* max_discount_factor.min(env discount) as f32 (opt.rs:73); default 0.99 */
} rl_values_opt_config;
int32_t rl_values_opt_config_default(rl_values_opt_config *cfg);
int32_t rl_values_opt_update(rl_mlp *critic, rl_adam *opt, rl_traj *traj, const rl_values_opt_config *cfg,
                             rl_critic_stats *stats, float *losses_out /* may be NULL */);

/* ---------------------------------------------------------------------------------------------
 * The two updates of ActorCriticAgent::batch_update_slice (src/torch/agents/actor_critic.rs:176-211) after the
 * advantages — `policy.update(&features, advantages, ..)` (Trpo::update) and `critic.update(&features, ..)`
 * (ValuesOpt::update) — as ONE call.  They share no data beyond the trajectory: the advantages come from the critic as
 * it stood BEFORE either update (rl_gae), the critic's targets are the returns (or one-step TD values of the critic as
 * it stands when the call begins), so the reference's sequential order is not a dependence.  The engine therefore
 * enqueues the critic chain (targets + opt_steps_per_update x {gradient, reduce + Adam}) on a second HIP stream, with its
 * own slab rows / reduced vector / collective channel, and runs the TRPO chain on the main stream beside it: each
 * chain's single-workgroup bookkeeping launches (and, with several ranks, its latency-bound all-reduces) hide under
 * the other chain's compute.  Arithmetic and order INSIDE each chain are those of rl_trpo_update and
 * rl_values_opt_update: results are bit-identical to calling the two one after the other (tests/test_gpu_parity.py).
 * The chains run one after the other instead when the modules are not the fused 5-128-{2,1} MLPs, when kernel variant 1
 * or rl_engine_set_serial_update(engine, 1) / RELEARN_SERIAL_UPDATE=1 is selected, or when an RCCL job could not build
 * its second communicator.  Later calls on the engine are ordered after both chains.  Errors: as the two calls. */
int32_t rl_actor_critic_update(rl_mlp *policy, rl_mlp *critic, rl_adam *critic_opt, rl_traj *traj,
                               const rl_trpo_config *policy_cfg, const rl_values_opt_config *critic_cfg,
                               rl_trpo_stats *policy_stats, rl_critic_stats *critic_stats /* may be NULL */,
                               float *critic_losses_out /* may be NULL */);
/* The same update in two halves, so that the NEXT collection period can start under the critic chain.  The next
 * period's actors depend on the updated policy only (`agent.actor(mode)` snapshots the policy, src/agents/mod.rs:48-59;
 * train_parallel hands those actors to its workers, src/simulation/train.rs:98-151); the critic is next read when the
 * following batch's advantages are formed (actor_critic.rs:190-194).
 *   _begin   enqueues the critic chain on the auxiliary stream, runs the TRPO chain to its end on the main stream and
 *            returns `policy_stats` — the critic chain may still be in flight.
 *   between  rl_rollout(env, policy, OTHER trajectory) runs beside the critic chain.  Every other entry point of the
 *            engine (and a rollout into the SAME trajectory, or with the critic as its policy) is ordered behind the
 *            chain by a device-side wait: nothing can observe a half-updated critic, the calls just do not overlap.
 *   _finish  waits for the chain and returns its statistics.  Exactly one update may be pending per engine
 *            (RL_ERR_INVALID_ARGUMENT otherwise; _finish without _begin likewise).
 * rl_actor_critic_update is _begin followed by _finish.  Every number is the one the sequential calls produce: the
 * halves reorder launches across streams, never arithmetic (tests/test_gpu_parity.py).  When the chains cannot run
 * side by side (see above) _begin runs both to the end and _finish only hands the statistics over.
 * A NaN policy step (RL_ERR_OPT_NAN) is raised by _begin and ends the update (nothing stays pending); in the
 * side-by-side form the critic chain has then already advanced the critic and its optimiser state — the reference,
 * panicking inside policy.update, never reaches critic.update; in the sequential form neither does this library. */
int32_t rl_actor_critic_update_begin(rl_mlp *policy, rl_mlp *critic, rl_adam *critic_opt, rl_traj *traj,
                                     const rl_trpo_config *policy_cfg, const rl_values_opt_config *critic_cfg,
                                     rl_trpo_stats *policy_stats);
int32_t rl_actor_critic_update_finish(rl_traj *traj, rl_critic_stats *critic_stats /* may be NULL */,
                                      float *critic_losses_out /* may be NULL */);
/* 1: rl_actor_critic_update runs its two chains one after the other on the main stream (A/B runs, per-kernel timing) */
int32_t rl_engine_set_serial_update(rl_engine *engine, int32_t serial);

/* ---------------------------------------------------------------------------------------------
 * First-order policy updates and the critic-free advantage (the rest of the ActorCriticConfig matrix,
 * src/torch/agents/actor_critic.rs:20-45).
 *   Ppo::update        src/torch/agents/policies/ppo.rs:97-146  (clipped surrogate, n_backward_steps with Adam)
 *   Reinforce::update  src/torch/agents/policies/reinforce.rs:64-88 (one Adam step on -mean(log pi(a) * A))
 *   RewardToGo critic  src/torch/agents/critics/rtg.rs:28-33 (advantages = discounted reward-to-go, no update) */
typedef struct {
  uint64_t opt_steps_per_update; /* 10 */
  double clip_distance;          /* 0.2 */
} rl_ppo_config;
int32_t rl_ppo_config_default(rl_ppo_config *cfg); /* PpoConfig::default, ppo.rs:27-41 */
typedef struct {
  double entropy;               /* mean entropy at the initial parameters ("entropy", ppo.rs:114; reinforce.rs:84) */
  double loss_first, loss_last; /* surrogate loss before the first / last optimisation step */
  uint64_t steps;
} rl_policy_opt_stats;
int32_t rl_ppo_update(rl_mlp *policy, rl_adam *opt, rl_traj *traj, const rl_ppo_config *cfg,
                      rl_policy_opt_stats *stats, float *losses_out /* may be NULL */);
int32_t rl_reinforce_update(rl_mlp *policy, rl_adam *opt, rl_traj *traj, rl_policy_opt_stats *stats);
/* RL_TRAJ_ADVANTAGES = RL_TRAJ_RETURNS = reward-to-go (reward_to_go, critics/mod.rs:101-105) */
int32_t rl_reward_to_go(rl_traj *traj, float gamma);

/* ---------------------------------------------------------------------------------------------
 * DQN with the replay buffer resident in HBM (BASELINE.json configs[2]).
 *   DqnConfig / DqnAgent / DqnActor     src/torch/agents/dqn.rs:26-72,110-380
 *   ExplorationRateSchedule, DataCollectionSchedule   src/torch/agents/schedules.rs:7-69
 *   ReplayBuffer                        src/agents/buffers/replay.rs:11-127
 * Every lane is one ReplayBuffer of `buffer_capacity` steps (the reference has one per worker thread,
 * dqn.rs:129-130): step data lives in a per-lane ring `[capacity][n_lanes]`, the eviction rule "drop the whole
 * oldest episode when full" runs inside the collecting kernel.  Minibatch episodes are drawn with the agent's own
 * Prng exactly like dqn.rs:280-291 (cycle over the buffers, `Uniform::new(0, num_episodes)`, stop after the
 * episode that reaches `minibatch_steps`) — by a device kernel that evaluates the draws in parallel and keeps the
 * sequential semantics.  Targets (dqn.rs:300-309), the MSE loss on the taken action's value (dqn.rs:316-326) and
 * Adam (n_backward_steps, src/torch/agents/mod.rs:35-72) follow. */
enum { RL_DQN_TARGET_REWARD_TO_GO = 0, RL_DQN_TARGET_ONE_STEP_TD = 1 }; /* StepValueTarget, critics/mod.rs:203-214 */
enum { RL_SCHEDULE_CONSTANT = 0, RL_SCHEDULE_LINEAR_ANNEALED = 1 };     /* schedules.rs:7-15 */
enum { RL_COLLECT_CONSTANT = 0, RL_COLLECT_FIRST_REST = 1 };            /* schedules.rs:50-56 */
typedef struct {
  int32_t target;
  int32_t exploration_kind;
  double exploration_start, exploration_end; /* Constant(rate): rate = exploration_start */
  uint64_t exploration_period;
  uint64_t minibatch_steps;      /* dqn.rs:63 */
  uint64_t opt_steps_per_update; /* dqn.rs:64 */
  uint64_t buffer_capacity;      /* steps PER LANE (dqn.rs:129-130 "capacity of each individual buffer") */
  uint64_t episode_capacity;     /* episode-end slots per lane; 0 = buffer_capacity (never binds, like the deque) */
  int32_t update_kind;
  uint64_t update_first, update_rest; /* Constant(value): value = update_first */
  float discount_factor;         /* env.discount_factor() as f32 (dqn.rs:179) */
  uint32_t agent_key[8];         /* the agent's Prng seed words: Prng::from_rng(rng) in build_agent (dqn.rs:94) */
} rl_dqn_config;
/* DqnConfig::default (dqn.rs:57-72) with buffer_capacity left at 0 (the caller divides its step budget over the
 * lanes) and discount 0.99 (CartPole, src/envs/cartpole.rs:203-213) */
int32_t rl_dqn_config_default(rl_dqn_config *cfg);
/* `qnet` maps obs_dim -> n_actions; `opt` must have been created for `qnet`.  DqnConfig<MB> is generic over the module
 * (dqn.rs:26-39): any feed-forward module builds — the fused 5-128-2 shape on the fused kernels, other MlpConfigs on the
 * per-layer kernels; recurrent modules -> RL_ERR_BUILD_AGENT.
 * What builds: every env kind with two actions, each stepped by its own lane code —
 *   RL_ENV_CARTPOLE                           4 or 5 observation features
 *   RL_ENV_CHAIN                              5, or 6 under a visible step limit
 *   RL_ENV_BANDIT with two arms               5
 *   RL_ENV_MEMORY, MemoryGame(2, h)           2 + h, + 1 under a visible step limit: 4..8
 * with any feed-forward module of obs_dim inputs and 2 outputs.  A module of one Relu hidden layer of <= 128 units over 4
 * or 5 features collects in the fused kernel (the whole horizon in one launch); every other module, and every env of 6..8
 * features, collects step by step on the per-layer kernels.  Steps of 6..8 features keep features 5..7 in a second
 * 16-byte record beside the 32-byte one (the replay fields read the same: RL_REPLAY_OBS is [obs_dim][C][N]).
 * Refused: more than two actions (a bandit of >= 3 arms, MemoryGame(>= 3, h)) -> RL_ERR_UNSUPPORTED (rl_dqn_create_finite
 * builds them); a module that does
 * not match the env's (obs_dim, n_actions) -> RL_ERR_INVALID_ARGUMENT; an env kind or feature count outside the table ->
 * RL_ERR_UNSUPPORTED with a message that names it.  No env is ever collected by another env's lane code. */
int32_t rl_dqn_create(rl_env *env, rl_mlp *qnet, rl_adam *opt, const rl_dqn_config *cfg, rl_dqn **out);
/* DqnConfig<VB> over a sequence module (VB::Module: SeqPacked + SeqIterative, dqn.rs:75-86): `qnet` is a recurrent chain.
 * The returned handle is an rl_dqn like rl_dqn_create's: every rl_dqn_* entry point and rl_summary_push_dqn take it.
 *   actor    (dqn.rs:348-380) per lane and step: gen_bool(eps) first; an exploring step returns gen_range(0..2) BEFORE the
 *            module's step() — the module does not see that observation and the lane's recurrent state (h, and c of an
 *            LSTM, of every layer) stays exactly what it was; a greedy step advances the state and takes the first
 *            maximal output.  The state is zero at an episode's first step (initial_state) and at the first step of every
 *            rl_dqn_collect (the horizon rule records a cut episode as Interrupt: what follows is a new recorded episode).
 *   update   (dqn.rs:263-337) seq_packed runs every sampled episode from the zero state over ALL its observations, the
 *            explored ones included; loss = mse_loss(Q(s_t)[a_t], target_t, Mean) over the minibatch's sampled steps.
 *            RL_DQN_TARGET_ONE_STEP_TD (critics/mod.rs:101-148): the module runs over the episode plus one slot — the
 *            successor observation of an Interrupt, nothing (value 0) after a Terminate — and target_t = r_t + gamma *
 *            amax(Q_ext[t + 1]), under no_grad with the parameters of that optimisation step.
 * What builds: the env table of rl_dqn_create (CartPole 4 | 5 features, Chain 5 | 6, the two-armed bandit, MemoryGame(2, h)
 * 4..8) with any recurrent chain of obs_dim inputs and 2 outputs — GRU or LSTM, Mlp or Linear tail, 1..4 layers, with or
 * without recurrent bias vectors, from any of the recurrent constructors.  Collection is one launch per horizon on the
 * lane-per-thread kernels at the module's own widths; RL_MB_TARGET holds the recurrent targets, rl_dqn_minibatch_gradient
 * returns the gradient in the module's flat order.
 * Refused, by this entry point's name: a feed-forward module -> RL_ERR_BUILD_AGENT (use rl_dqn_create); more than two
 * actions -> RL_ERR_UNSUPPORTED; a module that does not match the env's (obs_dim, n_actions) -> RL_ERR_INVALID_ARGUMENT;
 * RL_ENV_META_BANDIT lanes -> RL_ERR_UNSUPPORTED.  rl_dqn_update of such an agent on an engine with a communicator of
 * more than one rank -> RL_ERR_UNSUPPORTED before anything is changed; rl_actor_to_cbor of a recurrent DqnActor ->
 * RL_ERR_UNSUPPORTED. */
int32_t rl_dqn_create_recurrent(rl_env *env, rl_mlp *qnet, rl_adam *opt, const rl_dqn_config *cfg, rl_dqn **out);
/* DqnConfig over any finite action space (dqn.rs:75-86, AS: FiniteSpace): 2..8 actions, a feed-forward or a recurrent
 * action-value module.  The returned handle is an rl_dqn: every rl_dqn_* entry point and rl_summary_push_dqn take it.
 *   actor    (dqn.rs:360-379) gen_bool(eps); an exploring step returns action_space.sample(rng) = gen_range(0..n_actions)
 *            from the lane's sequential actor stream (rand 0.8.5 UniformInt::sample_single: widening multiply, retry on
 *            rejection), a greedy step argmax — the first maximal of the n_actions outputs.  A recurrent module's state is
 *            held over an exploring step, as in rl_dqn_create_recurrent.
 *   targets  RL_DQN_TARGET_ONE_STEP_TD takes amax(-1) over the n_actions outputs (dqn.rs:300-309), `gamma * vnext`, then the
 *            add; the loss is mse_loss on the taken action's value (dqn.rs:316-326).
 * What builds:
 *   two actions                               what rl_dqn_create builds for a feed-forward module and rl_dqn_create_recurrent
 *                                             for a recurrent one, through them: same kernels, same bytes, same refusals
 *   RL_ENV_BANDIT of 3..8 arms                5 observation features
 *   RL_ENV_MEMORY, MemoryGame(k >= 3, h)      k + h, + 1 under a visible step limit: 4..8 (6..8: the second record array)
 *   RL_ENV_TABULAR_MDP, 2..8 actions          n_states, + 1 under a visible step limit: 2..8; two actions too build HERE,
 *                                             with a feed-forward module on the per-layer kernels alone (a module of
 *                                             the fused shape or a recurrent one -> RL_ERR_UNSUPPORTED)
 * with any feed-forward module of obs_dim inputs and n_actions outputs (rl_mlp_create_layers: always the per-layer
 * kernels, collection step by step), or any recurrent chain of n_actions outputs from rl_rnn_chain_create (GRU or LSTM, Mlp
 * or Linear tail, 1..4 layers: collection is one launch per horizon).
 * Refused, by this entry point's name: RL_ENV_META_BANDIT lanes -> RL_ERR_UNSUPPORTED; a module that does not match the
 * env's (obs_dim, n_actions) -> RL_ERR_INVALID_ARGUMENT (more than eight actions cannot be constructed upstream).
 * rl_dqn_update of a recurrent agent on more than one rank -> RL_ERR_UNSUPPORTED before anything is changed;
 * rl_actor_to_cbor of a recurrent DqnActor -> RL_ERR_UNSUPPORTED. */
int32_t rl_dqn_create_finite(rl_env *env, rl_mlp *qnet, rl_adam *opt, const rl_dqn_config *cfg, rl_dqn **out);
int32_t rl_dqn_destroy(rl_dqn *dqn);
/* ExplorationRateSchedule::exploration_rate(global_steps, mode) (schedules.rs:35-45); training = 0 -> 0.0 */
int32_t rl_dqn_exploration_rate(const rl_dqn *dqn, int32_t training, double *rate_out);
/* DqnAgent::min_update_size (dqn.rs:207-209): the step bound of the next collection, summed over all lanes */
int32_t rl_dqn_min_update_size(const rl_dqn *dqn, uint64_t *min_steps_out, uint64_t *slack_steps_out);
typedef struct {
  double exploration_rate;
  uint64_t steps;          /* steps written (all lanes of this rank) */
  uint64_t episodes_ended; /* Terminate + Interrupt flags among them (incl. the horizon cut) */
} rl_dqn_collect_stats;
/* `horizon` env-actor steps on every lane with the epsilon-greedy actor (DqnActor::act, dqn.rs:360-379), written
 * to the replay rings.  RL_ERR_BUFFER_FULL when an episode outgrows a lane's capacity (replay.rs:93-94). */
int32_t rl_dqn_collect(rl_dqn *dqn, uint64_t horizon, rl_dqn_collect_stats *stats /* may be NULL */);
typedef struct {
  double loss_first, loss_last;
  uint64_t opt_steps;
  uint64_t global_steps;         /* after the update (dqn.rs:276) */
  uint64_t last_minibatch_steps, last_minibatch_episodes;
} rl_dqn_update_stats;
/* DqnAgent::batch_update (dqn.rs:263-337): opt_steps_per_update x {sample minibatch, targets, MSE, Adam} */
int32_t rl_dqn_update(rl_dqn *dqn, rl_dqn_update_stats *stats, float *losses_out /* may be NULL */);

/* Inspection of the replay store and of single minibatches (what the reference's tests reach through
 * ReplayBuffer::{episodes, num_steps, total_step_count}, replay.rs:52-86). */
enum { RL_REPLAY_HEAD = 0, RL_REPLAY_COUNT = 1, RL_REPLAY_EP_HEAD = 2, RL_REPLAY_EP_COUNT = 3, RL_REPLAY_TOTAL = 4,
       RL_REPLAY_EP_END = 5 /* u32 [E][n] */, RL_REPLAY_OBS = 6 /* f32 [D][C][n] */, RL_REPLAY_NEXT_OBS = 7,
       RL_REPLAY_ACTION = 8 /* u8 [C][n] */, RL_REPLAY_REWARD = 9 /* f32 [C][n] */, RL_REPLAY_FLAG = 10 /* u8 */,
       RL_REPLAY_ACTOR_POS = 11 /* u64 [n] */, RL_REPLAY_LAST_FLAGS = 12 /* u8 [T][n] of the last collection */ };
int32_t rl_dqn_replay_field_bytes(const rl_dqn *dqn, int32_t field, uint64_t *bytes);
int32_t rl_dqn_replay_read(rl_dqn *dqn, int32_t field, void *host, uint64_t bytes);
/* draw one minibatch (advances the agent Prng) and build its observation / action / target arrays;
 * `sequential` != 0 forces the one-thread sampler that the parallel one falls back to when a draw is rejected */
int32_t rl_dqn_minibatch_sample(rl_dqn *dqn, int32_t sequential, uint64_t *n_episodes_out, uint64_t *n_steps_out);
enum { RL_MB_EP_LANE = 0, RL_MB_EP_START = 1, RL_MB_EP_LEN = 2, RL_MB_EP_OFFSET = 3 /* u32 [n_episodes] */,
       RL_MB_OBS = 4 /* f32 [D][n_steps] */, RL_MB_ACTION = 5 /* u8 [n_steps] */, RL_MB_TARGET = 6 /* f32 */ };
int32_t rl_dqn_minibatch_read(rl_dqn *dqn, int32_t field, void *host, uint64_t bytes);
/* gradient of the MSE loss on the current minibatch (no parameter change) */
int32_t rl_dqn_minibatch_gradient(rl_dqn *dqn, float *grad_out, float *loss_out);
/* word position of the agent Prng (stream 0 of agent_key) */
int32_t rl_dqn_agent_rng_pos(rl_dqn *dqn, uint64_t *pos_out);

/* ---------------------------------------------------------------------------------------------
 * Step statistics of collected experience: the StepsSummary that train_parallel logs after every collection
 * (src/simulation/train.rs:160-175) and the example's evaluation prints (examples/cartpole-trpo.rs:82-93).
 *   OnlineMeanVariance<f64> (population variance; Chan et al.'s merge)   src/utils/stats.rs:11-15,119-203
 *   StepsSummary { step_feedback, episode_feedback, episode_length }      src/simulation/summary.rs:11-18
 *   OnlineStepsSummary::push                                             src/simulation/summary.rs:198-214
 *   RewardSummary (step and episode reward statistics)                   src/feedback/reward.rs:130-143
 * An rl_summary keeps, on the device, one OnlineStepsSummary per lane (the episode in progress: its length and its
 * return, f64) and the completed StepsSummary of everything pushed since the last clear.  Every pushed step adds its
 * reward (f32 widened to f64) to step_reward and to the lane's return, and 1 to the lane's length; a TERMINATE or
 * INTERRUPT successor pushes the lane's length and return as one episode and zeroes them.  Lanes persist across pushes
 * (the engine's lanes persist across periods): an episode that straddles pushes is counted once, in the push where it
 * ends, with its full length and return; the horizon cut leaves CONTINUE and ends nothing.  Results are bit-identical
 * from run to run for the same inputs and lane count (fixed merge tree, no atomics).
 * Deviation: merging with an empty side returns the other side unchanged (the reference's Add divides 0 / 0 into NaN
 * when both sides are empty, stats.rs:184-209). */
typedef struct {
  double mean;
  double squared_residual_sum;
  uint64_t count;
} rl_mean_variance; /* OnlineMeanVariance<f64>, src/utils/stats.rs:11-15 */
typedef struct {
  rl_mean_variance step_reward;
  rl_mean_variance episode_reward;
  rl_mean_variance episode_length;
} rl_steps_summary; /* StepsSummary<Reward>, src/simulation/summary.rs:11-18 */
/* per-lane carry zeroed, completed statistics empty; n_lanes = lanes of the trajectories / DQN agent pushed (this rank) */
int32_t rl_summary_create(rl_engine *engine, uint64_t n_lanes, rl_summary **out);
int32_t rl_summary_destroy(rl_summary *s);
/* OnlineStepsSummary::push for every step of the trajectory's reward and flag planes (summary.rs:198-214), time order
 * per lane.  Enqueues only (two launches on the engine's main stream); n_lanes must match.  It reads nothing but those
 * two planes, which no update writes: the intended spot is right after rl_rollout, and it may also sit between
 * rl_actor_critic_update_begin and _finish, where it does not wait for the critic chain (header above). */
int32_t rl_summary_push(rl_summary *s, const rl_traj *traj);
/* The same for the steps of the last rl_dqn_collect: successor codes from RL_REPLAY_LAST_FLAGS, each step's reward
 * from the replay record the collection wrote (ring slot (total - horizon + t) mod capacity, replay.rs:89-115).
 * RL_ERR_INVALID_ARGUMENT before the first collection or when the collection was longer than the ring. */
int32_t rl_summary_push_dqn(rl_summary *s, const rl_dqn *dqn);
/* the completed StepsSummary since the last clear (synchronises) */
int32_t rl_summary_read(rl_summary *s, rl_steps_summary *out);
/* empties the completed statistics (a new period: `OnlineStepsSummary::default().completed`); the episodes in progress
 * are kept unless forget_episodes_in_progress != 0 (after rl_env_reset: every lane starts a new episode) */
int32_t rl_summary_clear(rl_summary *s, int32_t forget_episodes_in_progress);
/* `impl Add for StepsSummary` (summary.rs; stats.rs:184-209) on the host, no engine: combines the summaries of ranks
 * or periods; `out` may alias `a` or `b` */
int32_t rl_steps_summary_merge(const rl_steps_summary *a, const rl_steps_summary *b, rl_steps_summary *out);

/* ---------------------------------------------------------------------------------------------
 * Bandit baselines on the meta-bandit lanes: the `eval` half of relearn_experiments/src/bin/rl2-bandits.rs (:166-261) —
 * a classical bandit algorithm run over RL_ENV_META_BANDIT lanes, the figure a learned RL^2 policy is judged against.
 * The actor is ResettingMetaAgent<TC> (src/agents/meta.rs:135-199) over SerialActorAgent (src/agents/serial.rs:43-95):
 * a fresh inner agent per trial, the inner actor always in Training mode, min_update_size {1, 0} — every pull updates
 * the inner agent at once.  TC by `kind`:
 *   RL_BANDIT_AGENT_RANDOM     RandomAgentConfig (src/agents/random.rs:59-73): act = IndexSpace::sample =
 *                              gen_range(0..k) (spaces/index.rs:65-67); no state
 *   RL_BANDIT_AGENT_TABULAR_Q  TabularQLearningAgentConfig { exploration_rate, initial_action_count,
 *                              initial_action_value } (src/agents/tabular.rs:21-51, 113-133, 159-180, 222-232): act
 *                              draws one gen::<f64>() — always, also at rate 0 — and takes gen_range(0..k) when the draw
 *                              is < exploration_rate, else the FIRST maximal value (ndarray-stats argmax); update, as
 *                              separate operations: count += 1; w = 1 / count; v *= 1 - w; v += w * reward (a bandit
 *                              step terminates: no successor value).  The experiment's EpsGreedy is (0.2, 2, 0.5), its
 *                              Greedy (0.0, 2, 0.5)
 *   RL_BANDIT_AGENT_UCB1       UCB1AgentConfig { exploration_rate } (src/agents/bandits/ucb.rs:106-160, 209-234): per
 *                              trial mean[a] = 0.5, count[a] = 2, visit = 2 k; act computes ucb[a] = sqrt(L /
 *                              (double)count[a]) * exploration_rate + mean[a] with L = 2.0 * ln((double)visit) and takes
 *                              the LAST maximal index (utils/iter/cmp.rs:58; a trial's first pull is arm k - 1), no
 *                              draw; update: visit += 1; count += 1; mean += (scaled - mean) / (double)count with
 *                              scaled = (reward + (-0.0)) * 1.0 (rewards declared in [0, 1], bandits.rs:161-163, 220-222)
 *   RL_BANDIT_AGENT_THOMPSON   BetaThompsonSamplingAgentConfig { num_samples } (src/agents/bandits/thompson_sampling.rs:
 *                              95-136, 186-205): per trial a low and a high reward count per arm, u64, both 1; act, for
 *                              arms 0 .. k - 1 in order, builds Beta::new((double)high, (double)low), draws num_samples
 *                              samples in sequence and sums them as 0.0 + x1 + x2 + ...; the LAST maximal sum wins
 *                              (Iterator::max_by, utils/iter/cmp.rs:68-74); update: reward > 0.5 ? high += 1 : low += 1
 *                              (the midpoint of the declared interval [0, 1], bandits.rs:161-163, 220-222).  The
 *                              experiment's TS is num_samples 1, its OTS 10 (rl2-bandits.rs:213-216).  The Beta sampler
 *                              is the engine's own statement, include/rl_beta.h: Cheng's BB / BC over rl_log / rl_exp of
 *                              rl_detmath.h and rl_u64_to_open01_f64 of rl_chacha.h, at most 64 attempts per sample,
 *                              4 words per attempt — build-defined as the Prng stream is; equality with rand_distr
 *                              0.4.3 is conditional on a check against its source, and the reference, which calls the
 *                              platform's ln / exp here, is not reproducible across libms either
 * All arithmetic is f64 in exactly these operations and this order, no contraction.  UCB1 takes `ln` of integers only
 * and never on the device: at creation the host fills L[j] = 2.0 * log((double)(2 k + j)), j = 0 .. E - 1 (E episodes
 * per trial), and the j-th pull of a trial reads L[j]; UCB1 with E > 1,048,576 -> RL_ERR_UNSUPPORTED.
 * Per step of the meta env (meta.rs:159-198): an observation that shows a finished inner episode updates the inner
 * agent with that pull, the action is some_element() = 0 and nothing is drawn (every restart step records action 0);
 * otherwise the inner actor acts.  A lane gets a fresh inner agent whenever its env state is at the start of a trial
 * (no inner episode done, no previous step, all E episodes left) — after an Interrupt's auto-reset, at the first step
 * ever and after rl_env_reset alike; a horizon that cuts a trial leaves the agent's state in the handle and the next
 * collection carries on.  Draws are sequential from the lane's ACTOR stream (ChaCha8 of seed_actor, stream = global
 * lane id): a u64 is two words, low first; gen::<f64>() is rl_u64_to_unit_f64, gen_range is rand 0.8.5's
 * UniformInt::sample_single.  The next unread word is per-lane state of the handle: 0 at creation, never rewound
 * (the policy rollouts' word t_global + t does not apply: these actors draw a varying number of words per step). */
typedef struct rl_bandit_agent rl_bandit_agent;
enum { RL_BANDIT_AGENT_RANDOM = 0, RL_BANDIT_AGENT_TABULAR_Q = 1, RL_BANDIT_AGENT_UCB1 = 2, /* 3 is left unassigned */
       RL_BANDIT_AGENT_THOMPSON = 4 };
typedef struct {
  int32_t kind;                  /* RL_BANDIT_AGENT_* */
  int32_t reserved;              /* 0 */
  double exploration_rate;       /* TABULAR_Q: epsilon; UCB1: the confidence scale; RANDOM: unused */
  uint64_t initial_action_count; /* TABULAR_Q; THOMPSON: num_samples, 1 .. 1024 */
  double initial_action_value;   /* TABULAR_Q */
} rl_bandit_agent_config;
/* the reference's Default impls: TABULAR_Q (0.2, 0, 0.0) (tabular.rs:43-51), UCB1 0.2 (ucb.rs:36-42), THOMPSON
 * num_samples 1 (thompson_sampling.rs, BetaThompsonSamplingAgentConfig::default), RANDOM nothing; an unknown kind ->
 * RL_ERR_INVALID_ARGUMENT */
int32_t rl_bandit_agent_config_default(int32_t kind, rl_bandit_agent_config *cfg);
/* The handle takes the env's lane count, arm count k and E, and owns its per-lane state and the ln table on the
 * device.  `env` must be RL_ENV_META_BANDIT (else RL_ERR_UNSUPPORTED, naming this entry point).
 * RL_ERR_INVALID_ARGUMENT, naming the field: a negative or non-finite exploration_rate / initial_action_value, a
 * TABULAR_Q exploration_rate above 1, reserved != 0, an unknown kind, a THOMPSON num_samples of 0.  A THOMPSON
 * num_samples above 1,024 -> RL_ERR_UNSUPPORTED, naming num_samples: the bound keeps the one launch's length in hand
 * on a shared device and is no limit of the reference's (the experiment uses 1 and 10). */
int32_t rl_bandit_agent_create(rl_env *env, const rl_bandit_agent_config *cfg, rl_bandit_agent **out);
int32_t rl_bandit_agent_destroy(rl_bandit_agent *agent);
/* T = the trajectory's horizon steps of every lane in one launch.  Leaves in `traj` exactly what rl_rollout leaves:
 * RL_TRAJ_OBS (slot T included), ACTION, REWARD, FLAG, TERM_OBS where a trial was cut by its Interrupt; the env's step
 * counter advances by T.  `env` must have the lanes, arms and episodes per trial the agent was made on, the trajectory
 * the env's shape (RL_ERR_INVALID_ARGUMENT). */
int32_t rl_bandit_agent_rollout(rl_bandit_agent *agent, rl_env *env, rl_traj *traj);
/* The agent's state AFTER the updates of all pulls recorded so far, lane-minor; a wrong byte count or a field the
 * kind does not have (RANDOM: only ACTOR_POS; TABULAR_Q: no VISITS, no LN_TABLE; THOMPSON: ACTOR_POS, LOW_COUNTS and
 * HIGH_COUNTS, which no other kind has) -> RL_ERR_INVALID_ARGUMENT. */
enum { RL_BANDIT_STATE_ACTOR_POS = 0 /* u64 [n]: next unread word of the lane's actor stream */,
       RL_BANDIT_STATE_COUNTS = 1 /* u64 [k][n] */, RL_BANDIT_STATE_VALUES = 2 /* f64 [k][n]: values / means */,
       RL_BANDIT_STATE_VISITS = 3 /* u64 [n] */, RL_BANDIT_STATE_LN_TABLE = 4 /* f64 [E] */,
       RL_BANDIT_STATE_LOW_COUNTS = 5 /* u64 [k][n], THOMPSON */, RL_BANDIT_STATE_HIGH_COUNTS = 6 /* u64 [k][n], THOMPSON */ };
int32_t rl_bandit_agent_state_read(rl_bandit_agent *agent, int32_t field, void *host, uint64_t bytes);

/* ---------------------------------------------------------------------------------------------
 * Actor serialisation in the reference's on-disk format: the CBOR document that
 * `serde_cbor::to_writer(file, &agent.actor(ActorMode::Evaluation))` writes (examples/cartpole-trpo.rs:71-76,
 * examples/cartpole-dqn.rs) and `serde_cbor::from_reader` loads for evaluation (:82-93).
 *   PolicyActor { observation_space, action_space, policy_module }      src/torch/agents/policies/actor.rs:10-14
 *   DqnActor { observation_space, action_space, action_value_fn, exploration_rate }  src/torch/agents/dqn.rs:340-346
 *   Mlp { layers: [Linear { kernel, bias }], activation, output_activation }         src/torch/modules/ff/mlp.rs:45-50
 *   Chain { first: RnnBase { weights { flat_weights, has_biases }, hidden_size, dropout, type_ }, second: Mlp,
 *           activation }                                  src/torch/modules/chain.rs:58-63, seq/rnn/mod.rs:90-99,186-191
 *   TensorDef { kind, shape, requires_grad, byte_order, data }                       src/torch/serialize.rs:62-81
 * observation / action spaces are those of the env the actor was trained on (NonEmptyFeatures<...>). */
enum { RL_ACTOR_POLICY = 0, RL_ACTOR_DQN = 1 };
/* Writes the document into `buf` (capacity `cap`) and its length into *len_out; with buf == NULL only the length is
 * returned.  `exploration_rate` is used by RL_ACTOR_DQN only (evaluation actors carry 0.0, schedules.rs:38). */
int32_t rl_actor_to_cbor(rl_env *env, rl_mlp *module, int32_t actor_kind, double exploration_rate, uint8_t *buf,
                         uint64_t cap, uint64_t *len_out);
/* Loads the module parameters of such a document (either actor kind) into `module`; the document's module must
 * have the handle's structure and shapes (RL_ERR_INVALID_ARGUMENT otherwise). */
int32_t rl_module_from_cbor(rl_mlp *module, const uint8_t *buf, uint64_t len);

/* The serialisation leaves on their own (host-only, no engine needed) — what every tensor and the action space of an
 * actor document are made of, and what the reference's serde_test token fixtures pin (src/torch/serialize.rs:187-352,
 * src/spaces/indexed_type.rs:409-422):
 *   TensorDef { kind: KindDef, shape: [i64], requires_grad: bool, byte_order: ByteOrder, data: bytes }
 *                                                    src/torch/serialize.rs:62-81; `impl From<&Tensor>` :83-106
 *   KindDef (remote definition of tch::Kind), variants in declaration order              src/torch/serialize.rs:12-31
 *   IndexedTypeSpace<T>: its only field is #[serde(skip)] -> a struct of length 0       src/spaces/indexed_type.rs:57-64
 * `data` holds the elements in row-major order, native (little-endian) byte order, element size of the kind.
 * Writers: buf == NULL returns the length only.  Readers refuse documents with another field order, unknown variants,
 * a non-native byte order (the reference panics there, serialize.rs:110-114) or a data length that does not match
 * shape x element size. */
typedef enum {
  RL_KIND_UINT8 = 0, RL_KIND_INT8 = 1, RL_KIND_INT16 = 2, RL_KIND_INT = 3, RL_KIND_INT64 = 4, RL_KIND_HALF = 5,
  RL_KIND_FLOAT = 6, RL_KIND_DOUBLE = 7, RL_KIND_COMPLEX_HALF = 8, RL_KIND_COMPLEX_FLOAT = 9,
  RL_KIND_COMPLEX_DOUBLE = 10, RL_KIND_BOOL = 11, RL_KIND_QINT8 = 12, RL_KIND_QUINT8 = 13, RL_KIND_QINT32 = 14,
  RL_KIND_BFLOAT16 = 15
} rl_tensor_kind;
int32_t rl_tensor_def_to_cbor(int32_t kind, const int64_t *shape, uint32_t rank, int32_t requires_grad,
                              const void *data, uint64_t data_bytes, uint8_t *buf, uint64_t cap, uint64_t *len_out);
/* shape_out receives at most shape_cap extents, data_out at most data_cap bytes (either may be NULL to query sizes
 * through rank_out / data_bytes_out) */
int32_t rl_tensor_def_from_cbor(const uint8_t *buf, uint64_t len, int32_t *kind_out, int64_t *shape_out,
                                uint32_t shape_cap, uint32_t *rank_out, int32_t *requires_grad_out, void *data_out,
                                uint64_t data_cap, uint64_t *data_bytes_out);
int32_t rl_indexed_type_space_to_cbor(uint8_t *buf, uint64_t cap, uint64_t *len_out);

/* ---------------------------------------------------------------------------------------------
 * CPU-only plumbing configuration (BASELINE.json configs[0]): examples/chain-tabular-q.rs — Chain
 * (src/envs/chain.rs:20-106) + epsilon-greedy tabular Q-learning (src/agents/tabular.rs:88-233) driven by
 * train_parallel (src/simulation/train.rs:68-186) with `n_threads` worker threads.  Runs on the host, like the
 * reference; q_values_out / counts_out are [5][2] row-major. */
int32_t rl_chain_tabular_q_train(uint64_t seed, uint64_t n_threads, uint64_t n_periods, uint64_t min_worker_steps,
                                 double exploration_rate, double *q_values_out, uint64_t *counts_out,
                                 uint64_t *total_steps_out);
/* evaluation run of examples/chain-tabular-q.rs:47-50: greedy actor, SimSeed::Root(seed), n_steps steps */
int32_t rl_chain_tabular_q_eval(const double *q_values, uint64_t seed, uint64_t n_steps, uint8_t *actions_out,
                                double *total_reward_out);

#ifdef __cplusplus
}
#endif
#endif /* RELEARN_HIP_H */
