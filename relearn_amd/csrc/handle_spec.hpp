// handle_spec.hpp — what a constructor of the C ABI decides before it allocates: which env and module shapes are refused
// and with which words, an env's D and A and the constants its kernels read, a module's parameter count and layout, its
// initial weights, and which path rl_rollout takes for a pair of the two.  Plain C++17 without a HIP
// include, so all of it runs on a machine without a GPU: tests/cpp/handle_spec_demo.cpp.  The allocating halves are
// env_build (abi_env.hip) and module_build (abi_module.hip).
// The ORDER in which a function here tests its refusals is behaviour: when two apply, the caller sees the first.
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/relearn_hip.h"
#include "../../include/rl_chacha.h"
#include "../../include/rl_detmath.h"
#include "host/envs.hpp"

struct RlError : std::runtime_error {
  int32_t code;
  RlError(int32_t c, const std::string &m) : std::runtime_error(m), code(c) {}
};

#define RL_REQUIRE(cond, msg)                                        \
  do {                                                               \
    if (!(cond)) throw RlError(RL_ERR_INVALID_ARGUMENT, (msg));      \
  } while (0)

constexpr uint32_t RL_MLP_MAX_HIDDEN = 4;   // hidden layers of a general MlpConfig
constexpr uint32_t RL_MLP_MAX_WIDTH = 256;  // widest hidden layer
constexpr uint32_t RL_MLP_MAX_OUT = 8;      // outputs of a general MLP: a categorical policy over IndexSpace::new(2..8)
constexpr uint32_t RL_TRAJ_MAX_OBS_DIM = 8;  // observation features of a trajectory (the envs here have 4 to 8)
constexpr uint32_t RL_ENV_MIN_OBS_DIM = 4;   // narrowest observation the env kernels are built for
// the wide entry points (rl_env_create_meta_bandit_wide, rl_rnn_chain_create_wide): meta-bandit lanes of up to 12 arms
// (k + 4 = 16 features) and recurrent chains of up to 16 inputs and 12 outputs on the lane-per-thread kernels.  The two
// constants above keep guarding what they guard: feed-forward modules, MemoryGame, DQN, the older constructors.
constexpr uint32_t RL_WIDE_MAX_OBS_DIM = 16;
constexpr uint32_t RL_WIDE_MAX_OUT = 12;
// the widest entry points (rl_env_create_meta_mdp_wide, rl_rnn_chain_create_wide20, rl_traj_create_wide): meta-MDP lanes
// of up to 10 states (S + A + 4 <= 20 features: DirichletRandomMdps::default's 10 x 5 has 19) and recurrent chains of up
// to 20 inputs.  RL_WIDE_MAX_OBS_DIM keeps guarding the entry points it guards.
constexpr uint32_t RL_XWIDE_MAX_OBS_DIM = 20;
// rl_env_create_partition, rl_rnn_chain_create_wide24, rl_traj_create_wide24: PartitionGame lanes (23 features, 24 under
// a visible step limit) and recurrent chains of up to 24 inputs.  RL_XWIDE_MAX_OBS_DIM keeps guarding what it guards.
constexpr uint32_t RL_PARTITION_MAX_OBS_DIM = 24;
constexpr uint32_t RL_RNN_MAX_LAYERS = 4;  // RnnBaseConfig::num_layers of a recurrent chain

// ---------------------------------------------------------------- env lanes: the struct every env kernel takes by value
// RL_ENV_TABULAR_MDP (MdpOps, env_lanes.hpp): the tables of the one MDP all lanes share, in one device allocation of the
// env handle — cum f32 [S][A][S] (running sums of the successor rows), mean and stddev f64 [S][A] — and their sizes
// (launch-uniform).  32 bytes: it lies over the bandit's eight arm values in CartPoleDev, which these lanes do not have, so
// that the struct — an argument of every env kernel — keeps its size and every field its offset.
struct MdpTablesDev {
  const float *cum;
  const double *mean, *stddev;
  uint32_t states, actions;
};

// RL_ENV_META_MDP (MetaMdpOps, env_lanes.hpp): every lane's own tables of the current trial, in one device allocation of
// the env handle — cum f32 [n][S*A][8] (a row's running sums padded to eight floats with 1.0f: one 32-byte sector; above
// eight states [n][S*A][16], MetaMdpWideOps: meta_mdp_row_floats), mean f64 [n][S*A], both indexed by the LOCAL lane
// — with the sizes and the inner step limit (launch-uniform).  The lanes write the
// tables in their reset and read them in their steps: plain pointers, never const __restrict__.  32 bytes, over the
// bandit's arm values like MdpTablesDev.
struct MetaMdpDev {
  float *cum;
  double *mean;
  uint32_t states, actions;
  uint32_t inner_steps;  // LatentStepLimit::new(L) of the inner episodes
  uint32_t pad_;
};
// ... and the distribution's four f64 parameters, over the first four cart-pole constants, which these lanes do not read
struct MetaMdpPriorDev {
  double alpha, reward_prior_mean, reward_prior_stddev, reward_stddev;
};

struct CartPoleDev {
  union {
    struct {
      double gravity, mass_pole, length_half_pole, friction_cart;
    };
    MetaMdpPriorDev mm_prior;  // RL_ENV_META_MDP
  };
  double friction_pole, time_step;
  double action_force, max_pos, max_angle;
  double total_weight, inv_total_mass, mass_length_pole;
  double init_low, init_scale;  // Uniform::new_inclusive(-0.05, 0.05)
  uint32_t key_env[8], key_actor[8];
  uint64_t lane_offset;
  uint32_t max_steps;
  int32_t limit_kind;
  uint32_t chain_size;   // RL_ENV_CHAIN / RL_ENV_MEMORY: number of states = one-hot width (MemoryGame: num_actions +
                         // history_len)
  uint32_t mem_actions;  // RL_ENV_MEMORY: num_actions (0 selects Chain in the shared lane code)
  uint32_t bandit;       // RL_ENV_BANDIT: != 0; reward = bandit_r[action], every step terminates
  union {
    float bandit_r[8];   // DeterministicBandit::from_values, 2..8 arms
    MdpTablesDev mdp;    // RL_ENV_TABULAR_MDP
    MetaMdpDev mm;       // RL_ENV_META_MDP
  };
  // RL_ENV_META_BANDIT (MetaOps, env_lanes.hpp): number of arms k (2..12; above four: rl_env_create_meta_bandit_wide)
  // and the bandit distribution (RL_BANDITS_*); `max_steps` holds TrialEpisodeLimit::episodes_per_trial (the trial limit is
  // this env's limit).  Last, so that the fields above keep their offsets in every kernel's arguments.
  uint32_t meta_arms;
  int32_t meta_dist;
};

static_assert(sizeof(MdpTablesDev) == 8 * sizeof(float) && sizeof(MetaMdpDev) == 8 * sizeof(float) &&
                  sizeof(MetaMdpPriorDev) == 4 * sizeof(double) && sizeof(CartPoleDev) == 248,
              "the tables lie over the eight arm values: the struct keeps its size");

// The tables of rl_env_create_tabular_mdp as the lanes read them (env_lanes.hpp, MdpOps), checked: `cum` [S][A][S] the f32
// running sums of the successor rows in index order (relearn::TabularMdp::cumulative, host/envs.hpp: from a row's last
// successor of positive probability on, the entries are exactly 1 — no draw reaches 1, so the rounding of a running sum,
// which may end at 1 - 1e-5, opens no bucket behind it), `mean` / `stddev` [S][A].
struct MdpTables {
  uint32_t S = 0, A = 0;  // S == 0: the env has none
  std::vector<float> cum;
  std::vector<double> mean, stddev;
};

inline MdpTables mdp_tables(const rl_env_config &cfg, const rl_tabular_mdp_config &mdp, const float *transitions,
                            const double *reward_mean, const double *reward_stddev) {
  MdpTables t;
  const uint32_t S = mdp.n_states, A = mdp.n_actions;
  if (S < 2 || S > RL_TRAJ_MAX_OBS_DIM || A < 2 || A > RL_MLP_MAX_OUT)
    throw RlError(RL_ERR_BUILD_ENV, "tabular-MDP lanes: n_states 2..8 and n_actions 2..8 (the lanes end at 8)");
  if (S + (cfg.limit_kind == RL_LIMIT_VISIBLE ? 1u : 0u) > RL_TRAJ_MAX_OBS_DIM)
    throw RlError(RL_ERR_BUILD_ENV, "tabular-MDP lanes: n_states + 1 observation features under a VisibleStepLimit, at "
                                    "most 8 in total");
  if (!std::isfinite(mdp.discount_factor))
    throw RlError(RL_ERR_BUILD_ENV, "tabular-MDP lanes: discount_factor is not finite");
  t.S = S;
  t.A = A;
  t.mean.resize((size_t)S * A);
  t.stddev.resize((size_t)S * A);
  for (uint32_t row = 0; row < S * A; ++row) {
    const std::string where = " (state " + std::to_string(row / A) + ", action " + std::to_string(row % A) + ")";
    const float *p = transitions + (size_t)row * S;
    float acc = 0.0f;
    for (uint32_t j = 0; j < S; ++j) {
      if (!std::isfinite(p[j]) || p[j] < 0.0f)
        throw RlError(RL_ERR_BUILD_ENV, "tabular-MDP lanes: a transition probability is negative or not finite" + where);
      acc = acc + p[j];
    }
    if (!(std::fabs((double)acc - 1.0) <= 1e-5))
      throw RlError(RL_ERR_BUILD_ENV, "tabular-MDP lanes: a transition row does not sum to 1 within 1e-5" + where);
    if (!std::isfinite(reward_mean[row]))
      throw RlError(RL_ERR_BUILD_ENV, "tabular-MDP lanes: a reward mean is not finite" + where);
    const double sd = reward_stddev != nullptr ? reward_stddev[row] : 1.0;  // mdps.rs:163
    if (!std::isfinite(sd) || sd < 0.0)
      throw RlError(RL_ERR_BUILD_ENV, "tabular-MDP lanes: a reward stddev is negative or not finite" + where);
    t.mean[row] = reward_mean[row];
    t.stddev[row] = sd;
  }
  // the running sums: the scalar mirror's (host/envs.hpp), one statement for both
  t.cum = relearn::TabularMdp(S, A, std::vector<float>(transitions, transitions + (size_t)S * A * S), t.mean, t.stddev).cumulative;
  return t;
}

// What env_build (abi_env.hip) allocates for: the config with the kind its constructor names, D and A, the lanes'
// constants complete but for the table pointers of dev.mdp (they point into the handle's memory), and the tables.
struct EnvSpec {
  rl_env_config cfg;
  uint32_t D, A;
  CartPoleDev dev;
  MdpTables mdp;
  uint32_t meta_mdp_rows = 0;  // RL_ENV_META_MDP: S * A rows of tables per lane (0: the env has none)
};

// the kinds rl_env_create and rl_env_create_bandit build (the other two have constructors that name them)
inline void env_check_kind(const rl_env_config &cfg) {
  if (cfg.kind == RL_ENV_META_BANDIT)
    throw RlError(RL_ERR_BUILD_ENV, "RL_ENV_META_BANDIT lanes are created by rl_env_create_meta_bandit");
  if (cfg.kind == RL_ENV_TABULAR_MDP)
    throw RlError(RL_ERR_BUILD_ENV, "RL_ENV_TABULAR_MDP lanes are created by rl_env_create_tabular_mdp");
  if (cfg.kind == RL_ENV_META_MDP)
    throw RlError(RL_ERR_BUILD_ENV, "RL_ENV_META_MDP lanes are created by rl_env_create_meta_mdp");
  if (cfg.kind == RL_ENV_PARTITION)
    throw RlError(RL_ERR_BUILD_ENV, "RL_ENV_PARTITION lanes are created by rl_env_create_partition");
  if (cfg.kind != RL_ENV_CARTPOLE && cfg.kind != RL_ENV_CHAIN && cfg.kind != RL_ENV_MEMORY && cfg.kind != RL_ENV_BANDIT)
    throw RlError(RL_ERR_BUILD_ENV, "unknown env kind");
}

// what every kind checks last, behind its own refusals: the step limit, the lane count — and only then that bandit lanes
// have no limit at all (a bandit under a limit of 0 steps, or without lanes, hears of those first)
inline void env_check_limit_and_lanes(const rl_env_config &cfg) {
  if (cfg.limit_kind != RL_LIMIT_NONE && (cfg.max_steps == 0 || cfg.max_steps >= (1ull << 32)))
    throw RlError(RL_ERR_BUILD_ENV, "step limit must be positive and < 2^32");  // StepLimit::new asserts > 0
  if (cfg.n_lanes == 0 || cfg.n_lanes >= (1ull << 31)) throw RlError(RL_ERR_BUILD_ENV, "bad n_lanes");
  if (cfg.kind == RL_ENV_BANDIT && cfg.limit_kind != RL_LIMIT_NONE)
    throw RlError(RL_ERR_BUILD_ENV, "bandit lanes take no step limit (every step ends the episode)");
}

// MemoryGame::new(num_actions, history_len) (memory.rs:40-50): num_actions + history_len states, one observation
// feature each [+ the remaining-steps feature of a VisibleStepLimit], within the widths the env kernels are built for:
// 4 (the narrowest env of this library, CartPole without a visible limit) .. 8 (the trajectory's widest observation).
// MemoryGame::default() = (2, 1) has three and stays refused (tests/test_gpu_memory.py pins that answer).  Both fields 0:
// (2, 3), the five states of the fused index-env kernels.
struct MemoryShape {
  uint64_t actions, history, states;
};
inline MemoryShape memory_shape(const rl_env_config &cfg) {
  MemoryShape m;
  m.actions = cfg.memory_num_actions ? cfg.memory_num_actions : 2;
  m.history = cfg.memory_num_actions || cfg.memory_history_len ? cfg.memory_history_len : 3;
  m.states = m.actions + m.history;
  if (cfg.kind == RL_ENV_MEMORY &&
      !(m.actions >= 2 && m.history >= 1 && m.actions <= RL_TRAJ_MAX_OBS_DIM && m.history <= RL_TRAJ_MAX_OBS_DIM &&
        m.states >= RL_ENV_MIN_OBS_DIM && m.states + (cfg.limit_kind == RL_LIMIT_VISIBLE ? 1 : 0) <= RL_TRAJ_MAX_OBS_DIM))
    throw RlError(RL_ERR_BUILD_ENV, "MemoryGame lanes: num_actions >= 2, history_len >= 1, and 4..8 observation "
                                    "features (num_actions + history_len >= 4; + 1 under a VisibleStepLimit <= 8)");
  return m;
}

// the config of a constructor that names the kind itself: whatever the caller's cfg.kind says, nothing reads it
inline rl_env_config env_config_of_kind(const rl_env_config &cfg, int32_t kind) {
  rl_env_config c = cfg;
  c.kind = kind;
  return c;
}

// the fields every kind fills the same way: the config (under the constructor's kind), the physics
// (From<PhysicalConstants> for InternalPhysicalConstants, cartpole.rs:238-251), the stream keys, the limit; everything else
// is zero for the kind's own function to assign
inline EnvSpec env_spec_begin(const rl_env_config &cfg, uint32_t D, uint32_t A) {
  EnvSpec s{};
  s.cfg = cfg;
  s.D = D;
  s.A = A;
  const rl_cartpole_params &p = cfg.cartpole;
  CartPoleDev &d = s.dev;
  d.gravity = p.gravity;
  d.mass_pole = p.mass_pole;
  d.length_half_pole = p.length_half_pole;
  d.friction_cart = p.friction_cart;
  d.friction_pole = p.friction_pole;
  d.time_step = p.time_step;
  d.action_force = p.action_force;
  d.max_pos = p.max_pos;
  d.max_angle = p.max_angle;
  const double total_mass = p.mass_cart + p.mass_pole;
  d.total_weight = p.gravity * total_mass;
  d.inv_total_mass = 1.0 / total_mass;
  d.mass_length_pole = p.mass_pole * p.length_half_pole;
  rl_seed_from_u64(cfg.seed_env, d.key_env);
  rl_seed_from_u64(cfg.seed_actor, d.key_actor);
  d.lane_offset = cfg.lane_offset;
  d.limit_kind = cfg.limit_kind;
  return s;
}

inline uint32_t env_step_limit(const rl_env_config &cfg) { return cfg.max_steps < (1ull << 32) ? (uint32_t)cfg.max_steps : 0u; }
inline uint32_t env_remaining_feature(const rl_env_config &cfg) { return cfg.limit_kind == RL_LIMIT_VISIBLE ? 1u : 0u; }

// CartPole, Chain, MemoryGame and bandit lanes once their own checks have passed.  `arm_r`: Reward -> f32 feedback, as
// every env's reward record.  Observations: CartPole's four features, or one-hot(states), [+ remaining].
inline EnvSpec env_spec_lanes(const rl_env_config &cfg, const MemoryShape &mem, uint32_t A, const float (&arm_r)[8]) {
  env_check_limit_and_lanes(cfg);
  const uint32_t n_states = cfg.kind == RL_ENV_MEMORY ? (uint32_t)mem.states : 5u;
  EnvSpec s = env_spec_begin(cfg, (cfg.kind == RL_ENV_CARTPOLE ? 4u : n_states) + env_remaining_feature(cfg), A);
  CartPoleDev &d = s.dev;
  d.init_low = -0.05;
  d.init_scale = rl_uniform_f64_inclusive_scale(-0.05, 0.05);
  d.max_steps = env_step_limit(cfg);
  d.chain_size = n_states;
  d.mem_actions = cfg.kind == RL_ENV_MEMORY ? (uint32_t)mem.actions : 0u;
  d.bandit = cfg.kind == RL_ENV_BANDIT ? 1u : 0u;
  for (uint32_t a = 0; a < 8; ++a) d.bandit_r[a] = arm_r[a];
  return s;
}

// rl_env_create: CartPole, Chain, MemoryGame, and the two-armed bandit of cfg.bandit_values
inline EnvSpec env_spec_basic(const rl_env_config &cfg) {
  env_check_kind(cfg);
  const MemoryShape mem = memory_shape(cfg);
  if (cfg.kind == RL_ENV_CHAIN && !(cfg.chain_size == 0 || cfg.chain_size == 5))
    throw RlError(RL_ERR_BUILD_ENV, "the Chain kernels are built for Chain::default (5 states)");
  const float arm_r[8] = {(float)cfg.bandit_values[0], (float)cfg.bandit_values[1], 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  return env_spec_lanes(cfg, mem, cfg.kind == RL_ENV_MEMORY ? (uint32_t)mem.actions : 2u, arm_r);
}

// rl_env_create_bandit: DeterministicBandit::from_values, 2..8 arms
inline EnvSpec env_spec_bandit(const rl_env_config &cfg, const double *values, uint32_t n_arms) {
  env_check_kind(cfg);
  const MemoryShape mem = memory_shape(cfg);  // (a MemoryGame config hears of its own shape first, then of its kind)
  if (cfg.kind != RL_ENV_BANDIT || n_arms < 2 || n_arms > 8)
    throw RlError(RL_ERR_BUILD_ENV, "bandit lanes: kind RL_ENV_BANDIT with 2..8 arm values");
  float arm_r[8];
  for (uint32_t a = 0; a < 8; ++a) arm_r[a] = a < n_arms ? (float)values[a] : 0.0f;
  return env_spec_lanes(cfg, mem, n_arms, arm_r);
}

// MetaEnv::new(distribution).wrap(TrialEpisodeLimit::new(episodes_per_trial)) (meta.rs:128-203, 541-617), whatever
// cfg.kind says.  `wide`: rl_env_create_meta_bandit_wide, whose bound and words apply above the older constructor's four
// arms; up to four it is that constructor.  Observations: MetaObservationSpace (meta.rs:357-363), n_arms + 4 features.
inline EnvSpec env_spec_meta(const rl_env_config &cfg_in, const rl_meta_bandit_config &meta, bool wide) {
  const rl_env_config cfg = env_config_of_kind(cfg_in, RL_ENV_META_BANDIT);
  if (wide && meta.n_arms > RL_TRAJ_MAX_OBS_DIM - 4) {
    if (meta.n_arms > RL_WIDE_MAX_OBS_DIM - 4)
      throw RlError(RL_ERR_BUILD_ENV, "rl_env_create_meta_bandit_wide: 2..12 arms (the observation has n_arms + 4 "
                                      "features, a trajectory of wide lanes at most 16)");
  } else if (meta.n_arms < 2 || meta.n_arms > RL_TRAJ_MAX_OBS_DIM - 4) {
    throw RlError(RL_ERR_BUILD_ENV, "meta-bandit lanes: 2..4 arms (the observation has n_arms + 4 features, a "
                                    "trajectory at most 8)");
  }
  if (meta.episodes_per_trial == 0)  // TrialEpisodeLimit::new asserts (meta.rs:548-553)
    throw RlError(RL_ERR_BUILD_ENV, "meta-bandit lanes: trials must contain at least 1 episode");
  if (meta.episodes_per_trial >= (1ull << 32))
    throw RlError(RL_ERR_BUILD_ENV, "meta-bandit lanes: episodes_per_trial must be < 2^32");
  if (meta.distribution != RL_BANDITS_UNIFORM_BERNOULLI && meta.distribution != RL_BANDITS_ONE_HOT &&
      meta.distribution != RL_BANDITS_ROUND_ROBIN)
    throw RlError(RL_ERR_BUILD_ENV, "meta-bandit lanes: unknown bandit distribution");
  if (cfg.limit_kind != RL_LIMIT_NONE)
    throw RlError(RL_ERR_BUILD_ENV, "meta-bandit lanes take no step limit (the trial's episode limit is this env's limit)");
  env_check_limit_and_lanes(cfg);
  EnvSpec s = env_spec_begin(cfg, meta.n_arms + 4, meta.n_arms);
  CartPoleDev &d = s.dev;
  // the means of UniformBernoulliBandits: Uniform::new_inclusive(0.0, 1.0) (bandits.rs:98-105); the trial's episode
  // limit in the place of the step limit
  d.init_low = 0.0;
  d.init_scale = rl_uniform_f64_inclusive_scale(0.0, 1.0);
  d.max_steps = (uint32_t)meta.episodes_per_trial;
  d.chain_size = 0;  // (no one-hot state: nothing takes these lanes for an index env of five states)
  d.bandit_r[0] = (float)cfg.bandit_values[0];  // (read by nothing on these lanes; part of the kernels' argument all the same)
  d.bandit_r[1] = (float)cfg.bandit_values[1];
  d.meta_arms = meta.n_arms;
  d.meta_dist = meta.distribution;
  return s;
}

// TabularMdp<_, Normal<f64>> (src/envs/mdps.rs:12-85) under the index lanes' step limit, whatever cfg.kind says.
// Observations: one-hot(states) [+ remaining].
inline EnvSpec env_spec_mdp(const rl_env_config &cfg_in, const rl_tabular_mdp_config &mdp, const float *transitions,
                            const double *reward_mean, const double *reward_stddev) {
  const rl_env_config cfg = env_config_of_kind(cfg_in, RL_ENV_TABULAR_MDP);
  MdpTables tables = mdp_tables(cfg, mdp, transitions, reward_mean, reward_stddev);
  env_check_limit_and_lanes(cfg);
  EnvSpec s = env_spec_begin(cfg, tables.S + env_remaining_feature(cfg), tables.A);
  CartPoleDev &d = s.dev;
  d.init_low = -0.05;
  d.init_scale = rl_uniform_f64_inclusive_scale(-0.05, 0.05);
  d.max_steps = env_step_limit(cfg);
  d.chain_size = 0;  // (as on meta lanes: nothing takes these for an index env of five states)
  d.mdp.states = tables.S;  // (over bandit_r, which these lanes do not have)
  d.mdp.actions = tables.A;
  s.mdp = std::move(tables);
  return s;
}

// MetaEnv::new(DirichletRandomMdps{..}.wrap(LatentStepLimit::new(L))).wrap(TrialEpisodeLimit::new(E)) (meta.rs:128-203,
// 541-617; mdps.rs:87-171; wrappers/step_limit.rs:13-89), whatever cfg.kind says.  Observations: MetaObservationSpace
// with the inner state's one-hot, S + A + 4 features — at most 16 through rl_env_create_meta_mdp; 10 x 5 (19) builds
// through rl_env_create_meta_mdp_wide.
constexpr uint32_t RL_META_MDP_MAX = 8;  // states, and actions
// rl_env_create_meta_mdp_wide: up to 10 states (the second row class of MetaMdpWideOps, env_lanes.hpp) and 20 features
constexpr uint32_t RL_META_MDP_WIDE_MAX_STATES = 10;
// floats of a lane's row of running sums, padded with 1.0f: one 32-byte sector up to eight states, 64 bytes beyond
inline uint32_t meta_mdp_row_floats(uint32_t S) { return S <= RL_META_MDP_MAX ? 8u : 16u; }
// `wide`: rl_env_create_meta_mdp_wide's ranges and name; inside the older ranges the two build the same spec
inline EnvSpec env_spec_meta_mdp_ranged(const rl_env_config &cfg_in, const rl_meta_mdp_config &meta, bool wide) {
  const rl_env_config cfg = env_config_of_kind(cfg_in, RL_ENV_META_MDP);
  const uint64_t S = meta.n_states, A = meta.n_actions;
  const std::string fn = wide ? "rl_env_create_meta_mdp_wide" : "rl_env_create_meta_mdp";
  if (wide) {
    if (S < 2 || S > RL_META_MDP_WIDE_MAX_STATES || A < 2 || A > RL_META_MDP_MAX || S + A + 4 > RL_XWIDE_MAX_OBS_DIM)
      throw RlError(RL_ERR_BUILD_ENV, fn + ": n_states 2..10 and n_actions 2..8 with n_states + n_actions + 4 observation "
                                           "features, at most 20");
  } else if (S < 2 || S > RL_META_MDP_MAX || A < 2 || A > RL_META_MDP_MAX || S + A + 4 > RL_WIDE_MAX_OBS_DIM)
    throw RlError(RL_ERR_BUILD_ENV, "rl_env_create_meta_mdp: n_states 2..8 and n_actions 2..8 with n_states + n_actions "
                                    "+ 4 observation features, at most 16");
  if (meta.max_inner_steps == 0 || meta.max_inner_steps >= (1ull << 32))  // StepLimit::new asserts > 0
    throw RlError(RL_ERR_BUILD_ENV, fn + ": max_inner_steps must be positive and < 2^32");
  if (meta.episodes_per_trial == 0 || meta.episodes_per_trial >= (1ull << 32))  // TrialEpisodeLimit::new (meta.rs:548-553)
    throw RlError(RL_ERR_BUILD_ENV, fn + ": episodes_per_trial must be positive and < 2^32");
  if (!std::isfinite(meta.alpha) || !(meta.alpha > 0.0))
    throw RlError(RL_ERR_BUILD_ENV, fn + ": alpha must be positive and finite");
  if (!std::isfinite(meta.reward_prior_mean))
    throw RlError(RL_ERR_BUILD_ENV, fn + ": reward_prior_mean is not finite");
  if (!std::isfinite(meta.reward_prior_stddev) || meta.reward_prior_stddev < 0.0)
    throw RlError(RL_ERR_BUILD_ENV, fn + ": reward_prior_stddev is negative or not finite");
  if (!std::isfinite(meta.reward_stddev) || meta.reward_stddev < 0.0)
    throw RlError(RL_ERR_BUILD_ENV, fn + ": reward_stddev is negative or not finite");
  if (!std::isfinite(meta.discount_factor))
    throw RlError(RL_ERR_BUILD_ENV, fn + ": discount_factor is not finite");
  if (cfg.limit_kind != RL_LIMIT_NONE)
    throw RlError(RL_ERR_BUILD_ENV, fn + ": the lanes take no step limit (the inner limit and the trial's "
                                    "episode limit are this env's limits)");
  env_check_limit_and_lanes(cfg);
  EnvSpec s = env_spec_begin(cfg, (uint32_t)(S + A + 4), (uint32_t)A);
  CartPoleDev &d = s.dev;
  d.init_low = -0.05;  // (read by nothing on these lanes)
  d.init_scale = rl_uniform_f64_inclusive_scale(-0.05, 0.05);
  d.max_steps = (uint32_t)meta.episodes_per_trial;  // the trial's episode limit in the place of the step limit
  d.chain_size = 0;  // (as on meta-bandit lanes: nothing takes these for an index env of five states)
  d.mm.cum = nullptr;  // (env_build points them into the handle's memory)
  d.mm.mean = nullptr;
  d.mm.states = (uint32_t)S;
  d.mm.actions = (uint32_t)A;
  d.mm.inner_steps = (uint32_t)meta.max_inner_steps;
  d.mm.pad_ = 0;
  d.mm_prior = MetaMdpPriorDev{meta.alpha, meta.reward_prior_mean, meta.reward_prior_stddev, meta.reward_stddev};
  s.meta_mdp_rows = (uint32_t)(S * A);
  return s;
}
inline EnvSpec env_spec_meta_mdp(const rl_env_config &cfg, const rl_meta_mdp_config &meta) {
  return env_spec_meta_mdp_ranged(cfg, meta, false);
}
// rl_env_create_meta_mdp_wide: n_states 2..10, n_actions 2..8, at most 20 features; sizes first, as the older one checks
inline EnvSpec env_spec_meta_mdp_wide(const rl_env_config &cfg, const rl_meta_mdp_config &meta) {
  return env_spec_meta_mdp_ranged(cfg, meta, true);
}

// PartitionGame (src/envs/partition.rs:11-130) under the index lanes' step limit, whatever cfg.kind says.  Observations
// (the derived space's order — spaces/tuple.rs, power.rs, option.rs:95-109, indexed_type.rs:175-187, boolean.rs:132-140):
// [element, 10] [feedback is None] [previous element, 10] [one-hot label, 2] [+ remaining]: 23 features, 24 under a
// visible limit.  Two actions (ClassifyLeft, ClassifyRight).  The lanes read the stream key and the limit alone.
constexpr uint32_t RL_PARTITION_FEATURES = 10;  // partition.rs:11 NUM_FEATURES
constexpr uint32_t RL_PARTITION_OBS_DIM = 2 * RL_PARTITION_FEATURES + 3;
inline EnvSpec env_spec_partition(const rl_env_config &cfg_in) {
  const rl_env_config cfg = env_config_of_kind(cfg_in, RL_ENV_PARTITION);
  if (cfg.limit_kind != RL_LIMIT_NONE && cfg.limit_kind != RL_LIMIT_LATENT && cfg.limit_kind != RL_LIMIT_VISIBLE)
    throw RlError(RL_ERR_BUILD_ENV, "rl_env_create_partition: limit_kind is RL_LIMIT_NONE, RL_LIMIT_LATENT or "
                                    "RL_LIMIT_VISIBLE");
  env_check_limit_and_lanes(cfg);
  EnvSpec s = env_spec_begin(cfg, RL_PARTITION_OBS_DIM + env_remaining_feature(cfg), 2);
  static_assert(RL_PARTITION_OBS_DIM + 1 == RL_PARTITION_MAX_OBS_DIM, "the widest chain and trajectory take these lanes");
  CartPoleDev &d = s.dev;
  d.init_low = -0.05;  // (read by nothing on these lanes)
  d.init_scale = rl_uniform_f64_inclusive_scale(-0.05, 0.05);
  d.max_steps = env_step_limit(cfg);
  d.chain_size = 0;  // (as on meta lanes: nothing takes these for an index env of five states)
  return s;
}

// The (S, A) shapes of RL_ENV_META_MDP lanes whose recurrent rollout is one launch (k_stack_rollout<.., MetaMdpOps, ..>,
// kernels_seq_stack.hip): the smallest, the odd widths, the default, the most features with the widest row, and the most
// actions with two head passes.  Every other shape in range runs the launch sequence per step.
struct MetaMdpShape {
  uint32_t S, A;
};
constexpr MetaMdpShape META_MDP_FUSED_SHAPES[] = {{2, 2}, {3, 2}, {4, 3}, {5, 5}, {8, 4}, {4, 8}};
inline bool meta_mdp_fused_shape(uint32_t S, uint32_t A) {
  for (const MetaMdpShape &m : META_MDP_FUSED_SHAPES)
    if (m.S == S && m.A == A) return true;
  return false;
}
// ... and of the lanes of rl_env_create_meta_mdp_wide above eight states (k_stack_rollout<.., MetaMdpWideOps, ..>): the
// reference's default size alone
constexpr MetaMdpShape META_MDP_WIDE_FUSED_SHAPES[] = {{10, 5}};
inline bool meta_mdp_wide_fused_shape(uint32_t S, uint32_t A) {
  for (const MetaMdpShape &m : META_MDP_WIDE_FUSED_SHAPES)
    if (m.S == S && m.A == A) return true;
  return false;
}

// ---------------------------------------------------------------- modules
enum { RL_MODULE_MLP = 0, RL_MODULE_GRU_MLP = 1, RL_MODULE_LSTM_MLP = 2 };
// a recurrent chain module (Chain<Gru | Lstm, Mlp>)?
inline bool rl_module_is_recurrent(int kind) { return kind == RL_MODULE_GRU_MLP || kind == RL_MODULE_LSTM_MLP; }
inline uint64_t rl_module_gates(int kind) { return kind == RL_MODULE_LSTM_MLP ? 4 : 3; }  // RnnImpl::GATES_MULTIPLE

// The shape half of a module handle (rl_mlp, engine.hpp, derives from it): what it computes and how its flat parameter
// vector is laid out.  The builders below return it checked and complete.
struct ModuleShape {
  int kind = RL_MODULE_MLP;
  uint32_t in_dim = 0, hidden = 0, out_dim = 0;  // GRU_MLP: hidden = the MLP's hidden width (0: a Linear tail, linear_tail())
  uint64_t P = 0;
  uint32_t gru_hidden = 0;
  // RnnBaseConfig::num_layers (seq/rnn/mod.rs:20-45,223-257).  > 1: stacked layers — flat order [W_ih, W_hh, b_ih, b_hh]
  // per layer (layer l > 0 reads the hidden output of layer l - 1), then the head; such a module runs the lane-per-thread
  // kernels of kernels_seq_stack.hip at its own widths (no twin).
  uint32_t rnn_layers = 1;
  // the lane-per-thread kernels run this recurrent module (stacked layers, more input features than the fused tile
  // kernels' five, or widths above their 128)
  // (or recurrent weights without bias vectors, RnnBaseConfig::bias_init = None: `has_bias` false — the gate rows then
  // start from 4 x 256 zeros kept behind the P parameters, like the bias-less MLP layers; the chain's MLP keeps its own)
  // (or a chain whose second module is one Linear, `linear_tail`: at every shape, 5 -> 128 included, and never a twin)
  // (or a chain of more than two outputs, rl_rnn_chain_create: the tile kernels and the twin stay two-action)
  bool lane_kernels() const {
    return rnn_layers > 1 || in_dim > 5 || gru_hidden > 128 || hidden > 128 || !has_bias || linear_tail() || out_dim > 2;
  }
  // ChainConfig<GruConfig | LstmConfig, LinearConfig> (modules/chain.rs:12-54): the recurrent layers -> ReLU -> one
  // Linear(gru_hidden, out_dim).  Marked by `hidden` == 0 on a recurrent kind (the MLP-tail chains have hidden >= 1);
  // flat order [layers .., kernel [out_dim][gru_hidden], bias [out_dim]]: rnn_layer_offset(rnn_layers) is the kernel.
  bool linear_tail() const { return rl_module_is_recurrent(kind) && hidden == 0; }
  uint64_t rnn_layer_offset(uint32_t l) const {  // W_ih of layer l; l == rnn_layers: the head's W1
    const uint64_t GH = rl_module_gates(kind) * (uint64_t)gru_hidden, nb = has_bias ? 2 * GH : 0;
    if (l == 0) return 0;
    return GH * (in_dim + gru_hidden) + nb + (uint64_t)(l - 1) * (GH * 2 * gru_hidden + nb);
  }
  // A recurrent chain of other widths than the tile kernels' 5 -> 128 -> 128 that still runs on them (in_dim <= 5, widths
  // <= 128): it gets a twin of the built shape, the same network embedded with zero padding (rl_mlp::exec)
  bool needs_twin() const {
    return rl_module_is_recurrent(kind) && !lane_kernels() && (in_dim != 5 || gru_hidden != 128 || hidden != 128);
  }
  // MlpConfig::hidden_sizes (ff/mlp.rs:13-34).  `general`: a shape the fused single-hidden-layer kernels do not cover
  // (no hidden layer, several, or one wider than 128) — it runs the per-layer kernels of kernels_general.hip; then
  // `hidden` is 0, which keeps every fused launcher away.
  uint32_t n_hidden = 1;
  uint32_t widths[RL_MLP_MAX_HIDDEN] = {0, 0, 0, 0};
  bool general = false;
  // MlpConfig::activation / output_activation (rl_activation); the fused kernels are built for Relu / Identity
  int act = 1, out_act = 0;
  // layer l (0 .. n_hidden; the last one is the output layer): fan-in, fan-out, offset of its kernel in the flat
  // parameter vector ([W, b] per layer, the reference's order)
  uint32_t n_layers() const { return n_hidden + 1; }
  uint32_t fan_in(uint32_t l) const { return l == 0 ? in_dim : widths[l - 1]; }
  uint32_t fan_out(uint32_t l) const { return l == n_hidden ? out_dim : widths[l]; }
  uint64_t layer_offset(uint32_t l) const {
    uint64_t o = 0;
    for (uint32_t i = 0; i < l; ++i) o += (uint64_t)fan_in(i) * fan_out(i) + (has_bias ? fan_out(i) : 0);
    return o;
  }
  // LinearConfig::bias_init = None (ff/linear.rs:13-33): layers without a bias vector — the flat vector holds the
  // kernels only.  Every layer kernel starts its dot products from `bias`; such a module's layers read it from
  // RL_MLP_MAX_WIDTH zeros kept BEHIND the P parameters in the same allocation (never written), and its gradient passes
  // skip the bias columns.  Always on the per-layer path (`general`).  On a recurrent kind: of the recurrent weights
  // (RnnBaseConfig::bias_init); the chain's MLP always has its own.
  bool has_bias = true;
  uint64_t bias_offset(uint32_t l) const { return has_bias ? layer_offset(l) + (uint64_t)fan_in(l) * fan_out(l) : P; }
  uint32_t hidden_units() const {
    uint32_t s = 0;
    for (uint32_t i = 0; i < n_hidden; ++i) s += widths[i];
    return s;
  }
  // floats of the parameter allocation: P, and behind them the zeros a module without bias vectors starts its rows from
  // (one widest layer; a recurrent one its four gates' rows)
  uint64_t alloc_floats() const {
    return P + (has_bias ? 0 : rl_module_is_recurrent(kind) ? 4 * RL_MLP_MAX_WIDTH : RL_MLP_MAX_WIDTH);
  }
};

// rl_mlp_create: one hidden layer, the fused kernels' shape
inline ModuleShape fused_mlp_shape(uint32_t in_dim, uint32_t hidden, uint32_t out_dim) {
  if (!(in_dim == 4 || in_dim == 5) || !(out_dim == 1 || out_dim == 2) || hidden == 0 || hidden > 128)
    throw RlError(RL_ERR_BUILD_AGENT, "supported MLP shapes: in_dim in {4,5}, 1 <= hidden <= 128, out_dim in {1,2}");
  ModuleShape m;
  m.in_dim = in_dim;
  m.hidden = hidden;
  m.out_dim = out_dim;
  m.widths[0] = hidden;
  m.P = (uint64_t)hidden * in_dim + hidden + (uint64_t)out_dim * hidden + out_dim;
  return m;
}

// rl_mlp_create_layers / rl_mlp_create_config (`hidden_sizes` not NULL unless n_hidden is 0)
inline ModuleShape mlp_shape(uint32_t in_dim, const uint32_t *hidden_sizes, uint32_t n_hidden, uint32_t out_dim,
                             int32_t activation, int32_t output_activation, bool has_bias) {
  // one hidden layer of at most 128 units, Relu inside and Identity on the output, with biases: the fused kernels, and
  // their constructor's bound and words (more than two outputs — a categorical policy over IndexSpace::new(3..8) — always
  // the per-layer kernels)
  if (has_bias && n_hidden == 1 && hidden_sizes[0] <= 128 && activation == RL_ACT_RELU &&
      output_activation == RL_ACT_IDENTITY && (in_dim == 4 || in_dim == 5) && out_dim <= 2)
    return fused_mlp_shape(in_dim, hidden_sizes[0], out_dim);
  // (the envs of this library have 4 or 5 features; other widths serve host-made histories: rl_traj_write)
  bool ok = in_dim >= 1 && in_dim <= RL_TRAJ_MAX_OBS_DIM && out_dim >= 1 && out_dim <= RL_MLP_MAX_OUT && n_hidden <= RL_MLP_MAX_HIDDEN;
  for (uint32_t l = 0; ok && l < n_hidden; ++l) ok = hidden_sizes[l] >= 1 && hidden_sizes[l] <= RL_MLP_MAX_WIDTH;
  if (!ok)
    throw RlError(RL_ERR_BUILD_AGENT, "supported MLP shapes: in_dim 1..8, at most 4 hidden layers of 1..256 units, "
                                      "out_dim 1..8");
  if (activation < RL_ACT_IDENTITY || activation > RL_ACT_TANH || output_activation < RL_ACT_IDENTITY ||
      output_activation > RL_ACT_TANH)
    throw RlError(RL_ERR_BUILD_AGENT, "activation / output_activation must be one of rl_activation "
                                      "(Identity, Relu, Sigmoid, Tanh)");
  ModuleShape m;
  m.in_dim = in_dim;
  m.hidden = 0;  // no fused kernel takes this module
  m.out_dim = out_dim;
  m.n_hidden = n_hidden;
  for (uint32_t l = 0; l < n_hidden; ++l) m.widths[l] = hidden_sizes[l];
  m.general = true;
  m.act = activation;
  m.out_act = output_activation;
  m.has_bias = has_bias;
  m.P = m.layer_offset(m.n_layers());
  return m;
}

// ChainConfig<GruConfig | LstmConfig, MlpConfig | LinearConfig>::build_module (modules/chain.rs:12-56, seq/rnn/mod.rs:
// 20-45,223-281): RnnBaseConfig { hidden_size, num_layers, .. } -> ReLU -> an Mlp with one hidden layer, or (mlp_hidden 0)
// one Linear(hidden_size, out_dim).  Every recurrent constructor fills an rl_rnn_chain_config and names its limits:
struct ChainLimits {
  uint32_t max_in, max_out, min_mlp_hidden;  // (min_mlp_hidden 1: the constructor has no Linear tail to offer)
  const char *refusal;
};
// in turn: rl_gru_mlp_create, rl_lstm_mlp_create, rl_rnn_mlp_create, rl_rnn_mlp_create_config; rl_rnn_linear_create;
// rl_rnn_chain_create; rl_rnn_chain_create_wide above that one's bounds
constexpr ChainLimits CHAIN_TWO_ACTIONS_MLP{
    RL_TRAJ_MAX_OBS_DIM, 2, 1,
    "supported recurrent chain shapes: in_dim 1..8, recurrent hidden 1..256, mlp_hidden 1..256, out_dim in {1,2}"};
constexpr ChainLimits CHAIN_TWO_ACTIONS_LINEAR{
    RL_TRAJ_MAX_OBS_DIM, 2, 0, "supported recurrent chain shapes: in_dim 1..8, recurrent hidden 1..256, out_dim in {1,2}"};
constexpr ChainLimits CHAIN_NARROW{
    RL_TRAJ_MAX_OBS_DIM, RL_MLP_MAX_OUT, 0,
    "supported recurrent chain shapes: in_dim 1..8, recurrent hidden 1..256, mlp_hidden 0..256, out_dim 1..8"};
constexpr ChainLimits CHAIN_WIDE{
    RL_WIDE_MAX_OBS_DIM, RL_WIDE_MAX_OUT, 0,
    "rl_rnn_chain_create_wide: in_dim 1..16, recurrent hidden 1..256, mlp_hidden 0..256, out_dim 1..12"};
constexpr ChainLimits CHAIN_WIDE20{
    RL_XWIDE_MAX_OBS_DIM, RL_WIDE_MAX_OUT, 0,
    "rl_rnn_chain_create_wide20: in_dim 1..20, recurrent hidden 1..256, mlp_hidden 0..256, out_dim 1..12"};
constexpr ChainLimits CHAIN_WIDE24{
    RL_PARTITION_MAX_OBS_DIM, RL_WIDE_MAX_OUT, 0,
    "rl_rnn_chain_create_wide24: in_dim 1..24, recurrent hidden 1..256, mlp_hidden 0..256, out_dim 1..12"};
// rl_rnn_chain_create_wide: within in_dim <= 8 and out_dim <= 8 it is rl_rnn_chain_create, bound and words
inline const ChainLimits &chain_limits_wide(const rl_rnn_chain_config &cfg) {
  return cfg.in_dim <= RL_TRAJ_MAX_OBS_DIM && cfg.out_dim <= RL_MLP_MAX_OUT ? CHAIN_NARROW : CHAIN_WIDE;
}
// rl_rnn_chain_create_wide20: at in_dim <= 16 it is rl_rnn_chain_create_wide, bound and words
inline const ChainLimits &chain_limits_wide20(const rl_rnn_chain_config &cfg) {
  return cfg.in_dim <= RL_WIDE_MAX_OBS_DIM ? chain_limits_wide(cfg) : CHAIN_WIDE20;
}
// rl_rnn_chain_create_wide24: at in_dim <= 20 it is rl_rnn_chain_create_wide20, bound and words
inline const ChainLimits &chain_limits_wide24(const rl_rnn_chain_config &cfg) {
  return cfg.in_dim <= RL_XWIDE_MAX_OBS_DIM ? chain_limits_wide20(cfg) : CHAIN_WIDE24;
}
// rl_traj_create / _wide / _wide24: the entry point a trajectory came through, and the most observation planes it takes.
// Inside the bound of the level below, a level is that level: bound and words (traj_alloc, abi_traj.hip).
enum TrajLevel { TRAJ_LEVEL_BASE = 0, TRAJ_LEVEL_WIDE = 1, TRAJ_LEVEL_WIDE24 = 2 };
inline uint32_t traj_max_obs_dim(TrajLevel level) {
  return level == TRAJ_LEVEL_WIDE24 ? RL_PARTITION_MAX_OBS_DIM : level == TRAJ_LEVEL_WIDE ? RL_XWIDE_MAX_OBS_DIM : RL_WIDE_MAX_OBS_DIM;
}

// the module kind of a config's cell; its first two refusals (tested before a NULL handle is, by every constructor that
// takes the cell and the flag from its caller)
inline int chain_kind(const rl_rnn_chain_config &cfg) {
  if (cfg.cell != RL_CELL_GRU && cfg.cell != RL_CELL_LSTM) throw RlError(RL_ERR_BUILD_AGENT, "unknown recurrent cell");
  if (cfg.rnn_bias != 0 && cfg.rnn_bias != 1) throw RlError(RL_ERR_BUILD_AGENT, "rnn_bias is 0 or 1");
  return cfg.cell == RL_CELL_GRU ? RL_MODULE_GRU_MLP : RL_MODULE_LSTM_MLP;
}

// The tile kernels are built for 5 -> 128 -> 128 -> {1, 2}; narrower shapes (in_dim <= 5, widths <= 128) run on them
// embedded with zero padding (needs_twin).  num_layers in 2..4 (stacked layers), a Linear tail, more than two outputs or
// five inputs: the lane-per-thread kernels of kernels_seq_stack.hip at the module's own widths (lane_kernels).
inline ModuleShape chain_shape(const rl_rnn_chain_config &cfg, const ChainLimits &lim) {
  ModuleShape m;
  m.kind = chain_kind(cfg);
  if (cfg.num_layers == 0) throw RlError(RL_ERR_BUILD_AGENT, "RnnBaseConfig::num_layers must be at least 1");
  if (cfg.num_layers > RL_RNN_MAX_LAYERS)
    throw RlError(RL_ERR_UNSUPPORTED, "recurrent chains are built for RnnBaseConfig::num_layers <= 4");
  if (cfg.in_dim < 1 || cfg.in_dim > lim.max_in || cfg.hidden < 1 || cfg.hidden > RL_MLP_MAX_WIDTH ||
      cfg.mlp_hidden < lim.min_mlp_hidden || cfg.mlp_hidden > RL_MLP_MAX_WIDTH || cfg.out_dim < 1 || cfg.out_dim > lim.max_out)
    throw RlError(RL_ERR_BUILD_AGENT, lim.refusal);
  m.in_dim = cfg.in_dim;
  m.gru_hidden = cfg.hidden;
  m.hidden = cfg.mlp_hidden;
  m.out_dim = cfg.out_dim;
  m.rnn_layers = cfg.num_layers;
  m.has_bias = cfg.rnn_bias != 0;
  const uint64_t H = m.gru_hidden, H2 = m.hidden, A = m.out_dim;
  m.P = m.rnn_layer_offset(m.rnn_layers) + (H2 == 0 ? A * H + A : H2 * H + H2 + A * H2 + A);
  return m;
}

// the built shape a twin has (needs_twin): every padding entry stays 0 for the life of the module
inline ModuleShape chain_twin_shape(const ModuleShape &m) {
  return chain_shape(rl_rnn_chain_config{m.kind == RL_MODULE_GRU_MLP ? RL_CELL_GRU : RL_CELL_LSTM, 5, 128, 1, 1, 128, m.out_dim},
                     CHAIN_TWO_ACTIONS_MLP);
}

// ---------------------------------------------------------------- initial parameters
// The engine's initialisation stream and TensorBuilder::build on it (initializers.rs:8-64,67-83,152-176,328-364):
// ChaCha8(seed), stream 0; one Standard f32 per uniform element, value = (2u - 1) * lim in f32; normal elements by
// Box-Muller on consecutive draw pairs (an odd count leaves the pair's second value unused); orthogonal: QR of the normal
// matrix by modified Gram-Schmidt applied twice in f64 — positive diagonal of R, so the sign fold of init_orthogonal is the
// identity.  Zeros / Constant draw nothing.  (libtorch's RNG is unseeded in the reference: the stream is engine-defined.)
struct InitStream {
  uint32_t key[8];
  uint32_t words[16];
  uint64_t widx = 0;
  explicit InitStream(uint64_t seed) { rl_seed_from_u64(seed, key); }
  float next_f32() {
    if ((widx & 15) == 0) rl_chacha_block(key, widx >> 4, 0, 4, words);
    float u = rl_u32_to_unit_f32(words[widx & 15]);
    widx += 1;
    return u;
  }
  void normals(size_t count, std::vector<double> &z) {
    z.assign(count, 0.0);
    const double two_pi = 6.283185307179586;
    for (size_t i = 0; i < count; i += 2) {
      const double u1 = (double)next_f32(), u2 = (double)next_f32();
      double rho = std::sqrt(-2.0 * std::log(1.0 - u1)), sn, cs;
      rl_sincos(two_pi * u2, &sn, &cs);
      z[i] = rho * cs;
      if (i + 1 < count) z[i + 1] = rho * sn;
    }
  }
  static double variance(const rl_initializer &it, double fan_in, double fan_out) {
    switch (it.scale) {
      case RL_SCALE_CONSTANT: return it.value;
      case RL_SCALE_FAN_IN: return 1.0 / fan_in;
      case RL_SCALE_FAN_OUT: return 1.0 / fan_out;
      default: return 2.0 / (fan_in + fan_out);
    }
  }
  // one tensor of `rows` x `cols` elements (a 1-D tensor: rows = its length, cols = 1; fan_out = shape[0] either way,
  // calculate_fan_in_and_fan_out, initializers.rs:90-103)
  void fill(const rl_initializer &it, float *dst, uint64_t rows, uint64_t cols, double fan_in) {
    const size_t count = (size_t)rows * cols;
    const double fan_out = (double)rows;
    if (it.kind == RL_INIT_ZEROS) {
      for (size_t i = 0; i < count; ++i) dst[i] = 0.0f;
    } else if (it.kind == RL_INIT_CONSTANT) {
      for (size_t i = 0; i < count; ++i) dst[i] = (float)it.value;
    } else if (it.kind == RL_INIT_UNIFORM) {
      const float lim = (float)std::sqrt(3.0 * variance(it, fan_in, fan_out));
      for (size_t i = 0; i < count; ++i) {
        float t = 2.0f * next_f32();
        t = t - 1.0f;
        dst[i] = t * lim;
      }
    } else if (it.kind == RL_INIT_NORMAL) {
      const double sd = std::sqrt(variance(it, fan_in, fan_out));
      std::vector<double> z;
      normals(count, z);
      for (size_t i = 0; i < count; ++i) dst[i] = (float)(sd * z[i]);
    } else {  // orthogonal: tall = the [rows, cols] matrix, transposed when it is wide
      std::vector<double> z;
      normals(count, z);
      const bool wide = rows < cols;
      const uint64_t R = wide ? cols : rows, Cn = wide ? rows : cols;  // tall matrix R x Cn, columns orthonormalised
      std::vector<double> a((size_t)R * Cn);                           // column-major: a[c * R + r]
      for (uint64_t r = 0; r < rows; ++r)
        for (uint64_t c = 0; c < cols; ++c) {
          const double v = z[(size_t)r * cols + c];
          if (wide) a[(size_t)r * R + c] = v;  // tall[c][r] = flat[r][c]
          else a[(size_t)c * R + r] = v;
        }
      for (uint64_t c = 0; c < Cn; ++c) {
        double *v = a.data() + (size_t)c * R;
        for (int pass = 0; pass < 2; ++pass)
          for (uint64_t q = 0; q < c; ++q) {
            const double *w = a.data() + (size_t)q * R;
            double dot = 0.0;
            for (uint64_t r = 0; r < R; ++r) dot += w[r] * v[r];
            for (uint64_t r = 0; r < R; ++r) v[r] -= dot * w[r];
          }
        double nrm = 0.0;
        for (uint64_t r = 0; r < R; ++r) nrm += v[r] * v[r];
        nrm = std::sqrt(nrm);
        for (uint64_t r = 0; r < R; ++r) v[r] /= nrm;
      }
      for (uint64_t r = 0; r < rows; ++r)
        for (uint64_t c = 0; c < cols; ++c) dst[(size_t)r * cols + c] = (float)(wide ? a[(size_t)r * R + c] : a[(size_t)c * R + r]);
    }
  }
};

// what the _init_with entry points accept of one initializer (NULL: not given, nothing to check)
inline void check_initializer(const rl_initializer *i) {
  if (i == nullptr) return;
  RL_REQUIRE(i->kind >= RL_INIT_ZEROS && i->kind <= RL_INIT_ORTHOGONAL, "unknown initializer kind");
  if (i->kind == RL_INIT_UNIFORM || i->kind == RL_INIT_NORMAL) {
    RL_REQUIRE(i->scale >= RL_SCALE_CONSTANT && i->scale <= RL_SCALE_FAN_AVG, "unknown variance scale");
    RL_REQUIRE(i->scale != RL_SCALE_CONSTANT || i->value >= 0.0, "a variance must not be negative");
  }
}

constexpr rl_initializer GLOROT_UNIFORM{RL_INIT_UNIFORM, RL_SCALE_FAN_AVG, 0.0};  // LinearConfig::default, both tensors

// Linear::new for every layer of a feed-forward module (reference src/torch/modules/ff/linear.rs:54-68) with the given
// initializers, drawn from the engine's stream in flat parameter order (kernel then bias per layer)
struct MlpInits {
  rl_initializer kernel, bias;
};
inline std::vector<float> mlp_init_vector(const ModuleShape &m, uint64_t seed, const MlpInits &in) {
  std::vector<float> h(m.P);
  InitStream st(seed);
  size_t k = 0;
  for (uint32_t l = 0; l < m.n_layers(); ++l) {
    const uint64_t fin = m.fan_in(l), fout = m.fan_out(l);
    st.fill(in.kernel, h.data() + k, fout, fin, (double)(fin + 1));  // kernel [out][in]
    k += (size_t)fin * fout;
    if (m.has_bias) {  // (LinearConfig::bias_init = None: no tensor, no draws — linear.rs:54-68)
      st.fill(in.bias, h.data() + k, fout, 1, (double)(fin + 1));  // bias [out]
      k += fout;
    }
  }
  return h;
}
// rl_mlp_init_with's arguments (`kernel_init` not NULL), checked
inline MlpInits mlp_inits_checked(const ModuleShape &m, const rl_initializer *kernel_init, const rl_initializer *bias_init) {
  if (rl_module_is_recurrent(m.kind))
    throw RlError(RL_ERR_UNSUPPORTED, "rl_mlp_init_with: feed-forward modules only (the recurrent chains use "
                                      "RnnBaseConfig::default's initializers)");
  // LinearConfig::bias_init = None <=> the module was built without bias vectors (rl_mlp_create_config, bias = 0)
  if ((bias_init == nullptr) != !m.has_bias)
    throw RlError(RL_ERR_INVALID_ARGUMENT, m.has_bias ? "this module has bias vectors: bias_init must be given (build it "
                                                        "with rl_mlp_create_config(..., bias = 0) for bias_init = None)"
                                                      : "this module has no bias vectors: bias_init must be NULL");
  for (const rl_initializer *i : {kernel_init, bias_init}) check_initializer(i);
  if (bias_init && bias_init->kind == RL_INIT_ORTHOGONAL)  // init_orthogonal asserts shape.len() >= 2 (initializers.rs:331-334)
    throw RlError(RL_ERR_INVALID_ARGUMENT, "tensor for orthogonal init must be at least 2D: not a bias initializer");
  return MlpInits{*kernel_init, bias_init ? *bias_init : *kernel_init};
}

// RnnWeights::new (seq/rnn/mod.rs:223-257: per layer W_ih [G H, layer input] from input_weights_init, W_hh [G H, H] from
// hidden_weights_init, b_ih and b_hh [G H] from bias_init — 1-D tensors: fan_in 1, fan_out G H) + the MLP's Linear::new
// layers (ff/linear.rs:54-68: kernel and bias with fan_in = in + 1), drawn in flat order from one stream.
struct RnnInits {
  rl_initializer input, hidden, bias, mlp_kernel, mlp_bias;
};
inline RnnInits rnn_default_inits() {  // RnnBaseConfig::default (seq/rnn/mod.rs:36-45), LinearConfig::default
  const rl_initializer ortho{RL_INIT_ORTHOGONAL, RL_SCALE_FAN_AVG, 0.0}, zeros{RL_INIT_ZEROS, RL_SCALE_FAN_AVG, 0.0};
  return RnnInits{GLOROT_UNIFORM, ortho, zeros, GLOROT_UNIFORM, GLOROT_UNIFORM};
}
inline std::vector<float> chain_init_vector(const ModuleShape &m, uint64_t seed, const RnnInits &in) {
  const uint64_t H = m.gru_hidden, D = m.in_dim, H2 = m.hidden, A = m.out_dim, R = rl_module_gates(m.kind) * H;
  std::vector<float> h(m.P, 0.0f);
  InitStream st(seed);
  size_t k = 0;
  for (uint32_t layer = 0; layer < m.rnn_layers; ++layer) {
    const uint64_t K = layer == 0 ? D : H;
    st.fill(in.input, h.data() + k, R, K, (double)K);
    k += R * K;
    st.fill(in.hidden, h.data() + k, R, H, (double)H);
    k += R * H;
    if (m.has_bias) {  // (RnnBaseConfig::bias_init = None: no tensors, no draws — seq/rnn/mod.rs:246-251)
      st.fill(in.bias, h.data() + k, R, 1, 1.0);
      k += R;
      st.fill(in.bias, h.data() + k, R, 1, 1.0);
      k += R;
    }
  }
  // (a Linear tail, ModuleShape::linear_tail: the one Linear(H, A))
  const uint64_t dims[2][2] = {{H, H2 == 0 ? A : H2}, {H2, A}};
  for (int l = 0; l < (H2 == 0 ? 1 : 2); ++l) {
    const uint64_t fin = dims[l][0], fout = dims[l][1];
    st.fill(in.mlp_kernel, h.data() + k, fout, fin, (double)(fin + 1));
    k += fin * fout;
    st.fill(in.mlp_bias, h.data() + k, fout, 1, (double)(fin + 1));
    k += fout;
  }
  return h;
}
// rl_rnn_mlp_init_with's arguments, checked
inline RnnInits chain_inits_checked(const ModuleShape &m, const rl_initializer *input_weights_init,
                                    const rl_initializer *hidden_weights_init, const rl_initializer *bias_init,
                                    const rl_initializer *mlp_kernel_init, const rl_initializer *mlp_bias_init) {
  if (!rl_module_is_recurrent(m.kind))
    throw RlError(RL_ERR_INVALID_ARGUMENT, "rl_rnn_mlp_init_with: recurrent chains only (rl_mlp_init_with for MLPs)");
  // RnnBaseConfig::bias_init = None <=> the module was built without recurrent bias vectors (rl_rnn_mlp_create_config)
  if ((bias_init == nullptr) != !m.has_bias)
    throw RlError(RL_ERR_INVALID_ARGUMENT, m.has_bias ? "this module has recurrent bias vectors: bias_init must be given "
                                                        "(rl_rnn_mlp_create_config(..., bias = 0, ...) builds it without)"
                                                      : "this module has no recurrent bias vectors: bias_init must be NULL");
  if (mlp_bias_init == nullptr)
    throw RlError(RL_ERR_UNSUPPORTED, "the chain's MLP is built with bias vectors: its bias_init = None is not");
  RL_REQUIRE(input_weights_init && hidden_weights_init && mlp_kernel_init, "NULL initializer");
  for (const rl_initializer *i : {input_weights_init, hidden_weights_init, bias_init, mlp_kernel_init, mlp_bias_init})
    check_initializer(i);
  if ((bias_init && bias_init->kind == RL_INIT_ORTHOGONAL) || mlp_bias_init->kind == RL_INIT_ORTHOGONAL)  // initializers.rs:331-334
    throw RlError(RL_ERR_INVALID_ARGUMENT, "tensor for orthogonal init must be at least 2D: not a bias initializer");
  return RnnInits{*input_weights_init, *hidden_weights_init, bias_init ? *bias_init : *mlp_bias_init, *mlp_kernel_init,
                  *mlp_bias_init};
}

// ---------------------------------------------------------------- rl_rollout's path for an env and a policy
enum RolloutPath {
  ROLL_GENERAL,         // launch_gen_rollout: any feed-forward module, a launch sequence per step, every env kind
  ROLL_STACK,           // launch_stack_rollout: the lane-per-thread recurrent kernels (meta-bandit lanes: one launch)
  ROLL_TILE_RECURRENT,  // launch_rollout_gru: the recurrent tile kernels, the module or its twin
  ROLL_INDEX_MLP,       // launch_rollout_chain_mlp: the fused feed-forward kernel of the five-state index envs
  ROLL_CARTPOLE,        // launch_rollout: the fused feed-forward CartPole kernel
};
// the path's launcher advances the env's step counter itself, step by step (the fused ones leave the T steps to the caller)
inline bool rollout_path_counts_steps(RolloutPath p) { return p == ROLL_GENERAL || p == ROLL_STACK; }

// the first two refusals of a pair: the policy's shape against the env's D and A (rl_rollout tests them before it notes the
// env's action count on the trajectory, the others behind that)
inline void rollout_check_shapes(uint32_t D, uint32_t A, const ModuleShape &m) {
  // (the two-action recurrent constructors' modules; a chain of rl_rnn_chain_create has one output per action)
  if (rl_module_is_recurrent(m.kind) && A > 2 && m.out_dim <= 2)
    throw RlError(RL_ERR_UNSUPPORTED, "this recurrent chain is built for two actions: the env has more");
  RL_REQUIRE(m.in_dim == D && m.out_dim == A, "policy shape does not match the env");
}

// ... and before either: PartitionGame lanes have 23 or 24 features and a feed-forward module at most eight inputs, so no
// such pair matches; it is refused by name, before a shape is compared (rl_rollout tests this first of all)
inline void rollout_check_env_kind(int env_kind, const ModuleShape &m) {
  if (env_kind == RL_ENV_PARTITION && !rl_module_is_recurrent(m.kind))
    throw RlError(RL_ERR_UNSUPPORTED, "rl_rollout: feed-forward modules are not built for RL_ENV_PARTITION lanes (a "
                                      "recurrent chain of rl_rnn_chain_create_wide24 is)");
}

inline RolloutPath rollout_path(int env_kind, uint32_t D, uint32_t A, uint32_t chain_size, const ModuleShape &m) {
  rollout_check_env_kind(env_kind, m);
  rollout_check_shapes(D, A, m);
  const bool recurrent = rl_module_is_recurrent(m.kind);
  // the fused index-env kernels are built for five states (Chain::default, MemoryGame::new(2, 3), the bandit's
  // one-hot(5)): a MemoryGame of another size steps through the standalone env kernels
  const bool fused_index_env = env_kind == RL_ENV_CARTPOLE || chain_size == 5;
  if (m.general || (!recurrent && !fused_index_env)) return ROLL_GENERAL;
  // tabular-MDP lanes: every recurrent chain, the two-output ones of the tile kernels' shapes included, steps through the
  // lane-per-thread kernels (a single-layer chain's flat order is the stacked order at one layer: stack_ensure)
  if (env_kind == RL_ENV_TABULAR_MDP && recurrent) return ROLL_STACK;
  // meta-MDP lanes likewise (one launch at the shapes of META_MDP_FUSED_SHAPES).  A feed-forward module has at most eight
  // inputs: it matches 2 x 2 alone, and went to ROLL_GENERAL above (chain_size is 0 on these lanes)
  if (env_kind == RL_ENV_META_MDP) return ROLL_STACK;
  // PartitionGame lanes likewise: one launch at 24 features, the launch sequence per step at 23
  if (env_kind == RL_ENV_PARTITION) return ROLL_STACK;
  if (!fused_index_env && !m.lane_kernels())
    throw RlError(RL_ERR_UNSUPPORTED, "the fused recurrent rollout is built for index envs of five states");
  if (recurrent && m.lane_kernels()) return ROLL_STACK;
  if (recurrent) {  // (in_dim == D here: the tile kernels compute five features)
    RL_REQUIRE(D == 5, "recurrent rollouts need an env with five observation features");
    return ROLL_TILE_RECURRENT;
  }
  return env_kind != RL_ENV_CARTPOLE ? ROLL_INDEX_MLP : ROLL_CARTPOLE;
}
