// agents.hpp — C++ host side above the C ABI: the reference's trait surface for the accelerated path, same names,
// argument meaning and error behaviour (the reference is Rust; this image has no Rust toolchain, INTEGRATION.md shows
// the equivalent `extern "C"` binding a relearn maintainer adds).  Header-only; link against librelearn_hip.so.
//
//   EnvStructure / Environment     src/envs/mod.rs:76-127,165-193     -> CartPoleLanes, ChainLanes (vectorised)
//   BuildModule, MlpConfig, GruMlpConfig   src/torch/modules/mod.rs:14, ff/mlp.rs:13-34   -> MlpConfig, GruMlpConfig
//   BuildAgent / Agent / Actor / BatchUpdate / ActorMode   src/agents/mod.rs:48-59,101-114,144,167-215
//   Policy, Critic, Optimizer, TrustRegionOptimizer (abstract; Trpo / Ppo / Reinforce, ValuesOpt / RewardToGo,
//   AdamOptimizer, ConjugateGradientOptimizer implement them)   src/torch/agents/policies/mod.rs:21-53,
//   critics/mod.rs:20-99, src/torch/optimizers/mod.rs:25-92
//   ActorCriticConfig / ActorCriticAgent   src/torch/agents/actor_critic.rs:20-136,176-211
//   TrpoConfig / PpoConfig / ReinforceConfig   src/torch/agents/policies/{trpo,ppo,reinforce}.rs
//   ValuesOptConfig / RewardToGoConfig       src/torch/agents/critics/{opt,rtg}.rs
//   DqnConfig / DqnAgent                      src/torch/agents/dqn.rs:26-140,263-337
//   StatsLogger, ChunkLogger, ByCounter / ByTime, Display / TensorBoard back ends   src/logging/ -> logging.hpp
//   train_parallel's period loop and its metric names   src/simulation/train.rs:68-186
#pragma once
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <optional>
#include <vector>

#include "../../../include/relearn_hip.h"
#include "../../../include/rl_detmath.h"
#include "logging.hpp"
#include "envs.hpp"
#include "prng.hpp"

namespace relearn {

// ---------------------------------------------------------------- errors (the reference's error enums)
struct Error : std::runtime_error {
  int32_t code;
  Error(int32_t c, const std::string &m) : std::runtime_error(m), code(c) {}
};
struct BuildAgentError : Error { using Error::Error; };        // src/agents/mod.rs:219-226
struct BuildEnvError : Error { using Error::Error; };          // src/envs/builders.rs:62-66
struct WriteExperienceFull : Error { using Error::Error; };    // WriteExperienceError::Full, buffers/mod.rs:225-228
struct OptimizerNanError : Error { using Error::Error; };      // panic in Trpo::update, policies/trpo.rs:154-162
struct NoDeviceError : Error { using Error::Error; };

inline void check(int32_t rc, const rl_engine *eng = nullptr) {
  if (rc == RL_OK) return;
  const char *m = rl_last_error(eng);
  std::string msg = m ? m : "";
  switch (rc) {
    case RL_ERR_BUILD_AGENT: throw BuildAgentError(rc, msg);
    case RL_ERR_BUILD_ENV: throw BuildEnvError(rc, msg);
    case RL_ERR_BUFFER_FULL: throw WriteExperienceFull(rc, msg);
    case RL_ERR_OPT_NAN: throw OptimizerNanError(rc, msg);
    case RL_ERR_NO_DEVICE: throw NoDeviceError(rc, msg);
    default: throw Error(rc, msg);
  }
}

// ---------------------------------------------------------------- engine + handles
class Engine {
 public:
  explicit Engine(int device = 0) { check(rl_engine_create(device, &h_)); }
  ~Engine() { rl_engine_destroy(h_); }
  Engine(const Engine &) = delete;
  Engine &operator=(const Engine &) = delete;
  rl_engine *handle() const { return h_; }
  void sync() { check(rl_engine_sync(h_), h_); }

 private:
  rl_engine *h_ = nullptr;
};

enum class ActorMode { Training, Evaluation };  // src/agents/mod.rs:144
enum class StepLimit { None = RL_LIMIT_NONE, Latent = RL_LIMIT_LATENT, Visible = RL_LIMIT_VISIBLE };

// EnvStructure of N vectorised lanes (the spaces are those of the wrapped reference env)
class EnvLanes {
 public:
  ~EnvLanes() { rl_env_destroy(h_); }
  EnvLanes(const EnvLanes &) = delete;
  EnvLanes &operator=(const EnvLanes &) = delete;
  rl_env *handle() const { return h_; }
  Engine &engine() const { return eng_; }
  uint64_t num_lanes() const { return cfg_.n_lanes; }
  uint32_t num_observation_features() const { return obs_dim_; }
  uint32_t num_actions() const { return n_actions_; }
  double discount_factor() const { return discount_; }
  // lanes of rl_env_create_tabular_mdp: DQN builds through rl_dqn_create_finite at every action count, two included
  bool tabular_mdp() const { return tabular_mdp_; }
  // Environment::{initial_state, observe, step} for every lane (src/envs/mod.rs:76-127)
  void initial_state() { check(rl_env_reset(h_), eng_.handle()); }
  std::vector<float> observe() {
    std::vector<float> obs((size_t)obs_dim_ * cfg_.n_lanes);
    check(rl_env_observe(h_, obs.data()), eng_.handle());
    return obs;
  }
  struct StepResult {
    std::vector<float> reward, next_obs, interrupt_obs;
    std::vector<uint8_t> successor;  // RL_SUCC_CONTINUE / TERMINATE / INTERRUPT
  };
  StepResult step(const std::vector<uint8_t> &actions) {
    if (actions.size() != cfg_.n_lanes) throw Error(RL_ERR_INVALID_ARGUMENT, "one action per lane");
    StepResult r;
    r.reward.resize(cfg_.n_lanes);
    r.successor.resize(cfg_.n_lanes);
    r.next_obs.resize((size_t)obs_dim_ * cfg_.n_lanes);
    r.interrupt_obs.resize((size_t)obs_dim_ * cfg_.n_lanes);
    check(rl_env_step(h_, actions.data(), r.reward.data(), r.successor.data(), r.next_obs.data(),
                      r.interrupt_obs.data()), eng_.handle());
    return r;
  }

 protected:
  EnvLanes(Engine &eng, const rl_env_config &cfg, double discount) : eng_(eng), cfg_(cfg), discount_(discount) {
    check(rl_env_create(eng.handle(), &cfg_, &h_), eng.handle());
    check(rl_env_dims(h_, &obs_dim_, &n_actions_), eng.handle());
  }
  // bandit lanes of any number of arms (rl_env_create_bandit)
  EnvLanes(Engine &eng, const rl_env_config &cfg, const std::vector<double> &arm_values, double discount)
      : eng_(eng), cfg_(cfg), discount_(discount) {
    check(rl_env_create_bandit(eng.handle(), &cfg_, arm_values.data(), (uint32_t)arm_values.size(), &h_), eng.handle());
    check(rl_env_dims(h_, &obs_dim_, &n_actions_), eng.handle());
  }
  // meta-bandit lanes (rl_env_create_meta_bandit; above four arms rl_env_create_meta_bandit_wide)
  EnvLanes(Engine &eng, const rl_env_config &cfg, const rl_meta_bandit_config &meta, double discount)
      : eng_(eng), cfg_(cfg), discount_(discount) {
    check(meta.n_arms > 4 ? rl_env_create_meta_bandit_wide(eng.handle(), &cfg_, &meta, &h_)
                          : rl_env_create_meta_bandit(eng.handle(), &cfg_, &meta, &h_),
          eng.handle());
    check(rl_env_dims(h_, &obs_dim_, &n_actions_), eng.handle());
  }
  // tabular-MDP lanes (rl_env_create_tabular_mdp); `stddev` empty: 1.0 everywhere
  EnvLanes(Engine &eng, const rl_env_config &cfg, const rl_tabular_mdp_config &mdp, const std::vector<float> &transitions,
           const std::vector<double> &mean, const std::vector<double> &stddev)
      : eng_(eng), cfg_(cfg), discount_(mdp.discount_factor), tabular_mdp_(true) {
    const size_t rows = (size_t)mdp.n_states * mdp.n_actions;
    if (transitions.size() != rows * mdp.n_states || mean.size() != rows || (!stddev.empty() && stddev.size() != rows))
      throw BuildEnvError(RL_ERR_BUILD_ENV, "TabularMdpLanes: tables of [S][A][S] and [S][A]");
    check(rl_env_create_tabular_mdp(eng.handle(), &cfg_, &mdp, transitions.data(), mean.data(),
                                    stddev.empty() ? nullptr : stddev.data(), &h_), eng.handle());
    check(rl_env_dims(h_, &obs_dim_, &n_actions_), eng.handle());
  }
  // meta-MDP lanes (rl_env_create_meta_mdp; rl_env_create_meta_mdp_wide where that one's range ends)
  EnvLanes(Engine &eng, const rl_env_config &cfg, const rl_meta_mdp_config &meta)
      : eng_(eng), cfg_(cfg), discount_(meta.discount_factor) {
    // (above eight states or sixteen features — DirichletRandomMdps::default is 10 x 5 — the wide constructor)
    const bool wide = meta.n_states > 8 || meta.n_states + meta.n_actions + 4 > 16;
    check(wide ? rl_env_create_meta_mdp_wide(eng.handle(), &cfg_, &meta, &h_)
               : rl_env_create_meta_mdp(eng.handle(), &cfg_, &meta, &h_),
          eng.handle());
    check(rl_env_dims(h_, &obs_dim_, &n_actions_), eng.handle());
  }
  // PartitionGame lanes (rl_env_create_partition); discount factor 0.999 (partition.rs:81-83)
  struct PartitionGameTag {};
  EnvLanes(Engine &eng, const rl_env_config &cfg, PartitionGameTag)
      : eng_(eng), cfg_(cfg), discount_(PartitionGame{}.discount_factor) {
    check(rl_env_create_partition(eng.handle(), &cfg_, &h_), eng.handle());
    check(rl_env_dims(h_, &obs_dim_, &n_actions_), eng.handle());
  }
  Engine &eng_;
  rl_env_config cfg_;
  rl_env *h_ = nullptr;
  uint32_t obs_dim_ = 0, n_actions_ = 0;
  double discount_;
  bool tabular_mdp_ = false;
};

// `CartPole::default().wrap(VisibleStepLimit::new(max_steps))` x n_lanes (src/envs/cartpole.rs, wrappers/step_limit.rs)
class CartPoleLanes : public EnvLanes {
 public:
  CartPoleLanes(Engine &eng, uint64_t n_lanes, uint64_t max_steps = 500, StepLimit limit = StepLimit::Visible,
                uint64_t seed_env = 0, uint64_t seed_actor = 1, uint64_t lane_offset = 0)
      : EnvLanes(eng, config(n_lanes, max_steps, limit, seed_env, seed_actor, lane_offset), 0.99) {}

 private:
  static rl_env_config config(uint64_t n, uint64_t max_steps, StepLimit limit, uint64_t se, uint64_t sa, uint64_t off) {
    rl_env_config c{};
    c.kind = RL_ENV_CARTPOLE;
    c.limit_kind = (int32_t)limit;
    c.max_steps = max_steps;
    c.n_lanes = n;
    c.lane_offset = off;
    c.seed_env = se;
    c.seed_actor = sa;
    check(rl_cartpole_params_default(&c.cartpole));
    return c;
  }
};

// `Chain::default().wrap(LatentStepLimit::new(max_steps))` x n_lanes (src/envs/chain.rs)
class ChainLanes : public EnvLanes {
 public:
  ChainLanes(Engine &eng, uint64_t n_lanes, uint64_t max_steps = 100, StepLimit limit = StepLimit::Latent,
             uint64_t seed_env = 0, uint64_t seed_actor = 1, uint64_t lane_offset = 0)
      : EnvLanes(eng, config(n_lanes, max_steps, limit, seed_env, seed_actor, lane_offset), 0.95) {}

 private:
  static rl_env_config config(uint64_t n, uint64_t max_steps, StepLimit limit, uint64_t se, uint64_t sa, uint64_t off) {
    rl_env_config c{};
    c.kind = RL_ENV_CHAIN;
    c.limit_kind = (int32_t)limit;
    c.max_steps = max_steps;
    c.n_lanes = n;
    c.lane_offset = off;
    c.seed_env = se;
    c.seed_actor = sa;
    check(rl_cartpole_params_default(&c.cartpole));
    c.chain_size = 5;
    return c;
  }
};

// `MemoryGame::new(num_actions, history_len)` x n_lanes, optionally under a step limit (src/envs/memory.rs); discount
// factor 1.0.  4 <= num_actions + history_len, (+ 1 under a visible limit) <= 8 observation features; a policy for it has
// num_actions outputs (MlpConfig::build_module(env.num_observation_features(), env.num_actions()))
class MemoryGameLanes : public EnvLanes {
 public:
  MemoryGameLanes(Engine &eng, uint64_t n_lanes, uint64_t num_actions = 2, uint64_t history_len = 3,
                  uint64_t max_steps = 0, StepLimit limit = StepLimit::None, uint64_t seed_env = 0,
                  uint64_t seed_actor = 1, uint64_t lane_offset = 0)
      : EnvLanes(eng, config(n_lanes, num_actions, history_len, max_steps, limit, seed_env, seed_actor, lane_offset),
                 1.0) {}

 private:
  static rl_env_config config(uint64_t n, uint64_t na, uint64_t hl, uint64_t max_steps, StepLimit limit, uint64_t se,
                              uint64_t sa, uint64_t off) {
    rl_env_config c{};
    c.kind = RL_ENV_MEMORY;
    c.limit_kind = (int32_t)limit;
    c.max_steps = max_steps;
    c.n_lanes = n;
    c.lane_offset = off;
    c.seed_env = se;
    c.seed_actor = sa;
    check(rl_cartpole_params_default(&c.cartpole));
    c.memory_num_actions = na;
    c.memory_history_len = hl;
    return c;
  }
};

// `DeterministicBandit::from_values(values)` x n_lanes, 2..8 arms (src/envs/bandits.rs:109-116): every step is an episode,
// reward = the chosen arm's value, discount factor 1.0 (bandits.rs:52-54).  The environment of the reference's universal
// agent test (`train_deterministic_bandit`, src/agents/testing.rs:14-64).
class DeterministicBanditLanes : public EnvLanes {
 public:
  DeterministicBanditLanes(Engine &eng, uint64_t n_lanes, double value0 = 0.0, double value1 = 1.0,
                           uint64_t seed_env = 0, uint64_t seed_actor = 1, uint64_t lane_offset = 0)
      : EnvLanes(eng, config(n_lanes, value0, value1, seed_env, seed_actor, lane_offset), 1.0) {}
  DeterministicBanditLanes(Engine &eng, uint64_t n_lanes, const std::vector<double> &values, uint64_t seed_env = 0,
                           uint64_t seed_actor = 1, uint64_t lane_offset = 0)
      : EnvLanes(eng, config(n_lanes, 0.0, 0.0, seed_env, seed_actor, lane_offset), values, 1.0) {}

 private:
  static rl_env_config config(uint64_t n, double v0, double v1, uint64_t se, uint64_t sa, uint64_t off) {
    rl_env_config c{};
    c.kind = RL_ENV_BANDIT;
    c.limit_kind = RL_LIMIT_NONE;
    c.n_lanes = n;
    c.lane_offset = off;
    c.seed_env = se;
    c.seed_actor = sa;
    check(rl_cartpole_params_default(&c.cartpole));
    c.bandit_values[0] = v0;
    c.bandit_values[1] = v1;
    return c;
  }
};

// `MetaEnv::new(D::new(n_arms)).wrap(TrialEpisodeLimit::new(episodes_per_trial))` x n_lanes (src/envs/meta.rs:128-203,
// 541-617; D: src/envs/bandits.rs:128-243), 2..12 arms, n_arms + 4 observation features: the env of
// relearn_experiments/src/bin/rl2-bandits.rs.  A trial is 2 * episodes_per_trial - 1 steps and ends in an Interrupt;
// discount factor 1.0 (bandits.rs:165-167).  Defaults: UniformBernoulliBandits::default(), TrialEpisodeLimit::default().
class MetaBanditLanes : public EnvLanes {
 public:
  MetaBanditLanes(Engine &eng, uint64_t n_lanes, uint32_t n_arms = 2, uint64_t episodes_per_trial = 10,
                  int32_t distribution = RL_BANDITS_UNIFORM_BERNOULLI, uint64_t seed_env = 0, uint64_t seed_actor = 1,
                  uint64_t lane_offset = 0)
      : EnvLanes(eng, config(n_lanes, seed_env, seed_actor, lane_offset),
                 rl_meta_bandit_config{n_arms, distribution, episodes_per_trial}, 1.0) {}

 private:
  static rl_env_config config(uint64_t n, uint64_t se, uint64_t sa, uint64_t off) {
    rl_env_config c{};
    c.kind = RL_ENV_META_BANDIT;
    c.limit_kind = RL_LIMIT_NONE;
    c.n_lanes = n;
    c.lane_offset = off;
    c.seed_env = se;
    c.seed_actor = sa;
    check(rl_cartpole_params_default(&c.cartpole));
    return c;
  }
};

// `TabularMdp { transitions, discount_factor }` x n_lanes, optionally under a step limit (src/envs/mdps.rs:12-85): ONE MDP
// of 2..8 states and 2..8 actions for all lanes, from the scalar mirror's tables (host/envs.hpp: TabularMdp, or
// DirichletRandomMdps::sample_environment(seed, stream)); n_states (+ 1 under a visible limit) <= 8 observation features.
class TabularMdpLanes : public EnvLanes {
 public:
  TabularMdpLanes(Engine &eng, uint64_t n_lanes, const TabularMdp &mdp, uint64_t max_steps = 0,
                  StepLimit limit = StepLimit::None, uint64_t seed_env = 0, uint64_t seed_actor = 1,
                  uint64_t lane_offset = 0)
      : EnvLanes(eng, config(n_lanes, max_steps, limit, seed_env, seed_actor, lane_offset),
                 rl_tabular_mdp_config{(uint32_t)mdp.num_states, (uint32_t)mdp.num_actions(), mdp.discount_factor},
                 mdp.transitions, mdp.reward_mean, mdp.reward_stddev) {}

 private:
  static rl_env_config config(uint64_t n, uint64_t max_steps, StepLimit limit, uint64_t se, uint64_t sa, uint64_t off) {
    rl_env_config c{};
    c.kind = RL_ENV_TABULAR_MDP;
    c.limit_kind = (int32_t)limit;
    c.max_steps = max_steps;
    c.n_lanes = n;
    c.lane_offset = off;
    c.seed_env = se;
    c.seed_actor = sa;
    check(rl_cartpole_params_default(&c.cartpole));
    return c;
  }
};

// `MetaEnv::new(DirichletRandomMdps{..}.wrap(LatentStepLimit::new(L))).wrap(TrialEpisodeLimit::new(E))` x n_lanes
// (src/envs/meta.rs:128-203, 541-617 over mdps.rs:87-171): the second task of the RL^2 paper.  Every lane draws its own MDP
// at each trial's start; S + A + 4 observation features, at most 20 (S up to 10); a trial is E (L + 1) - 1 steps and ends in an
// Interrupt.  `dist`: the scalar mirror's distribution (host/envs.hpp), whose sample_environment(seed_env, g) is lane g's
// first trial.  Policies: the recurrent chains of rl_rnn_chain_create_wide, above 16 features rl_rnn_chain_create_wide20.
class MetaMdpLanes : public EnvLanes {
 public:
  MetaMdpLanes(Engine &eng, uint64_t n_lanes, const DirichletRandomMdps &dist, uint64_t max_inner_steps = 10,
               uint64_t episodes_per_trial = 10, double reward_stddev = 1.0, uint64_t seed_env = 0, uint64_t seed_actor = 1,
               uint64_t lane_offset = 0)
      : EnvLanes(eng, config(n_lanes, seed_env, seed_actor, lane_offset),
                 rl_meta_mdp_config{(uint32_t)dist.num_states, (uint32_t)dist.num_actions,
                                    dist.transition_prior_dirichlet_alpha, dist.reward_prior_mean, dist.reward_prior_stddev,
                                    reward_stddev, dist.discount_factor, max_inner_steps, episodes_per_trial}),
        states_(dist.num_states), trial_steps_(episodes_per_trial * (max_inner_steps + 1) - 1) {}
  uint64_t trial_steps() const { return trial_steps_; }
  // the current trial's tables of lanes [first, first + n) as the lanes read them: running sums [n][S*A][S], means [n][S*A]
  struct Tables {
    std::vector<float> cumulative;
    std::vector<double> reward_mean;
  };
  Tables read_tables(uint64_t first, uint64_t n) {
    Tables t;
    const size_t rows = (size_t)n * states_ * n_actions_;
    t.cumulative.resize(rows * states_);
    t.reward_mean.resize(rows);
    check(rl_env_meta_mdp_read_tables(h_, first, n, t.cumulative.data(), t.reward_mean.data()), eng_.handle());
    return t;
  }

 private:
  uint64_t states_, trial_steps_;
  static rl_env_config config(uint64_t n, uint64_t se, uint64_t sa, uint64_t off) {
    rl_env_config c{};
    c.kind = RL_ENV_META_MDP;
    c.limit_kind = RL_LIMIT_NONE;
    c.n_lanes = n;
    c.lane_offset = off;
    c.seed_env = se;
    c.seed_actor = sa;
    check(rl_cartpole_params_default(&c.cartpole));
    return c;
  }
};

// `PartitionGame::default().wrap(VisibleStepLimit::new(max_steps))` x n_lanes (src/envs/partition.rs; the env of
// relearn_experiments/src/bin/partition-game.rs, whose limit is 1000): 23 observation features, 24 under a visible limit,
// two actions, discount factor 0.999.  Lane g's episodes are the scalar mirror's (host/envs.hpp: PartitionGame) on the
// generator seed_from_u64(seed_env), stream g.  Policies: the recurrent chains of rl_rnn_chain_create_wide24.
class PartitionGameLanes : public EnvLanes {
 public:
  PartitionGameLanes(Engine &eng, uint64_t n_lanes, uint64_t max_steps = 1000, StepLimit limit = StepLimit::Visible,
                     uint64_t seed_env = 0, uint64_t seed_actor = 1, uint64_t lane_offset = 0)
      : EnvLanes(eng, config(n_lanes, max_steps, limit, seed_env, seed_actor, lane_offset), PartitionGameTag{}) {}

 private:
  static rl_env_config config(uint64_t n, uint64_t max_steps, StepLimit limit, uint64_t se, uint64_t sa, uint64_t off) {
    rl_env_config c{};
    c.kind = RL_ENV_PARTITION;
    c.limit_kind = (int32_t)limit;
    c.max_steps = max_steps;
    c.n_lanes = n;
    c.lane_offset = off;
    c.seed_env = se;
    c.seed_actor = sa;
    check(rl_cartpole_params_default(&c.cartpole));
    return c;
  }
};

// ---------------------------------------------------------------- modules (BuildModule)
class Module {
 public:
  ~Module() { rl_mlp_destroy(h_); }
  Module(const Module &) = delete;
  Module &operator=(const Module &) = delete;
  rl_mlp *handle() const { return h_; }
  uint64_t num_parameters() const { return n_; }
  std::vector<float> parameters() const {  // trainable_variables() flattened, reference order
    std::vector<float> p(n_);
    check(rl_params_get(h_, p.data(), n_), eng_.handle());
    return p;
  }
  void set_parameters(const std::vector<float> &p) { check(rl_params_set(h_, p.data(), p.size()), eng_.handle()); }

 protected:
  Module(Engine &eng, rl_mlp *h) : eng_(eng), h_(h) { check(rl_mlp_num_params(h_, &n_), eng.handle()); }
  friend struct MlpConfig;
  friend struct GruMlpConfig;
  friend struct ChainLstmMlpConfig;
  friend struct GruLinearConfig;
  Engine &eng_;
  rl_mlp *h_;
  uint64_t n_ = 0;
};

enum class Activation { Identity = RL_ACT_IDENTITY, Relu = RL_ACT_RELU, Sigmoid = RL_ACT_SIGMOID, Tanh = RL_ACT_TANH };

// Initializer / VarianceScale (src/torch/initializers.rs:8-64): the C ABI's rl_initializer with the reference's names
struct Initializer {
  rl_initializer raw;
  static Initializer Zeros() { return {{RL_INIT_ZEROS, RL_SCALE_FAN_AVG, 0.0}}; }
  static Initializer Constant(double v) { return {{RL_INIT_CONSTANT, RL_SCALE_FAN_AVG, v}}; }
  static Initializer Uniform(int32_t scale = RL_SCALE_FAN_AVG, double variance = 0.0) { return {{RL_INIT_UNIFORM, scale, variance}}; }
  static Initializer Normal(int32_t scale = RL_SCALE_FAN_AVG, double variance = 0.0) { return {{RL_INIT_NORMAL, scale, variance}}; }
  static Initializer Orthogonal() { return {{RL_INIT_ORTHOGONAL, RL_SCALE_FAN_AVG, 0.0}}; }
};

struct LinearConfig {  // LinearConfig { kernel_init, bias_init } (ff/linear.rs:13-33); default: Uniform(FanAvg) both
  Initializer kernel_init = Initializer::Uniform();
  std::optional<Initializer> bias_init = Initializer::Uniform();  // nullopt: layers without a bias vector
};

struct MlpConfig {  // MlpConfig { hidden_sizes, activation, output_activation, linear_config } (ff/mlp.rs:13-34)
  std::vector<uint32_t> hidden_sizes{128};  // MlpConfig::default; any list of up to four widths <= 256 builds
  Activation activation = Activation::Relu;             // between the hidden layers (ff/activation.rs:11-27)
  Activation output_activation = Activation::Identity;  // on the output
  LinearConfig linear_config;
  // width of the single hidden layer (the recurrent chains take exactly one)
  uint32_t single_hidden_size() const {
    if (hidden_sizes.size() != 1) throw BuildAgentError(RL_ERR_BUILD_AGENT, "the chain's MLP takes one hidden layer");
    return hidden_sizes[0];
  }
  std::unique_ptr<Module> build_module(Engine &eng, uint32_t in_dim, uint32_t out_dim, uint64_t seed) const {
    rl_mlp *h = nullptr;
    check(rl_mlp_create_config(eng.handle(), in_dim, hidden_sizes.data(), (uint32_t)hidden_sizes.size(), out_dim,
                               (int32_t)activation, (int32_t)output_activation, linear_config.bias_init ? 1 : 0, &h),
          eng.handle());
    std::unique_ptr<Module> m(new Module(eng, h));
    check(rl_mlp_init_with(h, seed, &linear_config.kernel_init.raw,
                           linear_config.bias_init ? &linear_config.bias_init->raw : nullptr),
          eng.handle());
    return m;
  }
};

// RnnBaseConfig (seq/rnn/mod.rs:20-45): the layer count and the three initializers
struct RnnBaseConfig {
  uint32_t num_layers = 1;  // stacked layers: 1..4
  Initializer input_weights_init = Initializer::Uniform();     // RnnBaseConfig::default: Uniform(FanAvg)
  Initializer hidden_weights_init = Initializer::Orthogonal();
  std::optional<Initializer> bias_init = Initializer::Zeros();  // nullopt: recurrent layers without bias vectors
};
using GruConfig = RnnBaseConfig;
using LstmConfig = RnnBaseConfig;

// More than two outputs (a categorical policy over IndexSpace::new(3..8)): the one constructor that builds them,
// rl_rnn_chain_create — the two-action constructors below stay what they are for out_dim <= 2.  mlp_hidden 0: a Linear tail.
inline int32_t rnn_chain_create_multi(Engine &eng, int32_t cell, const RnnBaseConfig &first, uint32_t hidden_dim,
                                      uint32_t mlp_hidden, uint32_t in_dim, uint32_t out_dim, rl_mlp **h) {
  rl_rnn_chain_config cfg;
  cfg.cell = cell;
  cfg.in_dim = in_dim;
  cfg.hidden = hidden_dim;
  cfg.num_layers = first.num_layers;
  cfg.rnn_bias = first.bias_init ? 1 : 0;
  cfg.mlp_hidden = mlp_hidden;
  cfg.out_dim = out_dim;
  // (more than eight inputs or outputs — the rl2-bandits experiment above four arms: the wide constructor)
  // (more than sixteen inputs — the RL2 MDP experiment at 10 x 5, 19 features: rl_rnn_chain_create_wide20)
  // (more than twenty inputs — the partition-game experiment, 24 features: rl_rnn_chain_create_wide24)
  if (in_dim > 20) return rl_rnn_chain_create_wide24(eng.handle(), &cfg, h);
  if (in_dim > 16) return rl_rnn_chain_create_wide20(eng.handle(), &cfg, h);
  return in_dim > 8 || out_dim > 8 ? rl_rnn_chain_create_wide(eng.handle(), &cfg, h)
                                   : rl_rnn_chain_create(eng.handle(), &cfg, h);
}
// the shapes the two-action constructors do not take: more than two outputs, or more than eight inputs
inline bool chain_by_config(uint32_t in_dim, uint32_t out_dim) { return out_dim > 2 || in_dim > 8; }

struct GruMlpConfig {  // ChainConfig<GruConfig, MlpConfig>::default (modules/mod.rs:14, chain.rs:19-32)
  GruConfig first_config;
  uint32_t hidden_dim = 128;
  MlpConfig second_config;
  std::unique_ptr<Module> build_module(Engine &eng, uint32_t in_dim, uint32_t out_dim, uint64_t seed) const {
    rl_mlp *h = nullptr;
    check(chain_by_config(in_dim, out_dim) ? rnn_chain_create_multi(eng, RL_CELL_GRU, first_config, hidden_dim,
                                               second_config.single_hidden_size(), in_dim, out_dim, &h)
                      : rl_rnn_mlp_create_config(eng.handle(), RL_CELL_GRU, in_dim, hidden_dim, first_config.num_layers,
                                                 first_config.bias_init ? 1 : 0, second_config.single_hidden_size(),
                                                 out_dim, &h),
          eng.handle());
    std::unique_ptr<Module> m(new Module(eng, h));
    const LinearConfig &lc = second_config.linear_config;
    check(rl_rnn_mlp_init_with(h, seed, &first_config.input_weights_init.raw, &first_config.hidden_weights_init.raw,
                               first_config.bias_init ? &first_config.bias_init->raw : nullptr, &lc.kernel_init.raw,
                               lc.bias_init ? &lc.bias_init->raw : nullptr),
          eng.handle());
    return m;
  }
};

// The reference defines `pub type LstmMlpConfig = ChainConfig<GruConfig, MlpConfig>` (modules/mod.rs:15): its
// "LSTM-MLP" configuration builds the GRU chain.  Kept as is, so that a configuration written against the reference
// builds the same network here.
using LstmMlpConfig = GruMlpConfig;

// ChainConfig<LstmConfig, MlpConfig>::default (chain.rs:19-32 with Lstm = RnnBase<LstmImpl>, seq/rnn/lstm.rs:12-51): what a
// user of the reference writes out to get an actual LSTM chain.
struct ChainLstmMlpConfig {
  LstmConfig first_config;
  uint32_t hidden_dim = 128;
  MlpConfig second_config;
  std::unique_ptr<Module> build_module(Engine &eng, uint32_t in_dim, uint32_t out_dim, uint64_t seed) const {
    rl_mlp *h = nullptr;
    check(chain_by_config(in_dim, out_dim) ? rnn_chain_create_multi(eng, RL_CELL_LSTM, first_config, hidden_dim,
                                               second_config.single_hidden_size(), in_dim, out_dim, &h)
                      : rl_rnn_mlp_create_config(eng.handle(), RL_CELL_LSTM, in_dim, hidden_dim, first_config.num_layers,
                                                 first_config.bias_init ? 1 : 0, second_config.single_hidden_size(),
                                                 out_dim, &h),
          eng.handle());
    std::unique_ptr<Module> m(new Module(eng, h));
    const LinearConfig &lc = second_config.linear_config;
    check(rl_rnn_mlp_init_with(h, seed, &first_config.input_weights_init.raw, &first_config.hidden_weights_init.raw,
                               first_config.bias_init ? &first_config.bias_init->raw : nullptr, &lc.kernel_init.raw,
                               lc.bias_init ? &lc.bias_init->raw : nullptr),
          eng.handle());
    return m;
  }
};

// ChainConfig<GruConfig | LstmConfig, LinearConfig> (modules/chain.rs:12-54): the recurrent layers -> ReLU -> ONE
// Linear(hidden_dim, out) — the model of the reference's rl2-bandits experiment (rl2-bandits.rs:349,379-394).  A Linear
// without a bias vector (LinearConfig::bias_init = None) is not built.
struct GruLinearConfig {
  GruConfig first_config;
  uint32_t hidden_dim = 128;
  LinearConfig second_config;
  std::unique_ptr<Module> build_module(Engine &eng, uint32_t in_dim, uint32_t out_dim, uint64_t seed) const {
    return build(eng, RL_CELL_GRU, first_config, hidden_dim, second_config, in_dim, out_dim, seed);
  }
  // (both cells: ChainLstmLinearConfig builds through it)
  static std::unique_ptr<Module> build(Engine &eng, int32_t cell, const RnnBaseConfig &first, uint32_t hidden_dim,
                                       const LinearConfig &second, uint32_t in_dim, uint32_t out_dim, uint64_t seed) {
    if (!second.bias_init)
      throw BuildAgentError(RL_ERR_BUILD_AGENT, "a recurrent chain's Linear tail is built with a bias vector");
    rl_mlp *h = nullptr;
    check(chain_by_config(in_dim, out_dim) ? rnn_chain_create_multi(eng, cell, first, hidden_dim, 0, in_dim, out_dim, &h)
                      : rl_rnn_linear_create(eng.handle(), cell, in_dim, hidden_dim, first.num_layers,
                                             first.bias_init ? 1 : 0, out_dim, &h),
          eng.handle());
    std::unique_ptr<Module> m(new Module(eng, h));
    check(rl_rnn_mlp_init_with(h, seed, &first.input_weights_init.raw, &first.hidden_weights_init.raw,
                               first.bias_init ? &first.bias_init->raw : nullptr, &second.kernel_init.raw,
                               &second.bias_init->raw),
          eng.handle());
    return m;
  }
};
struct ChainLstmLinearConfig {
  LstmConfig first_config;
  uint32_t hidden_dim = 128;
  LinearConfig second_config;
  std::unique_ptr<Module> build_module(Engine &eng, uint32_t in_dim, uint32_t out_dim, uint64_t seed) const {
    return GruLinearConfig::build(eng, RL_CELL_LSTM, first_config, hidden_dim, second_config, in_dim, out_dim, seed);
  }
};

// Is the module a configuration builds a sequence module with a state of its own (the recurrent chains)?  DqnConfig over
// one builds its agent through rl_dqn_create_recurrent (dqn.rs:75-86: VB::Module: SeqPacked + SeqIterative).
template <typename VB>
struct builds_recurrent_module : std::false_type {};
template <>
struct builds_recurrent_module<GruMlpConfig> : std::true_type {};
template <>
struct builds_recurrent_module<ChainLstmMlpConfig> : std::true_type {};
template <>
struct builds_recurrent_module<GruLinearConfig> : std::true_type {};
template <>
struct builds_recurrent_module<ChainLstmLinearConfig> : std::true_type {};

// ---------------------------------------------------------------- optimizers (src/torch/optimizers/mod.rs:25-92)
// `Optimizer` (first-order: backward_step) and `TrustRegionOptimizer` (trust_region_backward_step) are the reference's
// two optimizer traits; the update loops that drive them live in the library, so an implementation here hands the
// library what it needs: the device optimizer state, or the trust-region solver's settings.
class Optimizer {
 public:
  virtual ~Optimizer() = default;
  virtual rl_adam *handle() const = 0;  // device state of the rule (moments, step count)
};
class TrustRegionOptimizer {
 public:
  virtual ~TrustRegionOptimizer() = default;
  // fill the solver's part of a trust-region step (the caller sets the constraint bound)
  virtual void configure(rl_trpo_config &c) const = 0;
};

class AdamOptimizer final : public Optimizer {  // COptimizer over torch's Adam (optimizers/coptimizer.rs:16-110)
 public:
  AdamOptimizer(Module &m, Engine &eng, const rl_adam_config &c) { check(rl_adam_create(m.handle(), &c, &h_), eng.handle()); }
  ~AdamOptimizer() override { rl_adam_destroy(h_); }
  AdamOptimizer(const AdamOptimizer &) = delete;
  AdamOptimizer &operator=(const AdamOptimizer &) = delete;
  rl_adam *handle() const override { return h_; }

 private:
  rl_adam *h_ = nullptr;
};

struct AdamConfig {  // optimizers/coptimizer.rs:136-156
  double learning_rate = 1e-3, beta1 = 0.9, beta2 = 0.999, weight_decay = 0.0;
  std::unique_ptr<Optimizer> build_optimizer(Module &m, Engine &eng) const {  // BuildOptimizer::build_optimizer
    rl_adam_config c;
    check(rl_adam_config_default(&c));
    c.learning_rate = learning_rate;
    c.beta1 = beta1;
    c.beta2 = beta2;
    c.weight_decay = weight_decay;
    return std::unique_ptr<Optimizer>(new AdamOptimizer(m, eng, c));
  }
};

// The other three COptimizer configurations (coptimizer.rs:49-132, 170-205): the same handle type with another rule
// (rl_optimizer_create), so the update loops take them unchanged.
class RuleOptimizer final : public Optimizer {
 public:
  RuleOptimizer(Module &m, Engine &eng, const rl_optimizer_config &c) {
    check(rl_optimizer_create(m.handle(), &c, &h_), eng.handle());
  }
  ~RuleOptimizer() override { rl_adam_destroy(h_); }
  RuleOptimizer(const RuleOptimizer &) = delete;
  RuleOptimizer &operator=(const RuleOptimizer &) = delete;
  rl_adam *handle() const override { return h_; }

 private:
  rl_adam *h_ = nullptr;
};

struct SgdConfig {  // optimizers/coptimizer.rs:49-87
  double learning_rate = 1e-2, momentum = 0.0, weight_decay = 0.0, dampening = 0.0;
  bool nesterov = false;
  std::unique_ptr<Optimizer> build_optimizer(Module &m, Engine &eng) const {
    rl_optimizer_config c;
    check(rl_optimizer_config_default(RL_OPTIMIZER_SGD, &c));
    c.learning_rate = learning_rate;
    c.momentum = momentum;
    c.weight_decay = weight_decay;
    c.dampening = dampening;
    c.nesterov = nesterov ? 1 : 0;
    return std::unique_ptr<Optimizer>(new RuleOptimizer(m, eng, c));
  }
};

struct RmsPropConfig {  // optimizers/coptimizer.rs:89-132
  double learning_rate = 1e-2, momentum = 0.0, alpha = 0.99, eps = 1e-8;
  bool centered = false;
  double weight_decay = 0.0;
  std::unique_ptr<Optimizer> build_optimizer(Module &m, Engine &eng) const {
    rl_optimizer_config c;
    check(rl_optimizer_config_default(RL_OPTIMIZER_RMSPROP, &c));
    c.learning_rate = learning_rate;
    c.momentum = momentum;
    c.alpha = alpha;
    c.eps = eps;
    c.centered = centered ? 1 : 0;
    c.weight_decay = weight_decay;
    return std::unique_ptr<Optimizer>(new RuleOptimizer(m, eng, c));
  }
};

struct AdamWConfig {  // optimizers/coptimizer.rs:170-205
  double learning_rate = 1e-3, beta1 = 0.9, beta2 = 0.999, weight_decay = 0.0;
  std::unique_ptr<Optimizer> build_optimizer(Module &m, Engine &eng) const {
    rl_optimizer_config c;
    check(rl_optimizer_config_default(RL_OPTIMIZER_ADAMW, &c));
    c.learning_rate = learning_rate;
    c.beta1 = beta1;
    c.beta2 = beta2;
    c.weight_decay = weight_decay;
    return std::unique_ptr<Optimizer>(new RuleOptimizer(m, eng, c));
  }
};

// ---------------------------------------------------------------- device-resident history (VecBuffer's stand-in)
class DeviceHistory {
 public:
  DeviceHistory(Engine &eng, uint64_t n_lanes, uint64_t horizon, uint32_t obs_dim) : n_(n_lanes), T_(horizon) {
    // (more than sixteen planes — the meta-MDP lanes of 10 x 5 — are rl_traj_create_wide's)
    // (more than twenty — the PartitionGame lanes — rl_traj_create_wide24's)
    check(obs_dim > 20   ? rl_traj_create_wide24(eng.handle(), n_lanes, horizon, obs_dim, &h_)
          : obs_dim > 16 ? rl_traj_create_wide(eng.handle(), n_lanes, horizon, obs_dim, &h_)
                         : rl_traj_create(eng.handle(), n_lanes, horizon, obs_dim, &h_),
          eng.handle());
  }
  ~DeviceHistory() { rl_traj_destroy(h_); }
  DeviceHistory(const DeviceHistory &) = delete;
  DeviceHistory &operator=(const DeviceHistory &) = delete;
  rl_traj *handle() const { return h_; }
  uint64_t num_steps() const { return n_ * T_; }
  uint64_t num_lanes() const { return n_; }
  uint64_t horizon() const { return T_; }
  std::vector<uint8_t> successors() const {
    std::vector<uint8_t> f(n_ * T_);
    check(rl_traj_read(h_, RL_TRAJ_FLAG, f.data(), f.size()));
    return f;
  }

 private:
  rl_traj *h_ = nullptr;
  uint64_t n_, T_;
};

// ---------------------------------------------------------------- step statistics (src/simulation/summary.rs)
// OnlineMeanVariance<f64> (src/utils/stats.rs:11-15,93-118): population variance; no value while empty
struct MeanVariance {
  rl_mean_variance s{};
  uint64_t count() const { return s.count; }
  std::optional<double> mean() const { return s.count ? std::optional<double>(s.mean) : std::nullopt; }
  std::optional<double> variance() const {
    return s.count ? std::optional<double>(s.squared_residual_sum / (double)s.count) : std::nullopt;
  }
  std::optional<double> stddev() const {
    const auto v = variance();
    return v ? std::optional<double>(std::sqrt(*v)) : std::nullopt;
  }
  // `impl Display` (stats.rs:28-46) with `{:.precision}`: "(μ = m; σ = s; n = c)", "-" for a missing value
  std::string display(int precision) const {
    auto num = [precision](const std::optional<double> &v) {
      if (!v) return std::string("-");
      char buf[64];
      std::snprintf(buf, sizeof buf, "%.*f", precision, *v);
      return std::string(buf);
    };
    return "(\u03bc = " + num(mean()) + "; \u03c3 = " + num(stddev()) + "; n = " + std::to_string(count()) + ")";
  }
};

// StepsSummary<Reward> (summary.rs:11-18): statistics of the step rewards, episode rewards and episode lengths
struct StepsSummary {
  MeanVariance step_reward, episode_reward, episode_length;
  StepsSummary() = default;
  explicit StepsSummary(const rl_steps_summary &s) {
    step_reward.s = s.step_reward;
    episode_reward.s = s.episode_reward;
    episode_length.s = s.episode_length;
  }
  rl_steps_summary raw() const { return rl_steps_summary{step_reward.s, episode_reward.s, episode_length.s}; }
  uint64_t num_steps() const { return step_reward.count(); }
  uint64_t num_episodes() const { return episode_length.count(); }
  // `impl Add` (summary.rs; stats.rs:184-209): ranks or periods combined; an empty side returns the other side
  StepsSummary operator+(const StepsSummary &o) const {
    const rl_steps_summary a = raw(), b = o.raw();
    rl_steps_summary r{};
    check(rl_steps_summary_merge(&a, &b, &r));
    return StepsSummary(r);
  }
  // `impl Display` (summary.rs:37-52), as examples/cartpole-trpo.rs:92 prints it with {:.3}
  std::string display(int precision) const {
    return "step_feedback: " + step_reward.display(precision) + "\nepisode_feedback: " +
           episode_reward.display(precision) + "\nepisode_length: " + episode_length.display(precision);
  }
  // train.rs:160-175 under the "sim" scope: ep/fbk/reward/{mean,stddev}, ep/length_{mean,stddev} (when an episode
  // ended), ep/count, step/fbk/reward/{mean,stddev} (RewardSummary::log, feedback/reward.rs:130-143), step/count
  void log(StatsLogger &sim) const {
    ScopedLogger ep(sim, "ep");
    if (num_episodes() > 0) {
      ep.log_scalar("fbk/reward/mean", *episode_reward.mean());
      ep.log_scalar("fbk/reward/stddev", *episode_reward.stddev());
      ep.log_scalar("length_mean", *episode_length.mean());
      ep.log_scalar("length_stddev", *episode_length.stddev());
    }
    ep.log_counter_increment("count", num_episodes());
    ScopedLogger step(sim, "step");
    if (num_steps() > 0) {
      step.log_scalar("fbk/reward/mean", *step_reward.mean());
      step.log_scalar("fbk/reward/stddev", *step_reward.stddev());
    }
    step.log_counter_increment("count", num_steps());
  }
};

// One OnlineStepsSummary per lane (summary.rs:166-214) kept on the device, plus the completed StepsSummary of everything
// pushed since the last clear (rl_summary_*).  Lanes persist across pushes: an episode is counted where it ends.
class StepsSummaryLanes {
 public:
  StepsSummaryLanes(Engine &eng, uint64_t n_lanes) : eng_(eng) {
    check(rl_summary_create(eng.handle(), n_lanes, &h_), eng.handle());
  }
  ~StepsSummaryLanes() { rl_summary_destroy(h_); }
  StepsSummaryLanes(const StepsSummaryLanes &) = delete;
  StepsSummaryLanes &operator=(const StepsSummaryLanes &) = delete;
  rl_summary *handle() const { return h_; }
  void push(const DeviceHistory &history) { check(rl_summary_push(h_, history.handle()), eng_.handle()); }
  void push_dqn(const rl_dqn *dqn) { check(rl_summary_push_dqn(h_, dqn), eng_.handle()); }
  StepsSummary read() const {
    rl_steps_summary s{};
    check(rl_summary_read(h_, &s), eng_.handle());
    return StepsSummary(s);
  }
  // a new period (the episodes in progress are kept); forget = true also drops them (after an env reset)
  void clear(bool forget_episodes_in_progress = false) {
    check(rl_summary_clear(h_, forget_episodes_in_progress ? 1 : 0), eng_.handle());
  }

 private:
  Engine &eng_;
  rl_summary *h_ = nullptr;
};

// ---------------------------------------------------------------- policies and critics
struct ConjugateGradientOptimizerConfig;
class ConjugateGradientOptimizer final : public TrustRegionOptimizer {  // conjugate_gradient.rs:67-260
 public:
  ConjugateGradientOptimizer(uint64_t iterations, uint64_t max_backtracks, double backtrack_ratio, double hpv_reg_coeff,
                             bool accept_violation)
      : iterations_(iterations), max_backtracks_(max_backtracks), backtrack_ratio_(backtrack_ratio),
        hpv_reg_coeff_(hpv_reg_coeff), accept_violation_(accept_violation) {}
  void configure(rl_trpo_config &c) const override {
    c.iterations = iterations_;
    c.max_backtracks = max_backtracks_;
    c.backtrack_ratio = backtrack_ratio_;
    c.hpv_reg_coeff = hpv_reg_coeff_;
    c.accept_violation = accept_violation_ ? 1 : 0;
  }

 private:
  uint64_t iterations_, max_backtracks_;
  double backtrack_ratio_, hpv_reg_coeff_;
  bool accept_violation_;
};
struct ConjugateGradientOptimizerConfig {  // conjugate_gradient.rs:41-65
  uint64_t iterations = 10, max_backtracks = 15;
  double backtrack_ratio = 0.8, hpv_reg_coeff = 1e-5;
  bool accept_violation = false;
  std::unique_ptr<TrustRegionOptimizer> build_optimizer() const {
    return std::unique_ptr<TrustRegionOptimizer>(
        new ConjugateGradientOptimizer(iterations, max_backtracks, backtrack_ratio, hpv_reg_coeff, accept_violation));
  }
};

enum class PolicyKind { Trpo, Ppo, Reinforce };

// Policy (src/torch/agents/policies/mod.rs:21-53): a module and the rule that improves it from a history whose
// advantages are in place.  `update` logs what the reference's implementation logs, under the caller's scope.
class Policy {
 public:
  virtual ~Policy() = default;
  virtual PolicyKind kind() const = 0;
  virtual void update(DeviceHistory &history, StatsLogger &logger) = 0;
  Module &module() { return *module_; }  // AsModule::as_module
  int32_t last_status() const { return last_status_; }  // OptimizerStepError of the last update, RL_OPT_OK otherwise

 protected:
  Policy(Engine &eng, std::unique_ptr<Module> m) : eng_(eng), module_(std::move(m)) {}
  Engine &eng_;
  std::unique_ptr<Module> module_;
  int32_t last_status_ = RL_OPT_OK;
};

class Trpo final : public Policy {  // policies/trpo.rs:63-164
 public:
  Trpo(Engine &eng, std::unique_ptr<Module> m, std::unique_ptr<TrustRegionOptimizer> opt, double max_policy_step_kl)
      : Policy(eng, std::move(m)), optimizer_(std::move(opt)) {
    check(rl_trpo_config_default(&cfg_));
    optimizer_->configure(cfg_);
    cfg_.max_policy_step_kl = max_policy_step_kl;
  }
  PolicyKind kind() const override { return PolicyKind::Trpo; }
  void update(DeviceHistory &history, StatsLogger &logger) override {
    rl_trpo_stats st{};
    check(rl_trpo_update(module_->handle(), history.handle(), &cfg_, &st), eng_.handle());  // OptimizerNanError: the
                                                                                           // reference panics (trpo.rs:154-162)
    log_stats(st, logger);
  }
  const rl_trpo_config &config() const { return cfg_; }
  void log_stats(const rl_trpo_stats &st, StatsLogger &logger) {
    logger.log_scalar("entropy", st.entropy);                  // trpo.rs:119
    logger.log_scalar("step_size", st.step_size);              // conjugate_gradient.rs:164
    logger.log_scalar("loss_initial", st.loss_initial);        // :200
    if (st.num_backtracks >= 0) {
      logger.log_scalar("num_backtracks", (double)st.num_backtracks);  // :219
      logger.log_scalar("step_scale", st.step_scale);                  // :220
    }
    logger.log_scalar("loss_final", st.loss_final);            // :225
    logger.log_scalar("constraint_val_final", st.constraint_val_final);  // :226
    last_status_ = st.status;  // OptimizerStepError::{LossNotImproving, ConstraintViolated}: warn and continue
  }

 private:
  std::unique_ptr<TrustRegionOptimizer> optimizer_;
  rl_trpo_config cfg_{};
};

class Ppo final : public Policy {  // policies/ppo.rs:63-137
 public:
  Ppo(Engine &eng, std::unique_ptr<Module> m, std::unique_ptr<Optimizer> opt, uint64_t opt_steps_per_update,
      double clip_distance)
      : Policy(eng, std::move(m)), optimizer_(std::move(opt)) {
    cfg_.opt_steps_per_update = opt_steps_per_update;
    cfg_.clip_distance = clip_distance;
  }
  PolicyKind kind() const override { return PolicyKind::Ppo; }
  void update(DeviceHistory &history, StatsLogger &logger) override {
    rl_policy_opt_stats st{};
    check(rl_ppo_update(module_->handle(), optimizer_->handle(), history.handle(), &cfg_, &st, nullptr), eng_.handle());
    logger.log_scalar("entropy", st.entropy);  // ppo.rs:114 (ToLog::NoAbsLoss: no final loss)
  }

 private:
  std::unique_ptr<Optimizer> optimizer_;
  rl_ppo_config cfg_{};
};

class Reinforce final : public Policy {  // policies/reinforce.rs:40-90
 public:
  Reinforce(Engine &eng, std::unique_ptr<Module> m, std::unique_ptr<Optimizer> opt)
      : Policy(eng, std::move(m)), optimizer_(std::move(opt)) {}
  PolicyKind kind() const override { return PolicyKind::Reinforce; }
  void update(DeviceHistory &history, StatsLogger &logger) override {
    rl_policy_opt_stats st{};
    check(rl_reinforce_update(module_->handle(), optimizer_->handle(), history.handle(), &st), eng_.handle());
    logger.log_scalar("loss", st.loss_first);
    logger.log_scalar("entropy", st.entropy);  // reinforce.rs:84
  }

 private:
  std::unique_ptr<Optimizer> optimizer_;
};

template <typename MB = MlpConfig>
struct TrpoConfig {  // policies/trpo.rs:18-41
  MB policy_fn_config;
  ConjugateGradientOptimizerConfig optimizer_config;
  double max_policy_step_kl = 0.01;
  std::unique_ptr<Policy> build_policy(Engine &eng, uint32_t in_dim, uint32_t out_dim, uint64_t seed) const {
    return std::unique_ptr<Policy>(new Trpo(eng, policy_fn_config.build_module(eng, in_dim, out_dim, seed),
                                            optimizer_config.build_optimizer(), max_policy_step_kl));
  }
};
template <typename MB = MlpConfig, typename OC = AdamConfig>
struct PpoConfig {  // policies/ppo.rs:13-41
  MB policy_fn_config;
  OC optimizer_config;
  uint64_t opt_steps_per_update = 10;
  double clip_distance = 0.2;
  std::unique_ptr<Policy> build_policy(Engine &eng, uint32_t in_dim, uint32_t out_dim, uint64_t seed) const {
    std::unique_ptr<Module> m = policy_fn_config.build_module(eng, in_dim, out_dim, seed);
    std::unique_ptr<Optimizer> o = optimizer_config.build_optimizer(*m, eng);
    return std::unique_ptr<Policy>(new Ppo(eng, std::move(m), std::move(o), opt_steps_per_update, clip_distance));
  }
};
template <typename MB = MlpConfig, typename OC = AdamConfig>
struct ReinforceConfig {  // policies/reinforce.rs
  MB policy_fn_config;
  OC optimizer_config;
  std::unique_ptr<Policy> build_policy(Engine &eng, uint32_t in_dim, uint32_t out_dim, uint64_t seed) const {
    std::unique_ptr<Module> m = policy_fn_config.build_module(eng, in_dim, out_dim, seed);
    std::unique_ptr<Optimizer> o = optimizer_config.build_optimizer(*m, eng);
    return std::unique_ptr<Policy>(new Reinforce(eng, std::move(m), std::move(o)));
  }
};

// Critic (src/torch/agents/critics/mod.rs:20-99): turns a history into per-step advantages for the policy and
// improves itself from the same history afterwards.
class Critic {
 public:
  virtual ~Critic() = default;
  virtual void advantages(DeviceHistory &history) = 0;                    // Critic::advantages
  virtual void update(DeviceHistory &history, StatsLogger &logger) = 0;   // Critic::update
  virtual Module *module() { return nullptr; }                            // a critic may have no trainable state
  virtual double discount_factor() const = 0;
};

enum class StepValueTarget { RewardToGo, OneStepTd };  // critics/mod.rs:203-215 (default RewardToGo)

class ValuesOpt final : public Critic {  // critics/opt.rs:41-126
 public:
  ValuesOpt(Engine &eng, std::unique_ptr<Module> m, std::unique_ptr<Optimizer> opt, double discount_factor,
            double gae_lambda, StepValueTarget target, uint64_t opt_steps_per_update)
      : eng_(eng), module_(std::move(m)), optimizer_(std::move(opt)), gamma_((float)discount_factor),
        lambda_(gae_lambda), target_(target), steps_(opt_steps_per_update) {}
  void advantages(DeviceHistory &history) override {
    check(rl_gae(history.handle(), module_->handle(), gamma_, (float)lambda_), eng_.handle());
  }
  void update(DeviceHistory &history, StatsLogger &logger) override {
    // ValuesOpt::update (critics/opt.rs:100-126): targets once under no-grad, then n_backward_steps
    rl_critic_stats cs{};
    rl_values_opt_config vc{};
    vc.opt_steps_per_update = steps_;
    vc.target = target_ == StepValueTarget::OneStepTd ? RL_VALUE_TARGET_ONE_STEP_TD : RL_VALUE_TARGET_REWARD_TO_GO;
    vc.discount_factor = gamma_;
    check(rl_values_opt_update(module_->handle(), optimizer_->handle(), history.handle(), &vc, &cs, nullptr), eng_.handle());
    logger.log_scalar("loss", cs.loss_last);  // n_backward_steps, ToLog::All (torch/agents/mod.rs:68-70)
  }
  rl_values_opt_config config() const {
    rl_values_opt_config vc{};
    vc.opt_steps_per_update = steps_;
    vc.target = target_ == StepValueTarget::OneStepTd ? RL_VALUE_TARGET_ONE_STEP_TD : RL_VALUE_TARGET_REWARD_TO_GO;
    vc.discount_factor = gamma_;
    return vc;
  }
  Optimizer &optimizer() { return *optimizer_; }
  Module *module() override { return module_.get(); }
  double discount_factor() const override { return gamma_; }

 private:
  Engine &eng_;
  std::unique_ptr<Module> module_;
  std::unique_ptr<Optimizer> optimizer_;
  float gamma_;
  double lambda_;
  StepValueTarget target_;
  uint64_t steps_;
};

class RewardToGo final : public Critic {  // critics/rtg.rs:22-40
 public:
  RewardToGo(Engine &eng, double discount_factor) : eng_(eng), gamma_((float)discount_factor) {}
  void advantages(DeviceHistory &history) override { check(rl_reward_to_go(history.handle(), gamma_), eng_.handle()); }
  void update(DeviceHistory &, StatsLogger &) override {}  // RewardToGo::update does nothing
  double discount_factor() const override { return gamma_; }

 private:
  Engine &eng_;
  float gamma_;
};

template <typename MB = MlpConfig, typename OC = AdamConfig>
struct ValuesOptConfig {  // critics/opt.rs:13-37
  MB state_value_fn_config;
  OC optimizer_config;
  double gae_lambda = 0.95;          // AdvantageFn::Gae { lambda }
  StepValueTarget target = StepValueTarget::RewardToGo;
  uint64_t opt_steps_per_update = 80;
  double max_discount_factor = 0.99;
  std::unique_ptr<Critic> build_critic(Engine &eng, uint32_t in_dim, double env_discount_factor, uint64_t seed) const {
    std::unique_ptr<Module> m = state_value_fn_config.build_module(eng, in_dim, 1, seed);
    std::unique_ptr<Optimizer> o = optimizer_config.build_optimizer(*m, eng);
    const double g = env_discount_factor < max_discount_factor ? env_discount_factor : max_discount_factor;  // opt.rs:73
    return std::unique_ptr<Critic>(new ValuesOpt(eng, std::move(m), std::move(o), g, gae_lambda, target, opt_steps_per_update));
  }
};
struct RewardToGoConfig {  // critics/rtg.rs:14-20
  std::unique_ptr<Critic> build_critic(Engine &eng, uint32_t, double env_discount_factor, uint64_t) const {
    return std::unique_ptr<Critic>(new RewardToGo(eng, env_discount_factor));
  }
};

// ---------------------------------------------------------------- Actor (src/agents/mod.rs:101-114)
// `act(episode_state, observation, rng) -> action`, one observation at a time.  The batched rollouts are the fast
// path (`ActorCriticAgent::collect`); this is the reference's per-step interface for a caller that steps its own
// environment.  The random state belongs to the caller, as in the reference.
class Actor {
 public:
  virtual ~Actor() = default;
  virtual uint32_t act(const std::vector<float> &observation_features, Prng &rng) = 0;
};

// PolicyActor (policies/actor.rs:30-56) over a feed-forward policy module: logits from the device module,
// Categorical::new (log_softmax) and the inverse-CDF draw of the rollouts (`log_probs.exp().multinomial(1)` with an
// explicit uniform from `rng`; same arithmetic as device_fns.hpp, include/rl_detmath.h).  With `rng` at word t of
// stream `lane` of the env's actor seed this returns exactly the action the device rollout takes for that lane and
// step.  Recurrent modules carry their episode state on the device: they act through the rollouts only.
class PolicyActor final : public Actor {
 public:
  PolicyActor(Engine &eng, Module &policy_module, uint32_t in_dim, uint32_t n_actions)
      : eng_(eng), module_(policy_module), in_dim_(in_dim), n_actions_(n_actions) {}
  uint32_t act(const std::vector<float> &x, Prng &rng) override {
    if (x.size() != in_dim_) throw Error(RL_ERR_INVALID_ARGUMENT, "observation has the wrong number of features");
    std::vector<float> z(n_actions_), lp(n_actions_);
    check(rl_mlp_forward(module_.handle(), x.data(), 1, z.data()), eng_.handle());
    float m = z[0];
    for (uint32_t a = 1; a < n_actions_; ++a)
      if (z[a] > m) m = z[a];
    float s = 0.0f;
    for (uint32_t a = 0; a < n_actions_; ++a) s += rl_expf(z[a] - m);
    const float ls = rl_logf(s);
    for (uint32_t a = 0; a < n_actions_; ++a) lp[a] = (z[a] - m) - ls;
    const float u = rng.gen_f32();
    float cum = 0.0f;
    for (uint32_t a = 0; a + 1 < n_actions_; ++a) {
      cum += rl_expf(lp[a]);
      if (u < cum) return a;
    }
    return n_actions_ - 1;  // the last index absorbs rounding
  }

 private:
  Engine &eng_;
  Module &module_;
  uint32_t in_dim_, n_actions_;
};

template <typename P, typename C>
struct ActorCriticConfig;

// ActorCriticAgent (actor_critic.rs:72-136) over a Policy and a Critic; `batch_update` follows batch_update_slice
// (actor_critic.rs:176-211): advantages, policy update, critic update, with the reference's metric names.
class ActorCriticAgent {
 public:
  Policy &policy() { return *policy_; }
  Critic &critic() { return *critic_; }
  Module &policy_module() { return policy_->module(); }
  Module *critic_module() { return critic_->module(); }
  // Agent::actor(mode): the policy module is the actor's state (both modes sample from the policy's distribution,
  // policies/mod.rs:42-53); the returned actor acts one observation at a time, `collect` is the batched form
  std::unique_ptr<Actor> actor(ActorMode) {
    return std::unique_ptr<Actor>(new PolicyActor(eng_, policy_->module(), obs_dim_, n_actions_));
  }
  DeviceHistory buffer(uint64_t horizon) const { return DeviceHistory(eng_, n_lanes_, horizon, obs_dim_); }

  // BatchUpdate::batch_update
  void batch_update(DeviceHistory &history, StatsLogger &logger) {
    log_elapsed(logger, "adv_est_time", [&] {
      critic_->advantages(history);
      eng_.sync();
    });
    ScopedLogger pl(logger, "policy");
    ScopedLogger cl(logger, "critic");
    Trpo *trpo = dynamic_cast<Trpo *>(policy_.get());
    ValuesOpt *vopt = dynamic_cast<ValuesOpt *>(critic_.get());
    if (trpo != nullptr && vopt != nullptr) {
      // policy.update and critic.update share nothing but the history and its advantages: one call, the two launch chains
      // side by side on two streams (rl_actor_critic_update; the same numbers as the two updates in turn).  Both scopes
      // log the joint wall time as their update_time.
      rl_trpo_stats ps{};
      rl_critic_stats cs{};
      const rl_values_opt_config vc = vopt->config();
      const auto t0 = std::chrono::steady_clock::now();
      check(rl_actor_critic_update(trpo->module().handle(), vopt->module()->handle(), vopt->optimizer().handle(),
                                   history.handle(), &trpo->config(), &vc, &ps, &cs, nullptr),
            eng_.handle());
      const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      trpo->log_stats(ps, pl);
      pl.log_duration("update_time", secs);
      cl.log_scalar("loss", cs.loss_last);
      cl.log_duration("update_time", secs);
      return;
    }
    log_elapsed(pl, "update_time", [&] { policy_->update(history, pl); eng_.sync(); });
    log_elapsed(cl, "update_time", [&] { critic_->update(history, cl); });
  }

  // one data-collection pass of every lane with the current policy (train.rs:124-158's thread fan-out)
  void collect(EnvLanes &env, DeviceHistory &history) {
    check(rl_rollout(env.handle(), policy_->module().handle(), history.handle()), eng_.handle());
  }
  int32_t last_status() const { return policy_->last_status(); }

 private:
  template <typename P, typename C>
  friend struct ActorCriticConfig;
  ActorCriticAgent(Engine &eng) : eng_(eng) {}
  Engine &eng_;
  std::unique_ptr<Policy> policy_;
  std::unique_ptr<Critic> critic_;
  uint64_t n_lanes_ = 0;
  uint32_t obs_dim_ = 0, n_actions_ = 0;
};

template <typename P, typename C>
struct ActorCriticConfig {  // actor_critic.rs:20-45
  P policy_config;
  C critic_config;

  // BuildAgent::build_agent(env, rng): `seed` seeds the engine-defined initialisation streams
  std::unique_ptr<ActorCriticAgent> build_agent(EnvLanes &env, uint64_t seed) const {
    Engine &eng = env.engine();
    std::unique_ptr<ActorCriticAgent> a(new ActorCriticAgent(eng));
    a->n_lanes_ = env.num_lanes();
    a->obs_dim_ = env.num_observation_features();
    a->n_actions_ = env.num_actions();
    a->policy_ = policy_config.build_policy(eng, env.num_observation_features(), env.num_actions(), seed);
    a->critic_ = critic_config.build_critic(eng, env.num_observation_features(), env.discount_factor(), seed + 1);
    return a;
  }
};

// ---------------------------------------------------------------- DQN (src/torch/agents/dqn.rs)
template <typename VB = MlpConfig, typename OC = AdamConfig>
struct DqnConfig {  // dqn.rs:26-72
  VB action_value_fn_config;
  OC optimizer_config;
  bool one_step_td = false;  // StepValueTarget::{RewardToGo, OneStepTd}
  double exploration_start = 1.0, exploration_end = 0.1;
  uint64_t exploration_period = 10000000;
  uint64_t minibatch_steps = 100000, opt_steps_per_update = 50;
  uint64_t buffer_capacity = 10000000;  // TOTAL steps; divided over the lanes (each lane is one ReplayBuffer)
  uint64_t update_first = 1000000, update_rest = 100000;  // DataCollectionSchedule::FirstRest
};

class DqnAgent;
template <typename VB, typename OC>
std::unique_ptr<DqnAgent> build_dqn_agent(const DqnConfig<VB, OC> &c, EnvLanes &env, uint64_t seed, const uint32_t (&agent_key)[8]);

class DqnAgent {
 public:
  ~DqnAgent() { rl_dqn_destroy(dqn_); }  // before the optimizer and the module it refers to
  Module &action_value_fn() { return *q_; }
  rl_dqn *handle() const { return dqn_; }
  struct Bound { uint64_t min_steps, slack_steps; };
  Bound min_update_size() const {  // dqn.rs:207-209
    Bound b{};
    check(rl_dqn_min_update_size(dqn_, &b.min_steps, &b.slack_steps), eng_.handle());
    return b;
  }
  double exploration_rate(ActorMode mode) const {
    double r = 0.0;
    check(rl_dqn_exploration_rate(dqn_, mode == ActorMode::Training ? 1 : 0, &r), eng_.handle());
    return r;
  }
  // every lane takes ceil(min_steps / lanes) steps with the epsilon-greedy actor (HistoryDataBound::divide)
  void collect(StatsLogger &logger) {
    const Bound b = min_update_size();
    const uint64_t horizon = (b.min_steps + n_lanes_ - 1) / n_lanes_;
    rl_dqn_collect_stats st{};
    check(rl_dqn_collect(dqn_, horizon, &st), eng_.handle());  // WriteExperienceFull when an episode outgrows a lane
    ScopedLogger sim(logger, "sim");
    sim.log_counter_increment("step/count", st.steps);           // train.rs:175
    sim.log_counter_increment("ep/count", st.episodes_ended);    // train.rs:171
  }
  // the same collection with the period's StepsSummary (train.rs:160-175) from the device: pushes the collection into
  // `summary`, logs the full set and clears the completed statistics (the episodes in progress carry over)
  void collect(StatsLogger &logger, StepsSummaryLanes &summary) {
    const Bound b = min_update_size();
    const uint64_t horizon = (b.min_steps + n_lanes_ - 1) / n_lanes_;
    check(rl_dqn_collect(dqn_, horizon, nullptr), eng_.handle());
    summary.push_dqn(dqn_);
    const StepsSummary s = summary.read();
    summary.clear();
    LogGroup group(logger);
    ScopedLogger sim(group, "sim");
    s.log(sim);
  }
  void batch_update(StatsLogger &logger) {  // dqn.rs:263-337
    logger.log_scalar("exploration_rate", exploration_rate(ActorMode::Training));  // :268-272
    rl_dqn_update_stats st{};
    check(rl_dqn_update(dqn_, &st, nullptr), eng_.handle());
    logger.log_scalar("loss", st.loss_last);  // ToLog::All
    global_steps_ = st.global_steps;
  }
  uint64_t global_steps() const { return global_steps_; }

 private:
  template <typename VB, typename OC>
  friend std::unique_ptr<DqnAgent> build_dqn_agent(const DqnConfig<VB, OC> &, EnvLanes &, uint64_t, const uint32_t (&)[8]);
  explicit DqnAgent(Engine &eng) : eng_(eng) {}
  Engine &eng_;
  std::unique_ptr<Module> q_;
  std::unique_ptr<Optimizer> opt_;
  rl_dqn *dqn_ = nullptr;
  uint64_t n_lanes_ = 0, global_steps_ = 0;
};

// BuildAgent for DqnConfig (dqn.rs:74-96); `agent_key` is the 32-byte seed `Prng::from_rng(rng)` draws
template <typename VB, typename OC>
std::unique_ptr<DqnAgent> build_dqn_agent(const DqnConfig<VB, OC> &c, EnvLanes &env, uint64_t seed, const uint32_t (&agent_key)[8]) {
  Engine &eng = env.engine();
  std::unique_ptr<DqnAgent> a(new DqnAgent(eng));
  a->n_lanes_ = env.num_lanes();
  a->q_ = c.action_value_fn_config.build_module(eng, env.num_observation_features(), env.num_actions(), seed);
  a->opt_ = c.optimizer_config.build_optimizer(*a->q_, eng);
  rl_dqn_config d;
  check(rl_dqn_config_default(&d));
  d.target = c.one_step_td ? RL_DQN_TARGET_ONE_STEP_TD : RL_DQN_TARGET_REWARD_TO_GO;
  d.exploration_kind = RL_SCHEDULE_LINEAR_ANNEALED;
  d.exploration_start = c.exploration_start;
  d.exploration_end = c.exploration_end;
  d.exploration_period = c.exploration_period;
  d.minibatch_steps = c.minibatch_steps;
  d.opt_steps_per_update = c.opt_steps_per_update;
  d.buffer_capacity = (c.buffer_capacity + env.num_lanes() - 1) / env.num_lanes();
  d.update_kind = RL_COLLECT_FIRST_REST;
  d.update_first = c.update_first;
  d.update_rest = c.update_rest;
  d.discount_factor = (float)env.discount_factor();
  std::memcpy(d.agent_key, agent_key, sizeof(d.agent_key));
  // a feed-forward module, or a recurrent chain: the actor then carries the module's state through an episode and the
  // update runs whole sampled episodes (relearn_hip.h, rl_dqn_create_recurrent); an env of more than two actions (AS:
  // FiniteSpace, dqn.rs:75-86) builds through rl_dqn_create_finite, either kind of module
  // (tabular-MDP lanes: rl_dqn_create_finite at every action count, step-wise collection)
  auto *create = env.num_actions() > 2 || env.tabular_mdp() ? rl_dqn_create_finite
                                       : (builds_recurrent_module<VB>::value ? rl_dqn_create_recurrent : rl_dqn_create);
  check(create(env.handle(), a->q_->handle(), a->opt_->handle(), &d, &a->dqn_), eng.handle());
  return a;
}

// ---------------------------------------------------------------- actor serialisation (examples/cartpole-trpo.rs:71-93)
// `serde_cbor::to_writer(file, &agent.actor(ActorMode::Evaluation))` / `serde_cbor::from_reader(file)`
inline std::vector<uint8_t> actor_to_cbor(EnvLanes &env, Module &module, int32_t actor_kind = RL_ACTOR_POLICY,
                                          double exploration_rate = 0.0) {
  uint64_t len = 0;
  check(rl_actor_to_cbor(env.handle(), module.handle(), actor_kind, exploration_rate, nullptr, 0, &len),
        env.engine().handle());
  std::vector<uint8_t> buf(len);
  check(rl_actor_to_cbor(env.handle(), module.handle(), actor_kind, exploration_rate, buf.data(), len, &len),
        env.engine().handle());
  return buf;
}
inline void module_from_cbor(Module &module, const std::vector<uint8_t> &doc, Engine &eng) {
  check(rl_module_from_cbor(module.handle(), doc.data(), doc.size()), eng.handle());
}

// ---------------------------------------------------------------- the period loop of train_parallel (train.rs:68-186)
inline void train_batched(ActorCriticAgent &agent, EnvLanes &env, DeviceHistory &history, uint64_t num_periods,
                          StatsLogger &logger) {
  for (uint64_t period = 0; period < num_periods; ++period) {
    const auto collect_start = std::chrono::steady_clock::now();
    agent.collect(env, history);
    env.engine().sync();
    {
      ScopedLogger sim(logger, "sim");
      uint64_t episodes = 0;
      for (uint8_t f : history.successors()) episodes += f != RL_SUCC_CONTINUE;
      // train.rs:160-175 logs the period's StepsSummary; with lanes that persist across periods the episode statistics
      // are per period: mean length = steps / episode ends (a moving estimate), CartPole's episode reward = its length
      if (episodes > 0) sim.log_scalar("ep/length_mean", (double)history.num_steps() / (double)episodes);
      sim.log_counter_increment("ep/count", episodes);                 // train.rs:171
      sim.log_counter_increment("step/count", history.num_steps());    // train.rs:175
      sim.log_duration("time", std::chrono::duration<double>(std::chrono::steady_clock::now() - collect_start).count());
    }
    const auto update_start = std::chrono::steady_clock::now();
    agent.batch_update(history, logger);
    ScopedLogger up(logger, "agent_update");
    up.log_duration("time", std::chrono::duration<double>(std::chrono::steady_clock::now() - update_start).count());
    up.log_counter_increment("count", 1);  // train.rs:182-184
  }
}

// The same loop with the period's StepsSummary computed on the device: `summary` (one lane per env lane) takes every
// collection, the full set of train.rs:160-175 is logged with the reference's definitions, and the completed
// statistics are cleared for the next period while the episodes in progress carry over (lanes persist).
inline void train_batched(ActorCriticAgent &agent, EnvLanes &env, DeviceHistory &history, uint64_t num_periods,
                          StatsLogger &logger, StepsSummaryLanes &summary) {
  for (uint64_t period = 0; period < num_periods; ++period) {
    const auto collect_start = std::chrono::steady_clock::now();
    agent.collect(env, history);
    summary.push(history);
    const StepsSummary s = summary.read();  // (synchronises)
    summary.clear();
    {
      LogGroup group(logger);
      ScopedLogger sim(group, "sim");
      s.log(sim);
      sim.log_duration("time", std::chrono::duration<double>(std::chrono::steady_clock::now() - collect_start).count());
    }
    const auto update_start = std::chrono::steady_clock::now();
    agent.batch_update(history, logger);
    ScopedLogger up(logger, "agent_update");
    up.log_duration("time", std::chrono::duration<double>(std::chrono::steady_clock::now() - update_start).count());
    up.log_counter_increment("count", 1);  // train.rs:182-184
  }
}

// ---------------------------------------------------------------- bandit baselines (src/agents/meta.rs, bandits/)
// The inner-agent configurations of relearn_experiments/src/bin/rl2-bandits.rs `eval` (:166-261) that the library runs on
// the meta-bandit lanes, each with the reference's Default.  `raw()` is the C ABI's rl_bandit_agent_config.
struct RandomAgentConfig {  // src/agents/random.rs:59-73: act = action_space.sample(rng)
  rl_bandit_agent_config raw() const { return rl_bandit_agent_config{RL_BANDIT_AGENT_RANDOM, 0, 0.0, 0, 0.0}; }
};
struct TabularQLearningAgentConfig {  // src/agents/tabular.rs:21-51
  double exploration_rate = 0.2;
  uint64_t initial_action_count = 0;
  double initial_action_value = 0.0;
  rl_bandit_agent_config raw() const {
    return rl_bandit_agent_config{RL_BANDIT_AGENT_TABULAR_Q, 0, exploration_rate, initial_action_count,
                                  initial_action_value};
  }
};
struct UCB1AgentConfig {  // src/agents/bandits/ucb.rs:18-42
  double exploration_rate = 0.2;
  rl_bandit_agent_config raw() const { return rl_bandit_agent_config{RL_BANDIT_AGENT_UCB1, 0, exploration_rate, 0, 0.0}; }
};
// src/agents/bandits/thompson_sampling.rs: the experiment's TS is num_samples 1, its OTS 10 (rl2-bandits.rs:213-216); the
// C ABI carries num_samples in initial_action_count.  The Beta sampler is include/rl_beta.h
struct BetaThompsonSamplingAgentConfig {
  uint64_t num_samples = 1;
  rl_bandit_agent_config raw() const {
    return rl_bandit_agent_config{RL_BANDIT_AGENT_THOMPSON, 0, 0.0, num_samples, 0.0};
  }
};

// ResettingMetaAgent<TC> (src/agents/meta.rs:21-199) over the lanes of a MetaBanditLanes: one inner agent per lane, built
// fresh from `TC` wherever the lane's trial starts, acting in Training mode and updated after every pull
// (SerialActorAgent, src/agents/serial.rs:43-95).  `collect` is the batched form of Actor::act driven by
// Environment::run: all steps of a horizon in one launch.  No updates at the meta level (meta.rs:201-227).
class ResettingMetaAgent {
 public:
  template <typename TC>
  ResettingMetaAgent(MetaBanditLanes &env, const TC &inner_agent_config) : eng_(env.engine()), n_lanes_(env.num_lanes()) {
    const rl_bandit_agent_config c = inner_agent_config.raw();
    check(rl_bandit_agent_create(env.handle(), &c, &h_), eng_.handle());
    n_arms_ = env.num_actions();
  }
  ~ResettingMetaAgent() { rl_bandit_agent_destroy(h_); }
  ResettingMetaAgent(const ResettingMetaAgent &) = delete;
  ResettingMetaAgent &operator=(const ResettingMetaAgent &) = delete;
  rl_bandit_agent *handle() const { return h_; }
  // history.horizon() steps of every lane of the env the agent was built on
  void collect(MetaBanditLanes &env, DeviceHistory &history) {
    check(rl_bandit_agent_rollout(h_, env.handle(), history.handle()), eng_.handle());
  }
  // the inner agents after the updates of all pulls so far: the next unread word of each lane's actor stream, the
  // per-arm selection counts and values / mean rewards [n_arms][n_lanes] (TabularQLearningAgentConfig, UCB1AgentConfig)
  std::vector<uint64_t> actor_word_positions() const { return read<uint64_t>(RL_BANDIT_STATE_ACTOR_POS, n_lanes_); }
  std::vector<uint64_t> action_counts() const { return read<uint64_t>(RL_BANDIT_STATE_COUNTS, n_arms_ * n_lanes_); }
  std::vector<double> action_values() const { return read<double>(RL_BANDIT_STATE_VALUES, n_arms_ * n_lanes_); }
  // BetaThompsonSamplingAgentConfig only: the per-arm counts of rewards at most / above 0.5, [n_arms][n_lanes]
  std::vector<uint64_t> low_reward_counts() const { return read<uint64_t>(RL_BANDIT_STATE_LOW_COUNTS, n_arms_ * n_lanes_); }
  std::vector<uint64_t> high_reward_counts() const { return read<uint64_t>(RL_BANDIT_STATE_HIGH_COUNTS, n_arms_ * n_lanes_); }

 private:
  template <typename T>
  std::vector<T> read(int32_t field, uint64_t count) const {
    std::vector<T> v(count);
    check(rl_bandit_agent_state_read(h_, field, v.data(), count * sizeof(T)), eng_.handle());
    return v;
  }
  Engine &eng_;
  rl_bandit_agent *h_ = nullptr;
  uint64_t n_lanes_;
  uint32_t n_arms_ = 0;
};

}  // namespace relearn
