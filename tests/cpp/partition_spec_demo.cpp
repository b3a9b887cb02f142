// partition_spec_demo.cpp — the HIP-free side of rl_env_create_partition, rl_rnn_chain_create_wide24 and
// rl_traj_create_wide24 on the CPU, one JSON document on stdout:
//   "spec"      env_spec_partition (relearn_amd/csrc/handle_spec.hpp) for a list of configs: the refusal's code and words,
//               or D, A, the kind and the lanes' constants
//   "kinds"     the older constructors' answer to the new kind (env_check_kind)
//   "chains"    chain_limits_wide24: the routing and the refusals of rl_rnn_chain_create_wide24
//   "traj"      traj_max_obs_dim: the plane bound of the three trajectory constructors
//   "rollout"   rollout_path for PartitionGame lanes: ROLL_STACK under a recurrent chain, the refusal of a feed-forward
//               module by name, and the older kinds' paths unchanged
//   "scalar"    the scalar env PartitionGame (host/envs.hpp): the first observation and two steps on one stream, the
//               stream position after each
//   "wrapped"   WithVisibleStepLimit<PartitionGame>: an episode of three steps, `remaining` in the observation
// tests/test_partition_spec_cpp.py reads it; the same program runs under ASan and UBSan.
//   g++ -std=c++17 -ffp-contract=off -Wall -Wextra -Werror -I <repo> tests/cpp/partition_spec_demo.cpp -o demo && ./demo
#include <cstring>
#include <iostream>
#include <sstream>

#include "relearn_amd/csrc/handle_spec.hpp"

static std::string quoted(const std::string &s) {
  std::string out = "\"";
  for (char c : s) {
    if (c == '"' || c == '\\') out += '\\';
    out += c;
  }
  return out + "\"";
}

static rl_env_config env_config(int32_t kind, int32_t limit, uint64_t max_steps, uint64_t n_lanes) {
  rl_env_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.kind = kind;
  cfg.limit_kind = limit;
  cfg.max_steps = max_steps;
  cfg.n_lanes = n_lanes;
  cfg.lane_offset = 25;
  cfg.seed_env = 3;
  cfg.seed_actor = 4;
  cfg.cartpole = rl_cartpole_params{9.8, 1.0, 0.1, 0.5, 0.01, 0.01, 0.02, 10.0, 2.4, 0.20943951023931953, 0.99};
  return cfg;
}

struct SpecCase {
  const char *name;
  int32_t kind, limit;
  uint64_t max_steps, lanes;
};

static std::string spec_json() {
  const std::vector<SpecCase> cases = {
      {"visible_1000", RL_ENV_PARTITION, RL_LIMIT_VISIBLE, 1000, 64},  // the experiment's
      {"latent_3", RL_ENV_PARTITION, RL_LIMIT_LATENT, 3, 200},
      {"no_limit", RL_ENV_PARTITION, RL_LIMIT_NONE, 0, 1},
      {"kind_not_read", RL_ENV_CARTPOLE, RL_LIMIT_VISIBLE, 3, 8},
      {"no_limit_ignores_max_steps", RL_ENV_PARTITION, RL_LIMIT_NONE, 7, 8},
      {"limit_kind_3", RL_ENV_PARTITION, 3, 5, 8},
      {"limit_kind_negative", RL_ENV_PARTITION, -1, 5, 8},
      {"visible_0_steps", RL_ENV_PARTITION, RL_LIMIT_VISIBLE, 0, 8},
      {"latent_2_32_steps", RL_ENV_PARTITION, RL_LIMIT_LATENT, 1ull << 32, 8},
      {"no_lanes", RL_ENV_PARTITION, RL_LIMIT_NONE, 0, 0},
      {"lanes_2_31", RL_ENV_PARTITION, RL_LIMIT_NONE, 0, 1ull << 31},
      // the order of the refusals is behaviour: the limit's kind, its steps, the lanes
      {"limit_kind_before_steps", RL_ENV_PARTITION, 3, 0, 0},
      {"steps_before_lanes", RL_ENV_PARTITION, RL_LIMIT_VISIBLE, 0, 0},
  };
  std::ostringstream o;
  o << "{";
  for (size_t i = 0; i < cases.size(); ++i) {
    const SpecCase &c = cases[i];
    o << (i ? ",\n  " : "\n  ") << quoted(c.name) << ": ";
    try {
      const EnvSpec s = env_spec_partition(env_config(c.kind, c.limit, c.max_steps, c.lanes));
      const CartPoleDev &d = s.dev;
      uint32_t key[8];
      rl_seed_from_u64(3, key);
      o << "{\"code\": 0, \"dims\": [" << s.D << ", " << s.A << "], \"kind\": " << s.cfg.kind << ", \"max_steps\": " << d.max_steps
        << ", \"limit_kind\": " << d.limit_kind << ", \"chain_size\": " << d.chain_size << ", \"mem_actions\": " << d.mem_actions
        << ", \"bandit\": " << d.bandit << ", \"lane_offset\": " << d.lane_offset << ", \"tables\": " << (s.mdp.S + s.meta_mdp_rows)
        << ", \"key_env_is_seed_3\": " << (std::memcmp(key, d.key_env, sizeof(key)) == 0 ? "true" : "false") << "}";
    } catch (const RlError &e) {
      o << "{\"code\": " << e.code << ", \"message\": " << quoted(e.what()) << "}";
    }
  }
  o << "}";
  return o.str();
}

static std::string kinds_json() {
  std::ostringstream o;
  const double values[2] = {0.0, 1.0};
  auto refusal = [&](auto fn) -> std::string {
    try {
      fn();
      return "{\"code\": 0}";
    } catch (const RlError &e) {
      return "{\"code\": " + std::to_string(e.code) + ", \"message\": " + quoted(e.what()) + "}";
    }
  };
  const rl_env_config cfg = env_config(RL_ENV_PARTITION, RL_LIMIT_NONE, 0, 8);
  o << "{\"rl_env_create\": " << refusal([&] { env_spec_basic(cfg); })
    << ", \"rl_env_create_bandit\": " << refusal([&] { env_spec_bandit(cfg, values, 2); }) << "}";
  return o.str();
}

static std::string chains_json() {
  auto build = [](uint32_t in, uint32_t out, uint32_t H = 8, uint32_t H2 = 0) -> std::string {
    const rl_rnn_chain_config cfg{RL_CELL_GRU, in, H, 1, 1, H2, out};
    try {
      const ModuleShape m = chain_shape(cfg, chain_limits_wide24(cfg));
      return "{\"code\": 0, \"in\": " + std::to_string(m.in_dim) + ", \"out\": " + std::to_string(m.out_dim) +
             ", \"P\": " + std::to_string(m.P) + ", \"lane_kernels\": " + (m.lane_kernels() ? "true" : "false") + "}";
    } catch (const RlError &e) {
      return "{\"code\": " + std::to_string(e.code) + ", \"message\": " + quoted(e.what()) + "}";
    }
  };
  const rl_rnn_chain_config c5{RL_CELL_GRU, 5, 8, 1, 1, 0, 2}, c14{RL_CELL_GRU, 14, 8, 1, 1, 0, 5}, c19{RL_CELL_GRU, 19, 8, 1, 1, 0, 5},
      c20{RL_CELL_GRU, 20, 8, 1, 1, 0, 12}, c21{RL_CELL_GRU, 21, 8, 1, 1, 0, 2}, c24{RL_CELL_LSTM, 24, 8, 1, 1, 6, 2};
  std::ostringstream o;
  o << "{\"policy_24_2\": " << build(24, 2, 8, 6) << ", \"critic_24_1\": " << build(24, 1, 8, 6) << ", \"policy_23_2\": " << build(23, 2)
    << ", \"in_21\": " << build(21, 2) << ", \"in_24_out_12\": " << build(24, 12) << ", \"in_0\": " << build(0, 2)
    << ", \"in_25\": " << build(25, 2) << ", \"out_13_at_24\": " << build(24, 13) << ", \"out_0_at_24\": " << build(24, 0)
    << ", \"hidden_257_at_24\": " << build(24, 2, 257) << ", \"out_13_at_19\": " << build(19, 13) << ", \"out_13_at_14\": " << build(14, 13)
    << ", \"in_9_out_9\": " << build(9, 9) << ", \"routing\": [" << (&chain_limits_wide24(c5) == &CHAIN_NARROW) << ", "
    << (&chain_limits_wide24(c14) == &CHAIN_WIDE) << ", " << (&chain_limits_wide24(c19) == &CHAIN_WIDE20) << ", "
    << (&chain_limits_wide24(c20) == &CHAIN_WIDE20) << ", " << (&chain_limits_wide24(c21) == &CHAIN_WIDE24) << ", "
    << (&chain_limits_wide24(c24) == &CHAIN_WIDE24) << "]}";
  return o.str();
}

static std::string rollout_json() {
  auto path = [](int kind, uint32_t D, uint32_t A, uint32_t chain_size, const ModuleShape &m) -> std::string {
    try {
      return "{\"code\": 0, \"path\": " + std::to_string((int)rollout_path(kind, D, A, chain_size, m)) + "}";
    } catch (const RlError &e) {
      return "{\"code\": " + std::to_string(e.code) + ", \"message\": " + quoted(e.what()) + "}";
    }
  };
  const rl_rnn_chain_config c24{RL_CELL_GRU, 24, 8, 1, 1, 6, 2}, c23{RL_CELL_LSTM, 23, 8, 1, 1, 0, 2}, c24x3{RL_CELL_GRU, 24, 8, 1, 1, 0, 3};
  const ModuleShape gru24 = chain_shape(c24, chain_limits_wide24(c24)), lstm23 = chain_shape(c23, chain_limits_wide24(c23)),
                    three = chain_shape(c24x3, chain_limits_wide24(c24x3)), ff = fused_mlp_shape(5, 16, 2);
  const uint32_t widths[1] = {16};
  const ModuleShape gen8 = mlp_shape(8, widths, 1, 2, RL_ACT_RELU, RL_ACT_IDENTITY, true);
  std::ostringstream o;
  o << "{\"gru_24\": " << path(RL_ENV_PARTITION, 24, 2, 0, gru24) << ", \"lstm_23\": " << path(RL_ENV_PARTITION, 23, 2, 0, lstm23)
    << ", \"gru_24_on_23\": " << path(RL_ENV_PARTITION, 23, 2, 0, gru24) << ", \"three_outputs\": " << path(RL_ENV_PARTITION, 24, 2, 0, three)
    << ", \"fused_mlp\": " << path(RL_ENV_PARTITION, 24, 2, 0, ff) << ", \"general_mlp\": " << path(RL_ENV_PARTITION, 24, 2, 0, gen8)
    << ", \"cartpole_fused_mlp\": " << path(RL_ENV_CARTPOLE, 5, 2, 0, ff) << ", \"chain_fused_mlp\": " << path(RL_ENV_CHAIN, 5, 2, 5, ff)
    << ", \"stack\": " << (int)ROLL_STACK << ", \"cartpole\": " << (int)ROLL_CARTPOLE << ", \"index_mlp\": " << (int)ROLL_INDEX_MLP << "}";
  return o.str();
}

static std::string scalar_json() {
  const relearn::PartitionGame env;
  relearn::Prng rng = relearn::Prng::seed_from_u64(11);
  rng.set_stream(5);
  relearn::PartitionGame::State s = env.initial_state(rng);
  std::ostringstream o;
  auto obs = [&](const relearn::PartitionGame::State &st) {
    std::string out = "[";
    const std::vector<float> f = env.observe(st, rng);
    for (size_t d = 0; d < f.size(); ++d) out += (d ? ", " : "") + std::to_string((int)f[d]);
    return out + "]";
  };
  o << "{\"features\": " << env.num_observation_features() << ", \"actions\": " << env.num_actions() << ", \"discount\": "
    << env.discount_factor << ", \"axis\": " << s.axis << ", \"pos0\": " << rng.word_pos() << ", \"obs0\": " << obs(s);
  for (int t = 1; t <= 2; ++t) {
    auto [succ, reward] = env.step(std::move(s), (uint64_t)(t - 1), rng);
    s = std::move(*succ.state);
    o << ", \"reward" << t << "\": " << reward << ", \"kind" << t << "\": " << (int)succ.kind << ", \"pos" << t
      << "\": " << rng.word_pos() << ", \"obs" << t << "\": " << obs(s);
  }
  o << "}";
  return o.str();
}

// ... and under the mirror's own visible step limit (WithVisibleStepLimit, host/envs.hpp): three steps, the third an Interrupt
static std::string wrapped_json() {
  const relearn::WithVisibleStepLimit<relearn::PartitionGame> env{relearn::PartitionGame{}, 3};
  relearn::Prng rng = relearn::Prng::seed_from_u64(11);
  rng.set_stream(5);
  auto s = env.initial_state(rng);
  std::ostringstream o;
  auto obs = [&](const auto &st) {
    std::ostringstream out;
    out.precision(9);  // (an f32 round-trips through nine digits)
    const std::vector<float> f = env.observe(st, rng);
    for (size_t d = 0; d < f.size(); ++d) out << (d ? ", " : "[") << f[d];
    return out.str() + "]";
  };
  o << "{\"features\": " << env.num_observation_features() << ", \"obs0\": " << obs(s);
  for (int t = 1; t <= 3; ++t) {
    auto [succ, reward] = env.step(std::move(s), (uint64_t)(t & 1), rng);
    s = std::move(*succ.state);
    o << ", \"reward" << t << "\": " << reward << ", \"kind" << t << "\": " << (int)succ.kind << ", \"obs" << t << "\": " << obs(s);
  }
  o << "}";
  return o.str();
}

int main() {
  std::cout << "{\"spec\": " << spec_json() << ",\n \"kinds\": " << kinds_json() << ",\n \"chains\": " << chains_json()
            << ",\n \"traj\": [" << traj_max_obs_dim(TRAJ_LEVEL_BASE) << ", " << traj_max_obs_dim(TRAJ_LEVEL_WIDE) << ", " << traj_max_obs_dim(TRAJ_LEVEL_WIDE24) << "]"
            << ",\n \"rollout\": " << rollout_json() << ",\n \"scalar\": " << scalar_json() << ",\n \"wrapped\": " << wrapped_json() << ",\n \"constants\": ["
            << RL_WIDE_MAX_OBS_DIM << ", " << RL_XWIDE_MAX_OBS_DIM << ", " << RL_PARTITION_MAX_OBS_DIM << ", "
            << RL_PARTITION_FEATURES << ", " << RL_PARTITION_OBS_DIM << ", " << (int)RL_ENV_PARTITION << "]}" << std::endl;
  return 0;
}
