// meta_mdp_wide_spec_demo.cpp — the HIP-free side of rl_env_create_meta_mdp_wide on the CPU, one JSON document on stdout:
//   "spec"      env_spec_meta_mdp_wide (relearn_amd/csrc/handle_spec.hpp) for a list of configs: the refusal's code and
//               words, or D, A, the kind, the lanes' constants and the floats of a stored row
//   "same"      over the whole range of env_spec_meta_mdp (S, A 2..8, S + A + 4 <= 16): the two specs are equal, byte for
//               byte in the lanes' struct; and outside it the older one refuses where the wide one builds
//   "fused"     the wide table of one-launch shapes and meta_mdp_wide_fused_shape over the range; the older table
//   "chains"    chain_limits_wide20: the routing and the refusals of rl_rnn_chain_create_wide20
//   "rows"      rl_dirichlet_row_normalise / rl_mdp_row_cumulative (include/rl_normal.h) at the bound 16 of the second row
//               class against the host's bound S, bit for bit, rows with zero entries among them
// tests/test_meta_mdp_wide_spec_cpp.py reads it; the same program runs under ASan and UBSan.
//   g++ -std=c++17 -ffp-contract=off -Wall -Wextra -Werror -I <repo> tests/cpp/meta_mdp_wide_spec_demo.cpp -o demo && ./demo
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

static rl_env_config env_config(int32_t limit, uint64_t n_lanes) {
  rl_env_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.kind = RL_ENV_CARTPOLE;  // (not read)
  cfg.limit_kind = limit;
  cfg.max_steps = limit != RL_LIMIT_NONE ? 10 : 0;
  cfg.n_lanes = n_lanes;
  cfg.lane_offset = 25;
  cfg.seed_env = 3;
  cfg.seed_actor = 4;
  cfg.cartpole = rl_cartpole_params{9.8, 1.0, 0.1, 0.5, 0.01, 0.01, 0.02, 10.0, 2.4, 0.20943951023931953, 0.99};
  return cfg;
}

static rl_meta_mdp_config meta_of(uint32_t S, uint32_t A) { return rl_meta_mdp_config{S, A, 1.0, 1.0, 1.0, 1.0, 1.0, 10, 10}; }

static uint32_t f32_bits(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}
static uint64_t f64_bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}

struct SpecCase {
  const char *name;
  rl_meta_mdp_config meta;
  int32_t limit;
  uint64_t lanes;
};

static std::string spec_json() {
  auto with = [](uint32_t S, uint32_t A, auto set) {
    rl_meta_mdp_config m = meta_of(S, A);
    set(m);
    return m;
  };
  auto none = [](auto &) {};
  const double inf = INFINITY, nan = NAN;
  const std::vector<SpecCase> cases = {
      {"10x5", meta_of(10, 5), RL_LIMIT_NONE, 64},
      {"9x2", with(9, 2, [](auto &m) { m.alpha = 2.5, m.max_inner_steps = 1, m.episodes_per_trial = 1; }), RL_LIMIT_NONE, 1},
      {"10x6", with(10, 6, [](auto &m) { m.alpha = 0.5, m.reward_stddev = 0.0; }), RL_LIMIT_NONE, 70},
      {"8x8", with(8, 8, [](auto &m) { m.max_inner_steps = (1ull << 32) - 1; }), RL_LIMIT_NONE, 70},
      {"9x7", meta_of(9, 7), RL_LIMIT_NONE, 70},
      {"5x5", meta_of(5, 5), RL_LIMIT_NONE, 70},
      {"states_1", meta_of(1, 5), RL_LIMIT_NONE, 8},
      {"states_11", meta_of(11, 2), RL_LIMIT_NONE, 8},
      {"actions_1", meta_of(10, 1), RL_LIMIT_NONE, 8},
      {"actions_9", meta_of(2, 9), RL_LIMIT_NONE, 8},
      {"21_features_10x7", meta_of(10, 7), RL_LIMIT_NONE, 8},
      {"21_features_9x8", meta_of(9, 8), RL_LIMIT_NONE, 8},
      {"inner_0", with(10, 5, [](auto &m) { m.max_inner_steps = 0; }), RL_LIMIT_NONE, 8},
      {"inner_2_32", with(10, 5, [](auto &m) { m.max_inner_steps = 1ull << 32; }), RL_LIMIT_NONE, 8},
      {"episodes_0", with(10, 5, [](auto &m) { m.episodes_per_trial = 0; }), RL_LIMIT_NONE, 8},
      {"episodes_2_32", with(5, 5, [](auto &m) { m.episodes_per_trial = 1ull << 32; }), RL_LIMIT_NONE, 8},
      {"alpha_0", with(10, 5, [](auto &m) { m.alpha = 0.0; }), RL_LIMIT_NONE, 8},
      {"alpha_nan", with(5, 5, [=](auto &m) { m.alpha = nan; }), RL_LIMIT_NONE, 8},
      {"prior_mean_nan", with(10, 5, [=](auto &m) { m.reward_prior_mean = nan; }), RL_LIMIT_NONE, 8},
      {"prior_stddev_negative", with(10, 5, [](auto &m) { m.reward_prior_stddev = -0.5; }), RL_LIMIT_NONE, 8},
      {"stddev_inf", with(10, 5, [=](auto &m) { m.reward_stddev = inf; }), RL_LIMIT_NONE, 8},
      {"discount_inf", with(10, 5, [=](auto &m) { m.discount_factor = inf; }), RL_LIMIT_NONE, 8},
      {"latent_limit", with(10, 5, none), RL_LIMIT_LATENT, 8},
      {"visible_limit", with(5, 5, none), RL_LIMIT_VISIBLE, 8},
      {"no_lanes", with(10, 5, none), RL_LIMIT_NONE, 0},
      // the order of the refusals is behaviour: sizes, the inner limit, the trial limit, alpha, the prior, the stddev,
      // the discount, the step limit, the lanes
      {"sizes_before_inner", with(11, 5, [](auto &m) { m.max_inner_steps = 0, m.alpha = 0.0; }), RL_LIMIT_LATENT, 0},
      {"inner_before_episodes", with(10, 5, [](auto &m) { m.max_inner_steps = 0, m.episodes_per_trial = 0; }), RL_LIMIT_NONE, 8},
      {"episodes_before_alpha", with(10, 5, [](auto &m) { m.episodes_per_trial = 0, m.alpha = 0.0; }), RL_LIMIT_NONE, 8},
      {"alpha_before_prior_mean", with(10, 5, [=](auto &m) { m.alpha = 0.0, m.reward_prior_mean = nan; }), RL_LIMIT_NONE, 8},
      {"prior_mean_before_prior_stddev",
       with(10, 5, [=](auto &m) { m.reward_prior_mean = nan, m.reward_prior_stddev = -1.0; }), RL_LIMIT_NONE, 8},
      {"prior_stddev_before_stddev", with(10, 5, [](auto &m) { m.reward_prior_stddev = -1.0, m.reward_stddev = -1.0; }),
       RL_LIMIT_NONE, 8},
      {"stddev_before_discount", with(10, 5, [=](auto &m) { m.reward_stddev = -1.0, m.discount_factor = inf; }), RL_LIMIT_NONE, 8},
      {"discount_before_limit", with(10, 5, [=](auto &m) { m.discount_factor = inf; }), RL_LIMIT_LATENT, 8},
      {"limit_before_lanes", with(10, 5, none), RL_LIMIT_LATENT, 0},
  };
  std::ostringstream o;
  o << "{";
  for (size_t i = 0; i < cases.size(); ++i) {
    const SpecCase &c = cases[i];
    o << (i ? ",\n  " : "\n  ") << quoted(c.name) << ": ";
    try {
      const EnvSpec s = env_spec_meta_mdp_wide(env_config(c.limit, c.lanes), c.meta);
      const CartPoleDev &d = s.dev;
      o << "{\"code\": 0, \"dims\": [" << s.D << ", " << s.A << "], \"kind\": " << s.cfg.kind << ", \"rows\": " << s.meta_mdp_rows
        << ", \"states\": " << d.mm.states << ", \"actions\": " << d.mm.actions << ", \"inner_steps\": " << d.mm.inner_steps
        << ", \"episodes\": " << d.max_steps << ", \"chain_size\": " << d.chain_size << ", \"lane_offset\": " << d.lane_offset
        << ", \"row_floats\": " << meta_mdp_row_floats(d.mm.states) << ", \"prior\": [" << f64_bits(d.mm_prior.alpha) << ", "
        << f64_bits(d.mm_prior.reward_prior_mean) << ", " << f64_bits(d.mm_prior.reward_prior_stddev) << ", "
        << f64_bits(d.mm_prior.reward_stddev) << "]"
        << ", \"tables_unset\": " << (d.mm.cum == nullptr && d.mm.mean == nullptr ? "true" : "false") << "}";
    } catch (const RlError &e) {
      o << "{\"code\": " << e.code << ", \"message\": " << quoted(e.what()) << "}";
    }
  }
  o << "}";
  return o.str();
}

// env_spec_meta_mdp_wide against env_spec_meta_mdp over every (S, A) either takes
static std::string same_json() {
  size_t equal = 0, wide_only = 0, neither = 0, differ = 0;
  for (uint32_t S = 0; S <= 12; ++S)
    for (uint32_t A = 0; A <= 10; ++A) {
      rl_meta_mdp_config m = meta_of(S, A);
      m.alpha = 0.5 + S, m.reward_prior_mean = 0.25 * A, m.reward_stddev = 0.5, m.max_inner_steps = 3 + S, m.episodes_per_trial = 2 + A;
      bool old_ok = true, wide_ok = true;
      EnvSpec a, b;
      try {
        a = env_spec_meta_mdp(env_config(RL_LIMIT_NONE, 70), m);
      } catch (const RlError &) {
        old_ok = false;
      }
      try {
        b = env_spec_meta_mdp_wide(env_config(RL_LIMIT_NONE, 70), m);
      } catch (const RlError &) {
        wide_ok = false;
      }
      if (old_ok && wide_ok) {
        const bool same = a.D == b.D && a.A == b.A && a.meta_mdp_rows == b.meta_mdp_rows &&
                          std::memcmp(&a.cfg, &b.cfg, sizeof(a.cfg)) == 0 && std::memcmp(&a.dev, &b.dev, sizeof(a.dev)) == 0 &&
                          meta_mdp_row_floats(b.dev.mm.states) == 8;
        (same ? equal : differ) += 1;
      } else if (wide_ok) {
        wide_only += 1;
      } else if (old_ok) {
        differ += 1;  // the wide constructor takes everything the older one takes
      } else {
        neither += 1;
      }
    }
  std::ostringstream o;
  o << "{\"equal\": " << equal << ", \"wide_only\": " << wide_only << ", \"neither\": " << neither << ", \"differ\": " << differ
    << "}";
  return o.str();
}

static std::string fused_json() {
  std::ostringstream o;
  o << "{\"table\": [";
  bool first = true;
  for (const MetaMdpShape &m : META_MDP_WIDE_FUSED_SHAPES) {
    o << (first ? "" : ", ") << "[" << m.S << ", " << m.A << "]";
    first = false;
  }
  o << "], \"accepted\": [";
  first = true;
  for (uint32_t S = 0; S <= 12; ++S)
    for (uint32_t A = 0; A <= 10; ++A)
      if (meta_mdp_wide_fused_shape(S, A)) {
        o << (first ? "" : ", ") << "[" << S << ", " << A << "]";
        first = false;
      }
  o << "], \"older_table\": [";
  first = true;
  for (const MetaMdpShape &m : META_MDP_FUSED_SHAPES) {
    o << (first ? "" : ", ") << "[" << m.S << ", " << m.A << "]";
    first = false;
  }
  o << "], \"older_takes_10x5\": " << (meta_mdp_fused_shape(10, 5) ? "true" : "false") << "}";
  return o.str();
}

static std::string chains_json() {
  auto build = [](uint32_t in, uint32_t out, uint32_t H = 8) -> std::string {
    const rl_rnn_chain_config cfg{RL_CELL_GRU, in, H, 1, 1, 0, out};
    try {
      const ModuleShape m = chain_shape(cfg, chain_limits_wide20(cfg));
      return "{\"code\": 0, \"in\": " + std::to_string(m.in_dim) + ", \"out\": " + std::to_string(m.out_dim) +
             ", \"P\": " + std::to_string(m.P) + ", \"lane_kernels\": " + (m.lane_kernels() ? "true" : "false") + "}";
    } catch (const RlError &e) {
      return "{\"code\": " + std::to_string(e.code) + ", \"message\": " + quoted(e.what()) + "}";
    }
  };
  const rl_rnn_chain_config c5{RL_CELL_GRU, 5, 8, 1, 1, 0, 2}, c14{RL_CELL_GRU, 14, 8, 1, 1, 0, 5}, c16{RL_CELL_GRU, 16, 8, 1, 1, 0, 12},
      c17{RL_CELL_GRU, 17, 8, 1, 1, 0, 5};
  std::ostringstream o;
  o << "{\"policy_19_5\": " << build(19, 5) << ", \"critic_19_1\": " << build(19, 1) << ", \"in_20_out_12\": " << build(20, 12)
    << ", \"in_17\": " << build(17, 5) << ", \"in_0\": " << build(0, 5) << ", \"in_21\": " << build(21, 5)
    << ", \"out_13_at_19\": " << build(19, 13) << ", \"out_0_at_19\": " << build(19, 0) << ", \"out_13_at_14\": " << build(14, 13)
    << ", \"hidden_257_at_19\": " << build(19, 5, 257) << ", \"in_9_out_9_at_8\": " << build(9, 9)
    << ", \"routing\": [" << (&chain_limits_wide20(c5) == &CHAIN_NARROW) << ", " << (&chain_limits_wide20(c14) == &CHAIN_WIDE) << ", "
    << (&chain_limits_wide20(c16) == &CHAIN_WIDE) << ", " << (&chain_limits_wide20(c17) == &CHAIN_WIDE20) << "]}";
  return o.str();
}

// the shared row functions at the second row class's bound (16, arrays padded) against the host's (S), S = 1..16
static std::string rows_json() {
  uint32_t key[8];
  rl_seed_from_u64(9, key);
  uint64_t pos = 0;
  size_t checked = 0, with_zero = 0, at_9_10 = 0;
  bool same = true, rule = true;
  for (uint32_t S = 1; S <= 16; ++S)
    for (int trial = 0; trial < (S == 9 || S == 10 ? 80 : 24); ++trial) {
      double g[16] = {}, sum = 0.0;
      for (uint32_t j = 0; j < S; ++j) {
        g[j] = rl_gamma_sample(0.3, key, 1, &pos);
        if (trial % 4 == 1 && j % 2 == 1) g[j] = 0.0;  // successors of probability zero, the last one among them
        if (trial % 4 == 2 && j + 1 == S && S > 1) g[j] = 0.0;
        if (trial % 4 == 3 && j >= 8) g[j] = 0.0;  // nothing behind the eighth entry: the tail of ones begins before it
        sum = sum + g[j];
      }
      if (sum == 0.0) continue;
      float p16[16] = {}, c16[16];
      for (float &v : c16) v = 1.0f;
      std::vector<float> p(S), c(S);
      rl_dirichlet_row_normalise(g, sum, S, 16, p16);
      rl_mdp_row_cumulative(p16, S, 16, c16);
      rl_dirichlet_row_normalise(g, sum, S, S, p.data());
      rl_mdp_row_cumulative(p.data(), S, S, c.data());
      bool zero = false;
      for (uint32_t j = 0; j < 16; ++j) {
        if (j < S) {
          same = same && f32_bits(p16[j]) == f32_bits(p[j]) && f32_bits(c16[j]) == f32_bits(c[j]);
          zero = zero || p[j] == 0.0f;
        } else {
          same = same && p16[j] == 0.0f && c16[j] == 1.0f;  // the padding stays
        }
      }
      // the rule itself: the count of cum[j] <= u over j < 15 never leaves 0 .. S - 1 for u < 1, and is monotone
      for (uint32_t j = 0; j + 1 < 16; ++j) rule = rule && c16[j] <= c16[j + 1];
      rule = rule && c16[S - 1] == 1.0f;
      checked += 1;
      with_zero += zero ? 1 : 0;
      at_9_10 += S == 9 || S == 10 ? 1 : 0;
    }
  std::ostringstream o;
  o << "{\"same\": " << (same ? "true" : "false") << ", \"rule\": " << (rule ? "true" : "false") << ", \"rows\": " << checked
    << ", \"zero_entries\": " << with_zero << ", \"rows_at_9_and_10\": " << at_9_10 << "}";
  return o.str();
}

int main() {
  std::cout << "{\"spec\": " << spec_json() << ",\n \"same\": " << same_json() << ",\n \"fused\": " << fused_json()
            << ",\n \"chains\": " << chains_json() << ",\n \"rows\": " << rows_json() << ",\n \"constants\": ["
            << RL_WIDE_MAX_OBS_DIM << ", " << RL_XWIDE_MAX_OBS_DIM << ", " << RL_META_MDP_MAX << ", "
            << RL_META_MDP_WIDE_MAX_STATES << "]}" << std::endl;
  return 0;
}
