// meta_mdp_spec_demo.cpp — the HIP-free side of the meta-MDP lanes on the CPU, one JSON document on stdout:
//   "spec"     env_spec_meta_mdp (relearn_amd/csrc/handle_spec.hpp) for a list of configs: the refusal's code and words, or
//              D, A, the kind and the lanes' constants
//   "fused"    the table of (S, A) shapes whose recurrent rollout is one launch, and meta_mdp_fused_shape over the range
//   "paths"    rollout_path for recurrent and feed-forward modules on these lanes
//   "rows"     rl_mdp_row_cumulative / rl_dirichlet_row_normalise (include/rl_normal.h) at the kernels' loop bound of 8
//              against the host's bound of S
//   "scalar"   the scalar env MetaRandomMdps (host/envs.hpp) stepped over three trials on a few streams: every reward,
//              successor code, observation and table as bit patterns
// tests/test_meta_mdp_spec_cpp.py compares it with tests/meta_mdp_ref.py; the same program runs under ASan and UBSan.
//   g++ -std=c++17 -ffp-contract=off -Wall -Wextra -Werror -I <repo> tests/cpp/meta_mdp_spec_demo.cpp -o demo && ./demo
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

static rl_meta_mdp_config meta_default() {  // rl_meta_mdp_config_default's values
  return rl_meta_mdp_config{5, 5, 1.0, 1.0, 1.0, 1.0, 1.0, 10, 10};
}

struct SpecCase {
  const char *name;
  rl_meta_mdp_config meta;
  int32_t limit;
  uint64_t lanes;
};

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

template <class T, class F>
static std::string list_of(const std::vector<T> &v, F bits) {
  std::ostringstream o;
  o << "[";
  for (size_t i = 0; i < v.size(); ++i) o << (i ? ", " : "") << bits(v[i]);
  o << "]";
  return o.str();
}

static std::string spec_json() {
  auto with = [](auto set) {
    rl_meta_mdp_config m = meta_default();
    set(m);
    return m;
  };
  const double inf = INFINITY, nan = NAN;
  const std::vector<SpecCase> cases = {
      {"default", meta_default(), RL_LIMIT_NONE, 64},
      {"2x2", with([](auto &m) { m.n_states = 2, m.n_actions = 2, m.max_inner_steps = 1, m.episodes_per_trial = 1; }), RL_LIMIT_NONE, 1},
      {"8x4", with([](auto &m) { m.n_states = 8, m.n_actions = 4, m.alpha = 0.5, m.reward_stddev = 0.0; }), RL_LIMIT_NONE, 70},
      {"4x8", with([](auto &m) { m.n_states = 4, m.n_actions = 8, m.alpha = 2.5; }), RL_LIMIT_NONE, 70},
      {"6x6", with([](auto &m) { m.n_states = 6, m.n_actions = 6, m.max_inner_steps = (1ull << 32) - 1; }), RL_LIMIT_NONE, 70},
      {"states_1", with([](auto &m) { m.n_states = 1; }), RL_LIMIT_NONE, 8},
      {"states_9", with([](auto &m) { m.n_states = 9, m.n_actions = 2; }), RL_LIMIT_NONE, 8},
      {"actions_1", with([](auto &m) { m.n_actions = 1; }), RL_LIMIT_NONE, 8},
      {"actions_9", with([](auto &m) { m.n_states = 2, m.n_actions = 9; }), RL_LIMIT_NONE, 8},
      {"17_features", with([](auto &m) { m.n_states = 8, m.n_actions = 5; }), RL_LIMIT_NONE, 8},
      {"reference_default_10x5", with([](auto &m) { m.n_states = 10, m.n_actions = 5; }), RL_LIMIT_NONE, 8},
      {"inner_0", with([](auto &m) { m.max_inner_steps = 0; }), RL_LIMIT_NONE, 8},
      {"inner_2_32", with([](auto &m) { m.max_inner_steps = 1ull << 32; }), RL_LIMIT_NONE, 8},
      {"episodes_0", with([](auto &m) { m.episodes_per_trial = 0; }), RL_LIMIT_NONE, 8},
      {"episodes_2_32", with([](auto &m) { m.episodes_per_trial = 1ull << 32; }), RL_LIMIT_NONE, 8},
      {"alpha_0", with([](auto &m) { m.alpha = 0.0; }), RL_LIMIT_NONE, 8},
      {"alpha_negative", with([](auto &m) { m.alpha = -1.0; }), RL_LIMIT_NONE, 8},
      {"alpha_inf", with([=](auto &m) { m.alpha = inf; }), RL_LIMIT_NONE, 8},
      {"alpha_nan", with([=](auto &m) { m.alpha = nan; }), RL_LIMIT_NONE, 8},
      {"prior_mean_nan", with([=](auto &m) { m.reward_prior_mean = nan; }), RL_LIMIT_NONE, 8},
      {"prior_stddev_negative", with([](auto &m) { m.reward_prior_stddev = -0.5; }), RL_LIMIT_NONE, 8},
      {"prior_stddev_inf", with([=](auto &m) { m.reward_prior_stddev = inf; }), RL_LIMIT_NONE, 8},
      {"stddev_negative", with([](auto &m) { m.reward_stddev = -1.0; }), RL_LIMIT_NONE, 8},
      {"stddev_nan", with([=](auto &m) { m.reward_stddev = nan; }), RL_LIMIT_NONE, 8},
      {"discount_inf", with([=](auto &m) { m.discount_factor = inf; }), RL_LIMIT_NONE, 8},
      {"latent_limit", meta_default(), RL_LIMIT_LATENT, 8},
      {"visible_limit", meta_default(), RL_LIMIT_VISIBLE, 8},
      {"no_lanes", meta_default(), RL_LIMIT_NONE, 0},
      {"sizes_before_alpha", with([](auto &m) { m.n_states = 1, m.alpha = 0.0; }), RL_LIMIT_NONE, 8},
  };
  std::ostringstream o;
  o << "{";
  for (size_t i = 0; i < cases.size(); ++i) {
    const SpecCase &c = cases[i];
    o << (i ? ",\n  " : "\n  ") << quoted(c.name) << ": ";
    try {
      const EnvSpec s = env_spec_meta_mdp(env_config(c.limit, c.lanes), c.meta);
      const CartPoleDev &d = s.dev;
      o << "{\"code\": 0, \"dims\": [" << s.D << ", " << s.A << "], \"kind\": " << s.cfg.kind << ", \"rows\": " << s.meta_mdp_rows
        << ", \"states\": " << d.mm.states << ", \"actions\": " << d.mm.actions << ", \"inner_steps\": " << d.mm.inner_steps
        << ", \"episodes\": " << d.max_steps << ", \"chain_size\": " << d.chain_size << ", \"lane_offset\": " << d.lane_offset
        << ", \"prior\": "
        << list_of(std::vector<double>{d.mm_prior.alpha, d.mm_prior.reward_prior_mean, d.mm_prior.reward_prior_stddev,
                                       d.mm_prior.reward_stddev},
                   f64_bits)
        << ", \"tables_unset\": " << (d.mm.cum == nullptr && d.mm.mean == nullptr ? "true" : "false") << "}";
    } catch (const RlError &e) {
      o << "{\"code\": " << e.code << ", \"message\": " << quoted(e.what()) << "}";
    }
  }
  o << "}";
  return o.str();
}

static std::string fused_json() {
  std::ostringstream o;
  o << "{\"table\": [";
  bool first = true;
  for (const MetaMdpShape &m : META_MDP_FUSED_SHAPES) {
    o << (first ? "" : ", ") << "[" << m.S << ", " << m.A << "]";
    first = false;
  }
  o << "], \"accepted\": [";
  first = true;
  for (uint32_t S = 0; S <= 9; ++S)
    for (uint32_t A = 0; A <= 9; ++A)
      if (meta_mdp_fused_shape(S, A)) {
        o << (first ? "" : ", ") << "[" << S << ", " << A << "]";
        first = false;
      }
  o << "]}";
  return o.str();
}

static const char *PATH_NAMES[] = {"ROLL_GENERAL", "ROLL_STACK", "ROLL_TILE_RECURRENT", "ROLL_INDEX_MLP", "ROLL_CARTPOLE"};

static std::string paths_json() {
  auto env = [](uint32_t S, uint32_t A) {
    rl_meta_mdp_config m = meta_default();
    m.n_states = S, m.n_actions = A;
    return env_spec_meta_mdp(env_config(RL_LIMIT_NONE, 8), m);
  };
  auto path = [](const EnvSpec &s, const ModuleShape &m) -> std::string {
    try {
      return quoted(PATH_NAMES[rollout_path(s.cfg.kind, s.D, s.A, s.dev.chain_size, m)]);
    } catch (const RlError &e) {
      return "{\"code\": " + std::to_string(e.code) + ", \"message\": " + quoted(e.what()) + "}";
    }
  };
  auto chain = [](int32_t cell, uint32_t in, uint32_t H, uint32_t H2, uint32_t out) {
    const rl_rnn_chain_config cfg{cell, in, H, 1, 1, H2, out};
    return chain_shape(cfg, chain_limits_wide(cfg));
  };
  const uint32_t sixteen[1] = {16};
  std::ostringstream o;
  o << "{\"gru_linear_5x5\": " << path(env(5, 5), chain(RL_CELL_GRU, 14, 128, 0, 5))
    << ", \"lstm_mlp_8x4\": " << path(env(8, 4), chain(RL_CELL_LSTM, 16, 12, 6, 4))
    << ", \"gru_mlp_3x3_outside_the_table\": " << path(env(3, 3), chain(RL_CELL_GRU, 10, 9, 6, 3))
    << ", \"gru_tile_shape_on_2x2\": " << path(env(2, 2), chain(RL_CELL_GRU, 8, 128, 128, 2))
    << ", \"feed_forward_2x2\": " << path(env(2, 2), mlp_shape(8, sixteen, 1, 2, RL_ACT_RELU, RL_ACT_IDENTITY, true))
    << ", \"wrong_width\": " << path(env(5, 5), chain(RL_CELL_GRU, 13, 12, 0, 5))
    << ", \"two_output_chain_on_five_actions\": " << path(env(5, 5), chain(RL_CELL_GRU, 14, 12, 0, 2)) << "}";
  return o.str();
}

// the shared row functions at the kernels' bound (8, arrays padded) against the host's (S)
static std::string rows_json() {
  uint32_t key[8];
  rl_seed_from_u64(9, key);
  uint64_t pos = 0;
  size_t checked = 0, with_zero = 0;
  bool same = true;
  for (uint32_t S = 1; S <= 8; ++S)
    for (int trial = 0; trial < 40; ++trial) {
      double g[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sum = 0.0;
      for (uint32_t j = 0; j < S; ++j) {
        g[j] = rl_gamma_sample(0.3, key, 1, &pos);
        if (trial % 4 == 1 && j % 2 == 1) g[j] = 0.0;  // successors of probability zero, the last one among them
        if (trial % 4 == 2 && j + 1 == S && S > 1) g[j] = 0.0;
        sum = sum + g[j];
      }
      if (sum == 0.0) continue;
      float p8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, c8[8] = {1, 1, 1, 1, 1, 1, 1, 1};
      std::vector<float> p(S), c(S);
      rl_dirichlet_row_normalise(g, sum, S, 8, p8);
      rl_mdp_row_cumulative(p8, S, 8, c8);
      rl_dirichlet_row_normalise(g, sum, S, S, p.data());
      rl_mdp_row_cumulative(p.data(), S, S, c.data());
      for (uint32_t j = 0; j < 8; ++j) {
        if (j < S) same = same && f32_bits(p8[j]) == f32_bits(p[j]) && f32_bits(c8[j]) == f32_bits(c[j]);
        else same = same && p8[j] == 0.0f && c8[j] == 1.0f;  // the padding stays
      }
      // the rule itself: running sums up to the last positive entry, exactly 1 from there on
      float acc = 0.0f;
      uint32_t last = 0;
      for (uint32_t j = 0; j < S; ++j)
        if (p[j] > 0.0f) last = j;
      for (uint32_t j = 0; j < S; ++j) {
        acc = acc + p[j];
        same = same && f32_bits(c[j]) == f32_bits(j >= last ? 1.0f : acc);
        with_zero += p[j] == 0.0f;
      }
      checked += 1;
    }
  return std::string("{\"same\": ") + (same ? "true" : "false") + ", \"rows\": " + std::to_string(checked) +
         ", \"zero_entries\": " + std::to_string(with_zero) + "}";
}

struct ScalarCase {
  uint64_t S, A, E, L;
  double alpha, reward_stddev;
  uint64_t seed;
};

static std::string scalar_json() {
  using namespace relearn;
  const std::vector<ScalarCase> cases = {{2, 2, 1, 1, 1.0, 1.0, 11}, {3, 2, 2, 3, 1.0, 0.0, 16}, {5, 5, 3, 4, 1.0, 1.0, 13},
                                         {8, 4, 2, 2, 0.5, 1.0, 14}, {4, 8, 2, 2, 2.5, 1.0, 15}, {10, 5, 2, 3, 1.0, 1.0, 17}};
  std::ostringstream o;
  o << "[";
  for (size_t ci = 0; ci < cases.size(); ++ci) {
    const ScalarCase &c = cases[ci];
    MetaRandomMdps env;
    env.dist.num_states = c.S, env.dist.num_actions = c.A;
    env.dist.transition_prior_dirichlet_alpha = c.alpha;
    env.max_inner_steps = c.L, env.episodes_per_trial = c.E, env.reward_stddev = c.reward_stddev;
    o << (ci ? ",\n " : "\n ") << "{\"S\": " << c.S << ", \"A\": " << c.A << ", \"E\": " << c.E << ", \"L\": " << c.L
      << ", \"alpha\": " << c.alpha << ", \"reward_stddev\": " << c.reward_stddev << ", \"seed\": " << c.seed
      << ", \"trial_steps\": " << env.trial_steps() << ", \"lanes\": {";
    const uint64_t lanes[3] = {0, 25, 69};
    for (size_t li = 0; li < 3; ++li) {
      Prng rng = Prng::seed_from_u64(c.seed);
      rng.set_stream(lanes[li]);
      MetaRandomMdps::State s = env.initial_state(rng);
      std::vector<float> reward, obs, term, cum;
      std::vector<double> mean;
      std::vector<int> flag;
      auto tables = [&](const MetaRandomMdps::State &st) {
        cum.insert(cum.end(), st.mdp.cumulative.begin(), st.mdp.cumulative.end());
        mean.insert(mean.end(), st.mdp.reward_mean.begin(), st.mdp.reward_mean.end());
      };
      tables(s);
      const uint64_t steps = 3 * env.trial_steps() + 1;
      for (uint64_t t = 0; t < steps; ++t) {
        auto [succ, r] = env.step(std::move(s), (3 * t + lanes[li]) % c.A, rng);
        reward.push_back((float)r);
        flag.push_back((int)succ.kind);
        if (succ.kind == SuccessorKind::Interrupt) {
          const auto f = env.observe(*succ.state, rng);
          term.insert(term.end(), f.begin(), f.end());
          s = env.initial_state(rng);
          tables(s);
        } else {
          s = std::move(*succ.state);
        }
        const auto f = env.observe(s, rng);
        obs.insert(obs.end(), f.begin(), f.end());
      }
      o << (li ? ", " : "") << "\"" << lanes[li] << "\": {\"reward\": " << list_of(reward, f32_bits)
        << ", \"flag\": " << list_of(flag, [](int v) { return v; }) << ", \"obs\": " << list_of(obs, f32_bits)
        << ", \"term_obs\": " << list_of(term, f32_bits) << ", \"cum\": " << list_of(cum, f32_bits)
        << ", \"mean\": " << list_of(mean, f64_bits) << "}";
    }
    o << "}}";
  }
  o << "]";
  // what the scalar env refuses takes the error path
  int refused = 0;
  for (int bad = 0; bad < 4; ++bad) {
    MetaRandomMdps env;
    if (bad == 0) env.max_inner_steps = 0;
    if (bad == 1) env.episodes_per_trial = 0;
    if (bad == 2) env.reward_stddev = -1.0;
    if (bad == 3) env.dist.transition_prior_dirichlet_alpha = 0.0;
    Prng rng = Prng::seed_from_u64(1);
    try {
      env.initial_state(rng);
    } catch (const std::invalid_argument &) {
      refused += 1;
    }
  }
  return "{\"cases\": " + o.str() + ", \"refused\": " + std::to_string(refused) + "}";
}

// Prng::word_pos against a count of the words taken
static std::string word_pos_json() {
  relearn::Prng rng = relearn::Prng::seed_from_u64(5);
  bool ok = rng.word_pos() == 0;
  rng.set_stream(7);
  ok = ok && rng.word_pos() == 0 && rng.stream() == 7;
  uint64_t taken = 0;
  for (int i = 0; i < 300; ++i) {
    if (i % 3 == 0) rng.next_u32(), taken += 1;
    else rng.next_u64(), taken += 2;
    ok = ok && rng.word_pos() == taken;
  }
  relearn::Prng other = relearn::Prng::seed_from_u64(5);
  other.set_stream(7);
  other.set_word_pos(rng.word_pos());
  ok = ok && other.word_pos() == taken && other.next_u64() == rng.next_u64();
  return ok ? "true" : "false";
}

int main() {
  std::cout << "{\"spec\": " << spec_json() << ",\n \"fused\": " << fused_json() << ",\n \"paths\": " << paths_json()
            << ",\n \"rows\": " << rows_json() << ",\n \"word_pos\": " << word_pos_json() << ",\n \"scalar\": " << scalar_json()
            << "}\n";
  return 0;
}
