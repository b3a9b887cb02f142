// handle_spec_demo.cpp — the HIP-free half of the env and module constructors (relearn_amd/csrc/handle_spec.hpp) on the
// CPU: for every line of the case list (tests/constructor_cases.py prints it) what the constructor refuses — status code
// and words — or decides (D and A; P, the floats to allocate, the twin), the path of every rollout pair, and initial
// parameter vectors as f32 bit patterns.  One JSON document on stdout; tests/test_handle_spec_cpp.py compares it with
// the table recorded on the device and with the oracle.
//   g++ -std=c++17 -ffp-contract=off -Wall -Wextra -Werror -I <repo> tests/cpp/handle_spec_demo.cpp -o demo && ./demo <list>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

#include "relearn_amd/csrc/handle_spec.hpp"

using Nums = std::vector<std::string>;
static int64_t I(const Nums &n, size_t i) { return std::stoll(n.at(i)); }
static uint64_t U(const Nums &n, size_t i) { return std::stoull(n.at(i)); }
static double F(const Nums &n, size_t i) { return std::stod(n.at(i)); }

static std::string quoted(const std::string &s) {
  std::string out = "\"";
  for (char c : s) {
    if (c == '"' || c == '\\') out += '\\';
    out += c;
  }
  return out + "\"";
}

static rl_env_config env_config(int64_t kind, int64_t limit, uint64_t max_steps, uint64_t n_lanes, uint64_t chain_size = 0,
                                uint64_t mem_actions = 0, uint64_t mem_history = 0) {
  rl_env_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.kind = (int32_t)kind;
  cfg.limit_kind = (int32_t)limit;
  cfg.max_steps = max_steps;
  cfg.n_lanes = n_lanes;
  cfg.seed_env = 3;
  cfg.seed_actor = 4;
  cfg.cartpole = rl_cartpole_params{9.8, 1.0, 0.1, 0.5, 0.01, 0.01, 0.02, 10.0, 2.4, 0.20943951023931953, 0.99};
  cfg.chain_size = chain_size;
  cfg.memory_num_actions = mem_actions;
  cfg.memory_history_len = mem_history;
  cfg.bandit_values[0] = 0.0;
  cfg.bandit_values[1] = 1.0;
  return cfg;
}

// the numbers of each constructor: tests/constructor_cases.py
static EnvSpec env_of(const std::string &ctor_in, const Nums &n_in) {
  std::string ctor = ctor_in;
  Nums n = n_in;
  int64_t kind = RL_ENV_CARTPOLE;
  uint64_t mem_actions = 0, mem_history = 0;
  if (ctor.size() > 3 && ctor.substr(ctor.size() - 3) == "_as") {  // kind, MemoryGame shape, then the constructor's numbers
    kind = I(n, 0), mem_actions = U(n, 1), mem_history = U(n, 2);
    ctor.resize(ctor.size() - 3);
    n.erase(n.begin(), n.begin() + 3);
  }
  if (ctor == "env") return env_spec_basic(env_config(I(n, 0), I(n, 1), U(n, 2), U(n, 3), U(n, 4), U(n, 5), U(n, 6)));
  if (ctor == "bandit") {
    std::vector<double> values(U(n, 4));
    for (size_t a = 0; a < values.size(); ++a) values[a] = 0.5 * (double)a - 1.0;
    return env_spec_bandit(env_config(I(n, 0), I(n, 1), U(n, 2), U(n, 3)), values.data(), (uint32_t)values.size());
  }
  const rl_env_config cfg = env_config(kind, I(n, 0), U(n, 1), U(n, 2), 0, mem_actions, mem_history);
  if (ctor == "meta" || ctor == "meta_wide")
    return env_spec_meta(cfg, rl_meta_bandit_config{(uint32_t)U(n, 3), (int32_t)I(n, 4), U(n, 5)}, ctor == "meta_wide");
  const uint32_t S = (uint32_t)U(n, 3), A = (uint32_t)U(n, 4);
  const int64_t table = I(n, 6);
  std::vector<float> tr((size_t)S * A * S, (float)(1.0 / (double)S));
  std::vector<double> mean((size_t)S * A), sd((size_t)S * A, 0.5);
  for (size_t row = 0; row < mean.size(); ++row) mean[row] = 0.25 * (double)row;
  if (table == 1) tr[3 * S] = -0.5f;
  if (table == 2 || table == 6) tr[1 * S] = 0.0f;
  if (table == 3 || table == 6) mean[2] = INFINITY;
  if (table == 4) sd[1] = -1.0;
  return env_spec_mdp(cfg, rl_tabular_mdp_config{S, A, F(n, 5)}, tr.data(), mean.data(),
                      table == 4 || table == 5 ? sd.data() : nullptr);
}

static ModuleShape module_of(const std::string &ctor, const Nums &n) {
  auto chain = [](int64_t cell, uint64_t in, uint64_t H, uint64_t layers, int64_t bias, uint64_t H2, uint64_t out) {
    return rl_rnn_chain_config{(int32_t)cell, (uint32_t)in, (uint32_t)H, (uint32_t)layers, (int32_t)bias, (uint32_t)H2, (uint32_t)out};
  };
  if (ctor == "mlp") return fused_mlp_shape((uint32_t)U(n, 0), (uint32_t)U(n, 1), (uint32_t)U(n, 2));
  if (ctor == "mlp_layers" || ctor == "mlp_config") {
    const size_t k = ctor == "mlp_layers" ? 4 : 5;
    std::vector<uint32_t> widths(1, 0);  // (never an empty array)
    for (size_t i = k + 1; i < n.size(); ++i) widths.insert(widths.end() - 1, (uint32_t)U(n, i));
    return mlp_shape((uint32_t)U(n, 0), widths.data(), (uint32_t)U(n, k), (uint32_t)U(n, 1), (int32_t)I(n, 2), (int32_t)I(n, 3),
                     k == 4 || I(n, 4) != 0);
  }
  if (ctor == "gru_mlp") return chain_shape(chain(RL_CELL_GRU, U(n, 0), U(n, 1), 1, 1, U(n, 2), U(n, 3)), CHAIN_TWO_ACTIONS_MLP);
  if (ctor == "lstm_mlp") return chain_shape(chain(RL_CELL_LSTM, U(n, 0), U(n, 1), 1, 1, U(n, 2), U(n, 3)), CHAIN_TWO_ACTIONS_MLP);
  if (ctor == "rnn_mlp") return chain_shape(chain(I(n, 0), U(n, 1), U(n, 2), U(n, 3), 1, U(n, 4), U(n, 5)), CHAIN_TWO_ACTIONS_MLP);
  if (ctor == "rnn_mlp_config")  // (any non-zero flag builds the bias vectors: rl_rnn_mlp_create_config)
    return chain_shape(chain(I(n, 0), U(n, 1), U(n, 2), U(n, 3), I(n, 4) != 0, U(n, 5), U(n, 6)), CHAIN_TWO_ACTIONS_MLP);
  if (ctor == "rnn_linear")
    return chain_shape(chain(I(n, 0), U(n, 1), U(n, 2), U(n, 3), I(n, 4), 0, U(n, 5)), CHAIN_TWO_ACTIONS_LINEAR);
  const rl_rnn_chain_config cfg = chain(I(n, 0), U(n, 1), U(n, 2), U(n, 3), I(n, 4), U(n, 5), U(n, 6));
  if (ctor == "chain") return chain_shape(cfg, CHAIN_NARROW);
  if (ctor == "chain_wide") return chain_shape(cfg, chain_limits_wide(cfg));
  throw std::runtime_error("unknown constructor " + ctor);
}

// the modules of the init cases (constructor_cases.py: `module`)
static ModuleShape init_module(int64_t which) {
  const uint32_t three[1] = {3};
  if (which == 0 || which == 1) return mlp_shape(4, three, 1, 1, RL_ACT_RELU, RL_ACT_IDENTITY, which == 0);
  return chain_shape(rl_rnn_chain_config{RL_CELL_GRU, 4, 3, 1, which == 2, 3, 1}, CHAIN_TWO_ACTIONS_MLP);
}

// (given kind scale value) groups from position `at` on
static std::vector<rl_initializer> initializers(const Nums &n, size_t at, std::vector<bool> &given) {
  std::vector<rl_initializer> out;
  for (size_t i = at; i + 3 < n.size(); i += 4) {
    given.push_back(I(n, i) != 0);
    out.push_back(rl_initializer{(int32_t)I(n, i + 1), (int32_t)I(n, i + 2), F(n, i + 3)});
  }
  return out;
}

static bool is_env(const std::string &ctor) {
  return ctor == "env" || ctor == "bandit" || ctor.rfind("meta", 0) == 0 || ctor.rfind("mdp", 0) == 0;
}

static std::string refusal(const RlError &e) {
  return "{\"code\": " + std::to_string(e.code) + ", \"message\": " + quoted(e.what()) + "}";
}

static std::string run_case(const std::string &ctor, const Nums &n) {
  std::ostringstream o;
  try {
    if (ctor == "init_mlp" || ctor == "init_rnn") {
      const ModuleShape m = init_module(I(n, 0));
      std::vector<bool> given;
      const std::vector<rl_initializer> in = initializers(n, 1, given);
      auto ptr = [&](size_t i) { return given[i] ? &in[i] : nullptr; };
      if (ctor == "init_mlp") mlp_inits_checked(m, ptr(0), ptr(1));
      else chain_inits_checked(m, ptr(0), ptr(1), ptr(2), ptr(3), ptr(4));
      o << "{\"code\": 0}";
    } else if (is_env(ctor)) {
      const EnvSpec s = env_of(ctor, n);
      o << "{\"code\": 0, \"dims\": [" << s.D << ", " << s.A << "], \"kind\": " << s.cfg.kind << "}";
    } else {
      const ModuleShape m = module_of(ctor, n);
      o << "{\"code\": 0, \"params\": " << m.P << ", \"alloc_floats\": " << m.alloc_floats()
        << ", \"twin_params\": " << (m.needs_twin() ? chain_twin_shape(m).alloc_floats() : 0) << "}";
    }
  } catch (const RlError &e) {
    return refusal(e);
  }
  return o.str();
}

static const char *PATH_NAMES[] = {"ROLL_GENERAL", "ROLL_STACK", "ROLL_TILE_RECURRENT", "ROLL_INDEX_MLP", "ROLL_CARTPOLE"};

static std::string bits_of(const std::vector<float> &v) {
  std::ostringstream o;
  o << "[";
  for (size_t i = 0; i < v.size(); ++i) {
    uint32_t b;
    std::memcpy(&b, &v[i], 4);
    o << (i ? ", " : "") << b;
  }
  o << "]";
  return o.str();
}

// initvec NAME mlp SEED in_dim out_dim bias n_hidden widths.. then kernel and bias as (kind scale value)
// initvec NAME chain SEED cell in_dim hidden num_layers rnn_bias mlp_hidden out_dim then five (kind scale value)
static std::string init_vector(const std::string &what, const Nums &n) {
  const uint64_t seed = U(n, 0);
  auto init_at = [&](size_t i) { return rl_initializer{(int32_t)I(n, i), (int32_t)I(n, i + 1), F(n, i + 2)}; };
  if (what == "mlp") {
    const uint32_t n_hidden = (uint32_t)U(n, 4);
    std::vector<uint32_t> widths(n_hidden ? n_hidden : 1, 0);
    for (uint32_t l = 0; l < n_hidden; ++l) widths[l] = (uint32_t)U(n, 5 + l);
    const ModuleShape m = mlp_shape((uint32_t)U(n, 1), widths.data(), n_hidden, (uint32_t)U(n, 2), RL_ACT_TANH, RL_ACT_IDENTITY,
                                    I(n, 3) != 0);
    return bits_of(mlp_init_vector(m, seed, MlpInits{init_at(5 + n_hidden), init_at(8 + n_hidden)}));
  }
  const rl_rnn_chain_config cfg{(int32_t)I(n, 1), (uint32_t)U(n, 2), (uint32_t)U(n, 3), (uint32_t)U(n, 4), (int32_t)I(n, 5),
                                (uint32_t)U(n, 6), (uint32_t)U(n, 7)};
  return bits_of(chain_init_vector(chain_shape(cfg, CHAIN_NARROW), seed,
                                   RnnInits{init_at(8), init_at(11), init_at(14), init_at(17), init_at(20)}));
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::cerr << "usage: handle_spec_demo <case list>\n";
    return 2;
  }
  std::ifstream in(argv[1]);
  std::map<std::string, std::pair<std::string, Nums>> cases;
  std::vector<std::string> out_cases, out_rollouts, out_inits;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string what, name, word;
    ls >> what >> name;
    Nums rest;
    while (ls >> word) rest.push_back(word);
    if (what == "case") {
      const std::string ctor = rest.at(0);
      rest.erase(rest.begin());
      cases[name] = {ctor, rest};
      out_cases.push_back(quoted(name) + ": " + run_case(ctor, rest));
    } else if (what == "rollout") {
      const auto &env = cases.at(rest.at(0)), &mod = cases.at(rest.at(1));
      std::string got;
      try {
        const EnvSpec s = env_of(env.first, env.second);
        got = quoted(PATH_NAMES[rollout_path(s.cfg.kind, s.D, s.A, s.dev.chain_size, module_of(mod.first, mod.second))]);
      } catch (const RlError &e) {
        got = refusal(e);
      }
      out_rollouts.push_back(quoted(name) + ": " + got);
    } else if (what == "initvec") {
      const std::string kind = rest.at(0);
      rest.erase(rest.begin());
      out_inits.push_back(quoted(name) + ": " + init_vector(kind, rest));
    }
  }
  auto join = [](const std::vector<std::string> &v) {
    std::string s;
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ",\n  " : "\n  ") + v[i];
    return s;
  };
  std::cout << "{\"cases\": {" << join(out_cases) << "},\n \"rollouts\": {" << join(out_rollouts) << "},\n \"inits\": {"
            << join(out_inits) << "}}\n";
  return 0;
}
