// rl2_wide_demo.cpp — the RL2 experiment at its default size, TEN arms, over the C++ host API
// (relearn_amd/csrc/host/agents.hpp): MetaEnv over UniformBernoulliBandits(10) (rl2-bandits.rs' --num-arms default) under
// a TrialEpisodeLimit of 3 episodes — MetaBanditLanes, which goes through rl_env_create_meta_bandit_wide above four arms —
// a GRU(16) -> ReLU -> Linear policy of ten outputs under TRPO and a critic of the same shape with one output fitted to
// the reward-to-go (GAE lambda 0.3), ActorCriticAgent::batch_update.  GruLinearConfig::build_module goes through
// rl_rnn_chain_create_wide above eight inputs or outputs: both modules here have 14 inputs.  64 lanes, two periods of two
// whole trials (10 steps) each.
// Prints one JSON object: the parameter counts, checksums of both modules' parameters and everything the RecordingLogger
// took, which tests/test_host_rl2_wide_cpp.py compares with the same two periods driven through the ctypes binding.
#include <cinttypes>
#include <cstdio>

#include "../../relearn_amd/csrc/host/agents.hpp"

using namespace relearn;

static double checksum(const std::vector<float> &p) {
  double s = 0.0;
  for (size_t i = 0; i < p.size(); ++i) s += (double)p[i] * (double)(1 + (i % 7));
  return s;
}

int main() {
  try {
    const uint64_t lanes = 64, episodes_per_trial = 3, horizon = 10, periods = 2;
    Engine eng(0);
    MetaBanditLanes env(eng, lanes, /*n_arms=*/10, episodes_per_trial, RL_BANDITS_UNIFORM_BERNOULLI, /*seed_env=*/71,
                        /*seed_actor=*/72);
    if (env.num_observation_features() != 14 || env.num_actions() != 10 || env.discount_factor() != 1.0) return 2;
    ActorCriticConfig<TrpoConfig<GruLinearConfig>, ValuesOptConfig<GruLinearConfig>> cfg;
    cfg.policy_config.policy_fn_config.hidden_dim = 16;
    cfg.critic_config.state_value_fn_config.hidden_dim = 16;
    cfg.critic_config.gae_lambda = 0.3;
    cfg.critic_config.opt_steps_per_update = 5;
    auto agent = cfg.build_agent(env, /*seed=*/73);
    DeviceHistory history = agent->buffer(horizon);
    RecordingLogger log;
    train_batched(*agent, env, history, periods, log);
    const std::vector<float> pp = agent->policy_module().parameters(), cp = agent->critic_module()->parameters();
    std::printf("{\"policy_params\": %zu, \"critic_params\": %zu, \"policy_checksum\": %.17g, \"critic_checksum\": %.17g, "
                "\"status\": %d, \"scalars\": {",
                pp.size(), cp.size(), checksum(pp), checksum(cp), (int)agent->last_status());
    bool first = true;
    for (auto &kv : log.scalars) {
      std::printf("%s\"%s\": %.17g", first ? "" : ", ", kv.first.c_str(), kv.second);
      first = false;
    }
    std::printf("}, \"counters\": {");
    first = true;
    for (auto &kv : log.counters) {
      std::printf("%s\"%s\": %" PRIu64, first ? "" : ", ", kv.first.c_str(), kv.second);
      first = false;
    }
    std::printf("}}\n");
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
