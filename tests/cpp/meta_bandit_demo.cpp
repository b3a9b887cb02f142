// meta_bandit_demo.cpp — the meta-RL bandit lanes over the C++ host API (relearn_amd/csrc/host/agents.hpp), the way
// relearn_experiments/src/bin/rl2-bandits.rs puts them together: MetaEnv over OneHotBandits(2) under a
// TrialEpisodeLimit of 3 episodes (MetaBanditLanes), a GRU(16) -> MLP([16]) policy under TRPO and a critic of the same
// shape fitted to the reward-to-go (GAE lambda 0.3), ActorCriticAgent::batch_update.  64 lanes, two periods of two whole
// trials (10 steps) each.
// Prints one JSON object: checksums of both modules' parameters and everything the RecordingLogger took, which
// tests/test_host_meta_bandit_cpp.py compares with the same two periods driven through the ctypes binding.
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
    MetaBanditLanes env(eng, lanes, /*n_arms=*/2, episodes_per_trial, RL_BANDITS_ONE_HOT, /*seed_env=*/61,
                        /*seed_actor=*/62);
    if (env.num_observation_features() != 6 || env.num_actions() != 2 || env.discount_factor() != 1.0) return 2;
    ActorCriticConfig<TrpoConfig<GruMlpConfig>, ValuesOptConfig<GruMlpConfig>> cfg;
    for (GruMlpConfig *c : {&cfg.policy_config.policy_fn_config, &cfg.critic_config.state_value_fn_config}) {
      c->hidden_dim = 16;
      c->second_config.hidden_sizes = {16};
    }
    cfg.critic_config.gae_lambda = 0.3;
    cfg.critic_config.opt_steps_per_update = 5;
    auto agent = cfg.build_agent(env, /*seed=*/63);
    DeviceHistory history = agent->buffer(horizon);
    RecordingLogger log;
    train_batched(*agent, env, history, periods, log);
    std::printf("{\"policy_checksum\": %.17g, \"critic_checksum\": %.17g, \"status\": %d, \"scalars\": {",
                checksum(agent->policy_module().parameters()), checksum(agent->critic_module()->parameters()),
                (int)agent->last_status());
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
