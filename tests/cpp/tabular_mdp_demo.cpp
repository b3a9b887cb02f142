// tabular_mdp_demo.cpp — tabular-MDP lanes over the C++ host API (relearn_amd/csrc/host/agents.hpp, host/envs.hpp): one
// MDP of four states and three actions from DirichletRandomMdps::sample_environment (seed 5, stream 0), stepped as a scalar
// env (TabularMdp, 20 steps on the stream of lane 0) and as 64 lanes under a visible limit of 8 (TabularMdpLanes) with a
// feed-forward TRPO policy and a critic of one hidden layer of 16, ActorCriticAgent::batch_update; two periods of one
// whole episode each.
// Prints one JSON object: checksums of the sampled tables, of the scalar env's rewards and states, of both modules'
// parameters and everything the RecordingLogger took, which tests/test_host_tabular_mdp_cpp.py compares with the same
// work driven through the ctypes binding.
#include <cinttypes>
#include <cstdio>

#include "../../relearn_amd/csrc/host/agents.hpp"

using namespace relearn;

template <typename T>
static double checksum(const std::vector<T> &p) {
  double s = 0.0;
  for (size_t i = 0; i < p.size(); ++i) s += (double)p[i] * (double)(1 + (i % 7));
  return s;
}

int main() {
  try {
    const uint64_t lanes = 64, limit = 8, periods = 2, seed_env = 61, seed_actor = 62;
    DirichletRandomMdps dist;  // Default: 10 x 5 — the lanes end at 8 x 8
    if (dist.num_states != 10 || dist.num_actions != 5) return 2;
    dist.num_states = 4;
    dist.num_actions = 3;
    const TabularMdp mdp = dist.sample_environment(/*seed=*/5, /*stream=*/0);
    // the scalar env on the stream of lane 0: what the first lane of a limit-free handle does
    Prng rng = Prng::seed_from_u64(seed_env);
    rng.set_stream(0);
    rng.set_word_pos(0);
    std::vector<float> rewards;
    std::vector<double> states;
    TabularMdp::State s = mdp.initial_state(rng);
    for (uint64_t t = 0; t < 20; ++t) {
      auto [succ, reward] = mdp.step(s, t % 3, rng);
      rewards.push_back((float)reward);
      s = *succ.state;
      states.push_back((double)s);
    }
    Engine eng(0);
    TabularMdpLanes env(eng, lanes, mdp, limit, StepLimit::Visible, seed_env, seed_actor);
    if (env.num_observation_features() != 5 || env.num_actions() != 3 || env.discount_factor() != 1.0) return 3;
    ActorCriticConfig<TrpoConfig<MlpConfig>, ValuesOptConfig<MlpConfig>> cfg;
    cfg.policy_config.policy_fn_config.hidden_sizes = {16};
    cfg.critic_config.state_value_fn_config.hidden_sizes = {16};
    cfg.critic_config.gae_lambda = 0.95;
    cfg.critic_config.opt_steps_per_update = 5;
    auto agent = cfg.build_agent(env, /*seed=*/63);
    DeviceHistory history = agent->buffer(limit);
    RecordingLogger log;
    train_batched(*agent, env, history, periods, log);
    std::printf("{\"transitions_checksum\": %.17g, \"reward_mean_checksum\": %.17g, \"scalar_rewards_checksum\": %.17g, "
                "\"scalar_states_checksum\": %.17g, \"policy_checksum\": %.17g, \"critic_checksum\": %.17g, \"status\": %d, "
                "\"scalars\": {",
                checksum(mdp.transitions), checksum(mdp.reward_mean), checksum(rewards), checksum(states),
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
