// rl2_chain_linear_demo.cpp — the agent of relearn_experiments/src/bin/rl2-bandits.rs over the C++ host API
// (relearn_amd/csrc/host/agents.hpp) with the experiment's model, `type Model = Chain<Gru, Linear>`
// (rl2-bandits.rs:349,379-394): ActorCriticConfig<TrpoConfig<GruLinearConfig>, ValuesOptConfig<GruLinearConfig>>,
// GRU -> ReLU -> Linear as policy and as critic, input weights Uniform(FanAvg), hidden weights Orthogonal, biases
// Zeros, LinearConfig::default; max_policy_step_kl 0.01, GAE lambda 0.3, 50 critic steps; hidden_dim 32 here.  MetaEnv
// over UniformBernoulliBandits(2) under a TrialEpisodeLimit of 3 episodes, 64 lanes, two periods of two whole trials
// (10 steps) each.
// Prints: the policy's and the critic's parameter counts, then the critic's loss of each period.
#include <cstdio>

#include "../../relearn_amd/csrc/host/agents.hpp"

using namespace relearn;

int main() {
  try {
    const uint64_t lanes = 64, episodes_per_trial = 3, horizon = 10, periods = 2;
    Engine eng(0);
    MetaBanditLanes env(eng, lanes, /*n_arms=*/2, episodes_per_trial, RL_BANDITS_UNIFORM_BERNOULLI, /*seed_env=*/71,
                        /*seed_actor=*/72);
    ActorCriticConfig<TrpoConfig<GruLinearConfig>, ValuesOptConfig<GruLinearConfig>> cfg;
    for (GruLinearConfig *c : {&cfg.policy_config.policy_fn_config, &cfg.critic_config.state_value_fn_config}) {
      c->first_config.input_weights_init = Initializer::Uniform(RL_SCALE_FAN_AVG);
      c->first_config.hidden_weights_init = Initializer::Orthogonal();
      c->first_config.bias_init = Initializer::Zeros();
      c->hidden_dim = 32;
      c->second_config = LinearConfig{};
    }
    cfg.policy_config.max_policy_step_kl = 0.01;
    cfg.critic_config.gae_lambda = 0.3;
    cfg.critic_config.opt_steps_per_update = 50;
    // (a Linear tail without a bias vector is refused when the agent is built)
    {
      auto bad = cfg;
      bad.critic_config.state_value_fn_config.second_config.bias_init = std::nullopt;
      try {
        bad.build_agent(env, 1);
        return 3;
      } catch (const BuildAgentError &) {
      }
    }
    auto agent = cfg.build_agent(env, /*seed=*/73);
    DeviceHistory history = agent->buffer(horizon);
    std::printf("%llu %llu", (unsigned long long)agent->policy_module().num_parameters(),
                (unsigned long long)agent->critic_module()->num_parameters());
    for (uint64_t period = 0; period < periods; ++period) {
      RecordingLogger log;
      agent->collect(env, history);
      eng.sync();
      agent->batch_update(history, log);
      if (log.scalars.count("critic/loss") != 1) return 2;
      std::printf(" %.9g", log.scalars.at("critic/loss"));
    }
    std::printf("\n");
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
