// meta_mdp_wide_demo.cpp — the second task of the RL2 paper at the reference's size over the C++ host API
// (relearn_amd/csrc/host/agents.hpp, host/envs.hpp): MetaEnv over DirichletRandomMdps of TEN states and FIVE actions
// (DirichletRandomMdps::default's sizes: 19 observation features) under a LatentStepLimit of 2 steps and a
// TrialEpisodeLimit of 2 episodes (trials of 5 steps) — MetaMdpLanes, 64 lanes — a GRU(16) -> ReLU -> Linear policy of five
// outputs under TRPO and a critic of the same shape with one output (GAE lambda 0.3), ActorCriticAgent::batch_update; two
// periods of 12 steps, so that a trial runs across them.  What this size routes differently in the host mirror: the lanes
// go through rl_env_create_meta_mdp_wide (rows of sixteen floats), GruLinearConfig::build_module through
// rl_rnn_chain_create_wide20 (19 inputs, for the policy and for the critic), DeviceHistory through rl_traj_create_wide
// (19 planes).  A wrong threshold in any of the three is a refusal by the older entry point, and this program exits 1.
// Before that, the scalar env MetaRandomMdps on the streams of lanes 0 and 63 against the lanes themselves: 11 driven
// steps (two trials and a step), rewards, successor codes and observations compared inside this program, and the tables
// the lanes read back — at the logical width of ten — against the scalar env's.
// Prints one JSON object: the driven steps' checksums, the parameter counts, checksums of both modules' parameters and
// everything the RecordingLogger took, which tests/test_host_meta_mdp_wide_cpp.py compares with the same work driven
// through the ctypes binding.
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
    const uint64_t lanes = 64, inner = 2, episodes = 2, horizon = 12, periods = 2, seed_env = 91, seed_actor = 92;
    DirichletRandomMdps dist;
    dist.num_states = 10;
    dist.num_actions = 5;
    dist.transition_prior_dirichlet_alpha = 0.5;
    Engine eng(0);
    std::vector<float> driven_rewards, driven_obs;
    {
      MetaMdpLanes env(eng, lanes, dist, inner, episodes, /*reward_stddev=*/0.5, seed_env, seed_actor);
      if (env.num_observation_features() != 19 || env.num_actions() != 5 || env.discount_factor() != 1.0) return 2;
      if (env.trial_steps() != 5) return 3;
      MetaRandomMdps scalar;
      scalar.dist = dist, scalar.max_inner_steps = inner, scalar.episodes_per_trial = episodes, scalar.reward_stddev = 0.5;
      const uint64_t watch[2] = {0, 63};
      Prng rng[2];
      MetaRandomMdps::State state[2];
      for (int w = 0; w < 2; ++w) {
        rng[w] = Prng::seed_from_u64(seed_env);
        rng[w].set_stream(watch[w]);
        state[w] = scalar.initial_state(rng[w]);
        const MetaMdpLanes::Tables t = env.read_tables(watch[w], 1);
        if (t.cumulative != state[w].mdp.cumulative || t.reward_mean != state[w].mdp.reward_mean) return 4;
      }
      for (uint64_t t = 0; t < 11; ++t) {
        std::vector<uint8_t> actions(lanes);
        for (uint64_t i = 0; i < lanes; ++i) actions[i] = (uint8_t)((t + i) % 5);
        const EnvLanes::StepResult r = env.step(actions);
        for (int w = 0; w < 2; ++w) {
          auto [succ, reward] = scalar.step(std::move(state[w]), actions[watch[w]], rng[w]);
          if ((float)reward != r.reward[watch[w]] || (uint8_t)succ.kind != r.successor[watch[w]]) return 5;
          if (succ.kind == SuccessorKind::Interrupt) {
            const std::vector<float> f = scalar.observe(*succ.state, rng[w]);
            for (size_t d = 0; d < f.size(); ++d)
              if (f[d] != r.interrupt_obs[d * lanes + watch[w]]) return 6;
            state[w] = scalar.initial_state(rng[w]);
            const MetaMdpLanes::Tables tb = env.read_tables(watch[w], 1);
            if (tb.cumulative != state[w].mdp.cumulative || tb.reward_mean != state[w].mdp.reward_mean) return 7;
          } else {
            state[w] = std::move(*succ.state);
          }
          const std::vector<float> f = scalar.observe(state[w], rng[w]);
          for (size_t d = 0; d < f.size(); ++d)
            if (f[d] != r.next_obs[d * lanes + watch[w]]) return 8;
        }
        driven_rewards.insert(driven_rewards.end(), r.reward.begin(), r.reward.end());
        driven_obs.insert(driven_obs.end(), r.next_obs.begin(), r.next_obs.end());
      }
    }
    MetaMdpLanes env(eng, lanes, dist, inner, episodes, /*reward_stddev=*/0.5, seed_env, seed_actor);
    ActorCriticConfig<TrpoConfig<GruLinearConfig>, ValuesOptConfig<GruLinearConfig>> cfg;
    cfg.policy_config.policy_fn_config.hidden_dim = 16;
    cfg.critic_config.state_value_fn_config.hidden_dim = 16;
    cfg.critic_config.gae_lambda = 0.3;
    cfg.critic_config.opt_steps_per_update = 5;
    auto agent = cfg.build_agent(env, /*seed=*/93);
    DeviceHistory history = agent->buffer(horizon);
    RecordingLogger log;
    train_batched(*agent, env, history, periods, log);
    const std::vector<float> pp = agent->policy_module().parameters(), cp = agent->critic_module()->parameters();
    std::printf("{\"driven_rewards_checksum\": %.17g, \"driven_obs_checksum\": %.17g, \"policy_params\": %zu, "
                "\"critic_params\": %zu, \"policy_checksum\": %.17g, \"critic_checksum\": %.17g, \"status\": %d, \"scalars\": {",
                checksum(driven_rewards), checksum(driven_obs), pp.size(), cp.size(), checksum(pp), checksum(cp),
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
