// partition_demo.cpp — the partition-game experiment's agent over the C++ host API (relearn_amd/csrc/host/agents.hpp,
// host/envs.hpp): PartitionGame under a VisibleStepLimit of 3 steps (24 observation features) — PartitionGameLanes, 64
// lanes — a GRU(16) -> ReLU -> MLP([16]) policy of two outputs under TRPO and a critic of the same shape with one output,
// ActorCriticAgent::batch_update; two periods of 7 steps, so that an episode runs across them.  What this size routes
// differently in the host mirror: the lanes go through rl_env_create_partition, GruMlpConfig::build_module through
// rl_rnn_chain_create_wide24 (24 inputs, for the policy and for the critic), DeviceHistory through rl_traj_create_wide24
// (24 planes).  A wrong threshold in either of the last two is a refusal by an older entry point, and this program exits 1.
// Before that, the scalar env WithVisibleStepLimit<PartitionGame> (host/envs.hpp: the mirror's own wrapper, what the
// CPU-only configuration runs) on the streams of lanes 0 and 63 against the lanes themselves: 8 driven steps (two episodes
// and two steps), rewards, successor codes and observations — the limit's `remaining` among them — compared inside this
// program.
// Prints one JSON object: the driven steps' checksums, the parameter counts, checksums of both modules' parameters and
// everything the RecordingLogger took, which tests/test_host_partition_cpp.py compares with the same work driven through
// the ctypes binding.
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

// a scalar observation against lane `lane` of the lanes' [D][lanes] plane
static bool same_obs(const std::vector<float> &f, const std::vector<float> &lanes_obs, uint64_t lanes, uint64_t lane) {
  for (size_t d = 0; d < f.size(); ++d)
    if (f[d] != lanes_obs[d * lanes + lane]) return false;
  return true;
}

int main() {
  try {
    const uint64_t lanes = 64, max_steps = 3, horizon = 7, periods = 2, seed_env = 91, seed_actor = 92;
    Engine eng(0);
    std::vector<float> driven_rewards, driven_obs;
    {
      PartitionGameLanes env(eng, lanes, max_steps, StepLimit::Visible, seed_env, seed_actor);
      if (env.num_observation_features() != 24 || env.num_actions() != 2 || env.discount_factor() != 0.999) return 2;
      // the scalar env the CPU-only configuration runs: the mirror's own visible step limit around PartitionGame
      const WithVisibleStepLimit<PartitionGame> scalar{PartitionGame{}, max_steps};
      if (scalar.num_observation_features() != 24 || scalar.num_actions() != 2) return 3;
      const uint64_t watch[2] = {0, 63};
      Prng rng[2];
      WithVisibleStepLimit<PartitionGame>::State state[2];
      const std::vector<float> first = env.observe();
      for (int w = 0; w < 2; ++w) {
        rng[w] = Prng::seed_from_u64(seed_env);
        rng[w].set_stream(watch[w]);
        state[w] = scalar.initial_state(rng[w]);
        if (!same_obs(scalar.observe(state[w], rng[w]), first, lanes, watch[w])) return 4;
      }
      uint64_t cuts = 0;
      for (uint64_t t = 0; t < 8; ++t) {
        std::vector<uint8_t> actions(lanes);
        for (uint64_t i = 0; i < lanes; ++i) actions[i] = (uint8_t)((t + i) % 2);
        const EnvLanes::StepResult r = env.step(actions);
        for (int w = 0; w < 2; ++w) {
          auto [succ, reward] = scalar.step(std::move(state[w]), actions[watch[w]], rng[w]);
          if ((float)reward != r.reward[watch[w]] || (uint8_t)succ.kind != r.successor[watch[w]]) return 5;
          if (succ.kind == SuccessorKind::Interrupt) {
            if (!same_obs(scalar.observe(*succ.state, rng[w]), r.interrupt_obs, lanes, watch[w])) return 6;
            state[w] = scalar.initial_state(rng[w]);
            cuts += 1;
          } else {
            state[w] = std::move(*succ.state);
          }
          if (!same_obs(scalar.observe(state[w], rng[w]), r.next_obs, lanes, watch[w])) return 8;
        }
        driven_rewards.insert(driven_rewards.end(), r.reward.begin(), r.reward.end());
        driven_obs.insert(driven_obs.end(), r.next_obs.begin(), r.next_obs.end());
      }
      if (cuts != 4) return 9;  // episodes of 3 steps in 8: two ends on each watched lane
    }
    PartitionGameLanes env(eng, lanes, max_steps, StepLimit::Visible, seed_env, seed_actor);
    ActorCriticConfig<TrpoConfig<GruMlpConfig>, ValuesOptConfig<GruMlpConfig>> cfg;
    cfg.policy_config.policy_fn_config.hidden_dim = 16;
    cfg.policy_config.policy_fn_config.second_config.hidden_sizes = {16};
    cfg.critic_config.state_value_fn_config.hidden_dim = 16;
    cfg.critic_config.state_value_fn_config.second_config.hidden_sizes = {16};
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
