// thompson_agents_demo.cpp — the Thompson-sampling baselines over the C++ host API (relearn_amd/csrc/host/agents.hpp), the
// way the `eval` half of relearn_experiments/src/bin/rl2-bandits.rs puts them together: MetaEnv over
// UniformBernoulliBandits(3) under a TrialEpisodeLimit of 4 episodes (MetaBanditLanes), a ResettingMetaAgent over
// BetaThompsonSamplingAgentConfig — TS (num_samples 1) and OTS (10) — 70 lanes, two collections of 10 steps (a trial is
// 7: the horizon cuts trials, the second collection carries on), a StepsSummary of both.
// Prints one JSON object per agent in a list: checksums of the planes of both collections, the agent's state and the
// summary, which tests/test_host_thompson_cpp.py compares with the same collections through the ctypes binding.
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

template <typename T>
static std::vector<T> plane(const DeviceHistory &h, int32_t field, uint64_t count) {
  std::vector<T> v(count);
  check(rl_traj_read(h.handle(), field, v.data(), count * sizeof(T)));
  return v;
}

static void run(Engine &eng, const char *name, const BetaThompsonSamplingAgentConfig &config, bool last) {
  const uint64_t lanes = 70, episodes_per_trial = 4, horizon = 10;
  MetaBanditLanes env(eng, lanes, /*n_arms=*/3, episodes_per_trial, RL_BANDITS_UNIFORM_BERNOULLI, /*seed_env=*/71,
                      /*seed_actor=*/72);
  ResettingMetaAgent agent(env, config);
  DeviceHistory history(eng, lanes, horizon, env.num_observation_features());
  StepsSummaryLanes summary(eng, lanes);
  std::printf("{\"agent\": \"%s\", \"collections\": [", name);
  for (int period = 0; period < 2; ++period) {
    agent.collect(env, history);
    summary.push(history);
    const uint64_t B = lanes * horizon, D = env.num_observation_features();
    std::printf("%s{\"obs\": %.17g, \"action\": %.17g, \"reward\": %.17g, \"flag\": %.17g}", period ? ", " : "",
                checksum(plane<float>(history, RL_TRAJ_OBS, D * (horizon + 1) * lanes)),
                checksum(plane<uint8_t>(history, RL_TRAJ_ACTION, B)), checksum(plane<float>(history, RL_TRAJ_REWARD, B)),
                checksum(plane<uint8_t>(history, RL_TRAJ_FLAG, B)));
  }
  std::printf("], \"pos\": %.17g, \"low\": %.17g, \"high\": %.17g", checksum(agent.actor_word_positions()),
              checksum(agent.low_reward_counts()), checksum(agent.high_reward_counts()));
  const StepsSummary s = summary.read();
  std::printf(", \"trials\": %" PRIu64 ", \"trial_reward_mean\": %.17g, \"trial_reward_stddev\": %.17g}%s\n",
              s.num_episodes(), *s.episode_reward.mean(), *s.episode_reward.stddev(), last ? "" : ",");
}

int main() {
  try {
    Engine eng(0);
    std::printf("[\n");
    run(eng, "ts", BetaThompsonSamplingAgentConfig{}, false);
    run(eng, "ots", BetaThompsonSamplingAgentConfig{10}, true);
    std::printf("]\n");
    // the reference's Default impl
    const BetaThompsonSamplingAgentConfig t;
    if (t.num_samples != 1 || t.raw().kind != RL_BANDIT_AGENT_THOMPSON || t.raw().initial_action_count != 1) return 2;
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
