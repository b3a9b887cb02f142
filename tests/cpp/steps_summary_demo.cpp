// steps_summary_demo.cpp — train_batched with the device StepsSummary (relearn_amd/csrc/host/agents.hpp:
// StepsSummaryLanes): the examples/cartpole-trpo.rs agent for two periods, logging the full set of
// src/simulation/train.rs:160-175.  Prints one JSON object with the logged scalars, counters and durations, which
// tests/test_gpu_steps_summary.py compares with the same run driven through the ctypes binding.
#include <cinttypes>
#include <cstdio>

#include "../../relearn_amd/csrc/host/agents.hpp"

using namespace relearn;

// both Display forms, newlines escaped for JSON
static std::string log_summary_display(StepsSummaryLanes &summary) {
  rl_steps_summary raw{};
  raw.step_reward = rl_mean_variance{1.0, 0.0, 8};
  raw.episode_reward = rl_mean_variance{2.5, 1.0, 4};
  raw.episode_length = rl_mean_variance{2.5, 1.0, 4};
  std::string out;
  for (const std::string &s : {StepsSummary(raw).display(3), summary.read().display(3)}) {
    if (!out.empty()) out += "\\n";
    for (char c : s) {
      if (c == '\n') out += "\\n";
      else out += c;
    }
  }
  return out;
}

int main() {
  try {
    Engine eng(0);
    CartPoleLanes env(eng, 256, 500, StepLimit::Visible, /*seed_env=*/0, /*seed_actor=*/1);
    ActorCriticConfig<TrpoConfig<MlpConfig>, ValuesOptConfig<MlpConfig>> cfg;
    cfg.critic_config.opt_steps_per_update = 5;
    auto agent = cfg.build_agent(env, /*seed=*/2);
    DeviceHistory history = agent->buffer(32);
    StepsSummaryLanes summary(eng, env.num_lanes());
    RecordingLogger log;
    train_batched(*agent, env, history, 2, log, summary);
    std::printf("{\"scalars\": {");
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
    std::printf("}, \"durations\": [");
    first = true;
    for (auto &kv : log.durations) {
      std::printf("%s\"%s\"", first ? "" : ", ", kv.first.c_str());
      first = false;
    }
    // the reference's `{:.3}` Display of a StepsSummary: the last period's, and the empty one the clear left behind
    std::string shown = log_summary_display(summary);
    std::printf("], \"display\": \"%s\"}\n", shown.c_str());
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
