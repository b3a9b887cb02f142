// dqn_gru_bandit_demo.cpp — the reference's GRU acceptance test of DQN over the C++ host API (relearn_amd/csrc/host/
// agents.hpp): src/torch/agents/tests/dqn.rs `default_gru_mlp_learns_derministic_bandit` runs
// `testing::train_deterministic_bandit(&config, 10, 0.9)` (src/agents/testing.rs:14-64) with DqnConfig<GruMlpConfig,
// AdamConfig> at learning rate 0.1, minibatch_steps 10, update_size Constant(10) and the defaults otherwise, on
// DeterministicBandit::from_values([0.0, 1.0]): 10 training periods, then 1,000 greedy evaluation steps, of which at least
// 900 must pull arm 1.  DqnConfig over a recurrent module configuration builds through rl_dqn_create_recurrent.
// usage: dqn_gru_bandit_demo [rtg|td]
// Prints one JSON object: how often the greedy actor pulled arm 1 and a checksum of the trained parameters, which
// tests/test_host_recurrent_dqn_cpp.py compares with the same run through the ctypes binding.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../relearn_amd/csrc/host/agents.hpp"

using namespace relearn;

static double checksum(const std::vector<float> &p) {
  double s = 0.0;
  for (size_t i = 0; i < p.size(); ++i) s += (double)p[i] * (double)(1 + (i % 7));
  return s;
}

int main(int argc, char **argv) {
  try {
    const bool td = argc > 1 && std::strcmp(argv[1], "td") == 0;
    const uint64_t lanes = 10;
    Engine eng(0);
    DeterministicBanditLanes env(eng, lanes, 0.0, 1.0, /*seed_env=*/1, /*seed_actor=*/2);
    DqnConfig<GruMlpConfig, AdamConfig> cfg;
    static_assert(builds_recurrent_module<GruMlpConfig>::value && !builds_recurrent_module<MlpConfig>::value,
                  "the GRU chain builds the recurrent agent, the MLP the feed-forward one");
    cfg.optimizer_config.learning_rate = 0.1;
    cfg.one_step_td = td;
    cfg.minibatch_steps = 10;
    cfg.update_first = cfg.update_rest = 10;
    cfg.buffer_capacity = 128 * lanes;  // (ten periods write 10 steps per lane at the most)
    const uint32_t key[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    auto agent = build_dqn_agent(cfg, env, /*seed=*/7, key);
    RecordingLogger log;
    for (int period = 0; period < 10; ++period) {
      agent->collect(log);
      agent->batch_update(log);
    }
    // the evaluation actor (ActorMode::Evaluation: exploration rate 0, schedules.rs:38): a second agent at rate 0 with
    // the trained parameters collects 100 steps per lane on lanes of its own; its recorded actions are the greedy ones
    DeterministicBanditLanes eval_env(eng, lanes, 0.0, 1.0, /*seed_env=*/1, /*seed_actor=*/2);
    DqnConfig<GruMlpConfig, AdamConfig> eval_cfg = cfg;
    eval_cfg.exploration_start = eval_cfg.exploration_end = 0.0;
    auto greedy = build_dqn_agent(eval_cfg, eval_env, /*seed=*/7, key);
    greedy->action_value_fn().set_parameters(agent->action_value_fn().parameters());
    check(rl_dqn_collect(greedy->handle(), 100, nullptr), eng.handle());
    uint64_t bytes = 0;
    check(rl_dqn_replay_field_bytes(greedy->handle(), RL_REPLAY_ACTION, &bytes), eng.handle());
    std::vector<uint8_t> actions(bytes);  // [capacity][lanes]
    check(rl_dqn_replay_read(greedy->handle(), RL_REPLAY_ACTION, actions.data(), bytes), eng.handle());
    uint64_t ones = 0;
    for (uint64_t i = 0; i < 100 * lanes; ++i) ones += actions[i];
    std::printf("{\"target\": \"%s\", \"arm1\": %llu, \"steps\": 1000, \"checksum\": %.17g, \"loss\": %.17g}\n",
                td ? "td" : "rtg", (unsigned long long)ones, checksum(agent->action_value_fn().parameters()),
                log.scalars["loss"]);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
