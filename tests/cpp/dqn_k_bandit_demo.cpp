// dqn_k_bandit_demo.cpp — the reference's DQN acceptance test at four arms over the C++ host API (relearn_amd/csrc/host/
// agents.hpp): `testing::train_deterministic_bandit(&config, 10, 0.9)` (src/agents/testing.rs:14-64) with
// DqnConfig<MlpConfig, AdamConfig> over hidden_sizes [16, 16] at learning rate 0.1, minibatch_steps 10, update_size
// Constant(10) and the defaults otherwise, on DeterministicBandit::from_values([0.0, 0.0, 0.0, 1.0]): 10 training periods,
// then 1,000 greedy evaluation steps, of which at least 900 must pull arm 3.  An env of more than two actions builds its
// agent through rl_dqn_create_finite (DqnConfig is generic over the action space: AS: FiniteSpace, dqn.rs:75-86).
// usage: dqn_k_bandit_demo [rtg|td]
// Prints one JSON object: how often the greedy actor pulled the best arm and a checksum of the trained parameters, which
// tests/test_host_dqn_k_bandit_cpp.py compares with the same run through the ctypes binding.
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
    const std::vector<double> values{0.0, 0.0, 0.0, 1.0};
    Engine eng(0);
    DeterministicBanditLanes env(eng, lanes, values, /*seed_env=*/1, /*seed_actor=*/2);
    if (env.num_actions() != values.size()) return 2;
    DqnConfig<MlpConfig, AdamConfig> cfg;
    cfg.action_value_fn_config.hidden_sizes = {16, 16};
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
    DeterministicBanditLanes eval_env(eng, lanes, values, /*seed_env=*/1, /*seed_actor=*/2);
    DqnConfig<MlpConfig, AdamConfig> eval_cfg = cfg;
    eval_cfg.exploration_start = eval_cfg.exploration_end = 0.0;
    auto greedy = build_dqn_agent(eval_cfg, eval_env, /*seed=*/7, key);
    greedy->action_value_fn().set_parameters(agent->action_value_fn().parameters());
    check(rl_dqn_collect(greedy->handle(), 100, nullptr), eng.handle());
    uint64_t bytes = 0;
    check(rl_dqn_replay_field_bytes(greedy->handle(), RL_REPLAY_ACTION, &bytes), eng.handle());
    std::vector<uint8_t> actions(bytes);  // [capacity][lanes]
    check(rl_dqn_replay_read(greedy->handle(), RL_REPLAY_ACTION, actions.data(), bytes), eng.handle());
    uint64_t best = 0;
    for (uint64_t i = 0; i < 100 * lanes; ++i) best += actions[i] == values.size() - 1 ? 1 : 0;
    std::printf("{\"target\": \"%s\", \"arms\": %llu, \"best\": %llu, \"steps\": 1000, \"checksum\": %.17g, \"loss\": %.17g}\n",
                td ? "td" : "rtg", (unsigned long long)values.size(), (unsigned long long)best,
                checksum(agent->action_value_fn().parameters()), log.scalars["loss"]);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
