// dqn_bandit_demo.cpp — the reference's own DQN acceptance test over the C++ host API (relearn_amd/csrc/host/agents.hpp):
// src/torch/agents/tests/dqn.rs runs `testing::train_deterministic_bandit(&config, 10, 0.9)` (src/agents/testing.rs:14-64)
// with DqnConfig<MlpConfig, AdamConfig> at learning rate 0.1, minibatch_steps 10, update_size Constant(10) and the
// defaults otherwise, on DeterministicBandit::from_values([0.0, 1.0]): 10 training periods, then 1,000 greedy evaluation
// steps, of which at least 900 must pull arm 1.
// usage: dqn_bandit_demo [lanes]   (10 lanes x 1 step per period by default; 2 lanes x 5 steps with `2`)
// Prints one JSON object: how often the greedy actor pulled arm 1 and a checksum of the trained parameters, which
// tests/test_host_dqn_bandit_cpp.py compares with the same run through the ctypes binding.
#include <cstdio>
#include <cstdlib>

#include "../../relearn_amd/csrc/host/agents.hpp"

using namespace relearn;

static double checksum(const std::vector<float> &p) {
  double s = 0.0;
  for (size_t i = 0; i < p.size(); ++i) s += (double)p[i] * (double)(1 + (i % 7));
  return s;
}

int main(int argc, char **argv) {
  try {
    const uint64_t lanes = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 10;
    if (lanes < 1 || lanes > 10) return 2;
    Engine eng(0);
    DeterministicBanditLanes env(eng, lanes, 0.0, 1.0, /*seed_env=*/1, /*seed_actor=*/2);
    DqnConfig<MlpConfig, AdamConfig> cfg;
    cfg.optimizer_config.learning_rate = 0.1;
    cfg.minibatch_steps = 10;
    cfg.update_first = cfg.update_rest = 10;
    cfg.buffer_capacity = 4096 * lanes;  // (ten periods write 10 steps per lane at the most)
    const uint32_t key[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    auto agent = build_dqn_agent(cfg, env, /*seed=*/7, key);
    RecordingLogger log;
    for (int period = 0; period < 10; ++period) {
      agent->collect(log);
      agent->batch_update(log);
    }
    // the evaluation actor: the greedy action of the action-value module on the env's observation
    const uint32_t D = env.num_observation_features();
    uint64_t ones = 0, taken = 0;
    std::vector<float> rows(lanes * D), z(lanes * 2);
    std::vector<uint8_t> actions(lanes);
    while (taken < 1000) {
      const std::vector<float> obs = env.observe();  // [D][lanes]
      for (uint64_t i = 0; i < lanes; ++i)
        for (uint32_t d = 0; d < D; ++d) rows[i * D + d] = obs[d * lanes + i];
      check(rl_mlp_forward(agent->action_value_fn().handle(), rows.data(), lanes, z.data()), eng.handle());
      for (uint64_t i = 0; i < lanes; ++i) {
        actions[i] = z[2 * i + 1] > z[2 * i] ? 1 : 0;  // argmax: first maximal index
        if (taken + i < 1000) ones += actions[i];
      }
      taken += lanes;
      env.step(actions);
    }
    std::printf("{\"lanes\": %llu, \"arm1\": %llu, \"steps\": 1000, \"checksum\": %.17g, \"loss\": %.17g}\n",
                (unsigned long long)lanes, (unsigned long long)ones, checksum(agent->action_value_fn().parameters()),
                log.scalars["loss"]);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
