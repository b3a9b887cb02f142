// The samplers of include/rl_normal.h and the host side of the tabular-MDP feature (relearn_amd/csrc/host/envs.hpp:
// DirichletRandomMdps::sample_environment, TabularMdp) as a stand-alone program for AddressSanitizer /
// UndefinedBehaviorSanitizer (tests/test_host_tabular_mdp_cpp.py builds and runs it on the CPU).  Prints a checksum so
// the work cannot be optimised away.
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "include/rl_normal.h"
#include "relearn_amd/csrc/host/envs.hpp"

int main() {
  using namespace relearn;
  double checksum = 0.0;
  uint32_t key[8];
  rl_seed_from_u64(11, key);
  uint64_t pos = 0;
  for (int i = 0; i < 2000; ++i) checksum += rl_normal_sample(key, 3, &pos);
  for (double alpha : {0.05, 0.5, 1.0, 2.5, 40.0})
    for (int i = 0; i < 500; ++i) checksum += rl_gamma_sample(alpha, key, 3, &pos);
  // the widest size the sampler takes, the reference's default, the smallest
  for (auto size : {std::pair<uint64_t, uint64_t>{64, 64}, {10, 5}, {1, 1}, {8, 8}}) {
    DirichletRandomMdps d;
    d.num_states = size.first;
    d.num_actions = size.second;
    d.transition_prior_dirichlet_alpha = size.first == 8 ? 0.25 : 1.0;
    const TabularMdp mdp = d.sample_environment(168, 2);
    Prng rng = Prng::seed_from_u64(170);
    TabularMdp::State s = mdp.initial_state(rng);
    for (uint64_t t = 0; t < 1000; ++t) {
      auto [succ, reward] = mdp.step(s, t % mdp.num_actions(), rng);
      s = *succ.state;
      if (s >= mdp.num_states) return 2;
      checksum += reward + (double)mdp.observe(s, rng);
    }
  }
  // what the sampler refuses takes the error path
  for (int bad = 0; bad < 4; ++bad) {
    DirichletRandomMdps d;
    if (bad == 0) d.num_states = 65;
    if (bad == 1) d.num_actions = 0;
    if (bad == 2) d.transition_prior_dirichlet_alpha = 0.0;
    if (bad == 3) d.reward_prior_stddev = -1.0;
    try {
      d.sample_environment(1, 0);
      return 3;
    } catch (const std::invalid_argument &) {
    }
  }
  try {
    TabularMdp wrong(2, 2, std::vector<float>(7), std::vector<double>(4));
    return 4;
  } catch (const std::invalid_argument &) {
  }
  std::printf("tabular mdp sanitize ok %.6f\n", checksum);
  return 0;
}
