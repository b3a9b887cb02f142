// bandit_agent.hpp — the bandit baselines on the meta-bandit lanes (rl_bandit_agent, include/relearn_hip.h; DESIGN.md
// §32): the handle, what the kernel gets of it by value, and the launcher kernels_bandit_agent.hip defines.
#pragma once
#include <cstdint>

#include "engine.hpp"

// UCB1: the table holds 2 ln(visit) for every pull of a trial, one f64 each (8 MiB at the bound)
constexpr uint64_t RL_BANDIT_LN_TABLE_MAX = 1ull << 20;
// THOMPSON: a pull draws k * num_samples Beta samples in the one launch; the bound keeps that launch's length in hand
constexpr uint64_t RL_BANDIT_NUM_SAMPLES_MAX = 1024;

// The inner agents' state, one per lane, lane-minor.  Views into rl_bandit_agent::mem.
struct BanditAgentDev {
  uint64_t *pos;      // [n] next unread word of the lane's actor stream (always even: u64 draws only)
  uint64_t *count;    // [k][n] TABULAR_Q: state_action_counts; UCB1: state_action_count (NULL: RANDOM)
  double *value;      // [k][n] TABULAR_Q: state_action_values; UCB1: state_action_mean_reward (NULL: RANDOM)
  uint64_t *visit;    // [n] UCB1: state_visit_count (NULL otherwise)
  const double *ln2;  // [E] UCB1: 2.0 * log((double)(2 k + j)), filled by the host at creation (NULL otherwise)
  double rate;        // exploration_rate
  double init_value;  // TABULAR_Q: initial_action_value
  uint64_t init_count;  // TABULAR_Q: initial_action_count
  uint64_t *low;      // [k][n] THOMPSON: low_reward_count (NULL otherwise)
  uint64_t *high;     // [k][n] THOMPSON: high_reward_count (NULL otherwise)
  uint32_t num_samples;  // THOMPSON: samples summed per arm and pull
};

struct rl_bandit_agent {
  rl_engine *eng;
  DevMem mem;
  rl_bandit_agent_config cfg;
  uint64_t n = 0;      // lanes, arms and episodes per trial of the env the agent was made on
  uint32_t k = 0;
  uint64_t E = 0;
  BanditAgentDev d{};
};

// T steps of every lane of `env` in one launch (advances env->t_global)
void launch_bandit_agent_rollout(rl_bandit_agent *agent, rl_env *env, rl_traj *traj);
