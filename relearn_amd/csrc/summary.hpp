// summary.hpp — the step summaries (rl_summary, include/relearn_hip.h): Chan's merge shared by the device kernels and
// the host entry point, the handle, and the launchers kernels_summary.hip defines.
#pragma once
#include <cstdint>

#include "../../include/relearn_hip.h"
#include "dev_mem.hpp"

#if defined(__HIPCC__) || defined(__HIP__)
#define RL_SUM_HD __host__ __device__ inline
#else
#define RL_SUM_HD inline
#endif

// `impl Add for OnlineMeanVariance` (src/utils/stats.rs:184-209) in the reference's order of operations, except that an
// empty side returns the other side unchanged (the reference divides 0 / 0 when both are empty)
RL_SUM_HD rl_mean_variance mv_merge(const rl_mean_variance &a, const rl_mean_variance &b) {
  if (b.count == 0) return a;
  if (a.count == 0) return b;
  const double na = (double)a.count, nb = (double)b.count;
  const uint64_t count = a.count + b.count;
  const double n = (double)count;
  rl_mean_variance r;
  r.mean = (a.mean * na + b.mean * nb) / n;
  const double delta = a.mean - b.mean;
  r.squared_residual_sum = a.squared_residual_sum + b.squared_residual_sum + delta * delta * na * nb / n;
  r.count = count;
  return r;
}

RL_SUM_HD rl_steps_summary ss_merge(const rl_steps_summary &a, const rl_steps_summary &b) {
  rl_steps_summary r;
  r.step_reward = mv_merge(a.step_reward, b.step_reward);
  r.episode_reward = mv_merge(a.episode_reward, b.episode_reward);
  r.episode_length = mv_merge(a.episode_length, b.episode_length);
  return r;
}

struct ReplayRec;

struct rl_summary {
  rl_engine *eng;
  DevMem mem;
  uint64_t n = 0;
  uint64_t *carry_len = nullptr;  // [n] length of the episode in progress
  double *carry_ret = nullptr;    // [n] its return
  rl_steps_summary *acc = nullptr;   // the completed StepsSummary since the last clear
  rl_steps_summary *part = nullptr;  // [max_groups] one record per workgroup of the last push
  uint64_t max_groups = 0;
};

// reward[t][lane] f32 and flag[t][lane] u8 planes, n lanes x T steps
void launch_summary_planes(rl_summary *s, const float *reward, const uint8_t *flag, uint32_t T);
// flag[t][lane] of a DQN collection of T steps; rewards from the replay records `rec` [n][C] at ring slot
// (total[lane] - T + t) mod C
void launch_summary_replay(rl_summary *s, const ReplayRec *rec, const uint32_t *total, uint32_t C,
                           const uint8_t *flag, uint32_t T);
