// kernels_bandit_agent.hip — the bandit baselines on the meta-bandit lanes (rl_bandit_agent_rollout):
// ResettingMetaAgent<TC> (src/agents/meta.rs:135-199) over SerialActorAgent (src/agents/serial.rs:43-95), TC =
// RandomAgentConfig (src/agents/random.rs:59-73), TabularQLearningAgentConfig (src/agents/tabular.rs:113-133, 159-180,
// 222-232), UCB1AgentConfig (src/agents/bandits/ucb.rs:106-160, 209-234) or BetaThompsonSamplingAgentConfig
// (src/agents/bandits/thompson_sampling.rs:95-136, 186-205) — an actor that is not a network.
//
//   k_meta_agent_rollout<KIND, D>   all T steps of the env's lanes in one launch, one thread per lane: the shape of
//                                   k_stack_rollout (kernels_seq_stack.hip) without a module.  The lane's MetaOps::State
//                                   and its inner agent (k = D - 4 counts and values, the visit count, the actor stream's
//                                   word position) are loaded once, live in registers for the whole horizon and are
//                                   stored once.  Nothing waits on another lane: no barrier, no LDS.
//
// Arithmetic: f64, the reference's operations in the reference's order; the unit is built with -ffp-contract=off and
// writes no fma.  f64 divide and square root are IEEE-correct on the device; UCB1 never evaluates `ln` here — it reads
// 2 ln(visit) from the table the host filled (BanditAgentDev::ln2); THOMPSON evaluates rl_log / rl_exp (rl_detmath.h).
// The per-arm arrays are indexed by the action through selects over the unrolled k arms, never through a
// lane-dependent index: that would put them into scratch memory (cp_reset, env_lanes.hpp, has the same reason).
#include "bandit_agent.hpp"
#include "env_lanes.hpp"
#include "../../include/rl_beta.h"

namespace {

constexpr int BA_BLOCK = 64;  // one wave per workgroup: the lanes spread over as many CUs as there are waves

// TrajSink, and the pull's reward kept for the inner agent's update
struct PullSink {
  TrajSink out;
  float reward;
  __device__ __forceinline__ void record(int action, float r, int succ) {
    reward = r;
    out.record(action, r, succ);
  }
  template <int D>
  __device__ __forceinline__ void successor(const float (&f)[D]) const {
    out.successor(f);
  }
};

// the inner agent of one lane (K arms, one observation: a bandit's singleton)
template <int KIND, int K>
struct InnerAgent {
  uint64_t count[K];
  double value[K];
  uint64_t visit;

  __device__ __forceinline__ void load(const BanditAgentDev &ag, uint32_t i, size_t n) {
    visit = 0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
      count[a] = KIND != RL_BANDIT_AGENT_RANDOM ? ag.count[(size_t)a * n + i] : 0;
      value[a] = KIND != RL_BANDIT_AGENT_RANDOM ? ag.value[(size_t)a * n + i] : 0.0;
    }
    if (KIND == RL_BANDIT_AGENT_UCB1) visit = ag.visit[i];
  }
  __device__ __forceinline__ void store(const BanditAgentDev &ag, uint32_t i, size_t n) const {
    if (KIND != RL_BANDIT_AGENT_RANDOM) {
#pragma unroll
      for (int a = 0; a < K; ++a) {
        ag.count[(size_t)a * n + i] = count[a];
        ag.value[(size_t)a * n + i] = value[a];
      }
    }
    if (KIND == RL_BANDIT_AGENT_UCB1) ag.visit[i] = visit;
  }
  // BuildAgent::build_agent: TabularQLearningAgent::new (tabular.rs:113-133), BaseUCB1Agent::new (ucb.rs:106-135: one
  // success and one failure per arm)
  __device__ __forceinline__ void fresh(const BanditAgentDev &ag) {
#pragma unroll
    for (int a = 0; a < K; ++a) {
      count[a] = KIND == RL_BANDIT_AGENT_UCB1 ? 2 : ag.init_count;
      value[a] = KIND == RL_BANDIT_AGENT_UCB1 ? 0.5 : ag.init_value;
    }
    visit = 2 * K;
  }
  // Actor::act in Training mode; `pos` is the next unread word of the lane's actor stream, `E` the episodes per trial
  __device__ __forceinline__ int act(const BanditAgentDev &ag, const uint32_t *key, uint64_t glane, uint64_t &pos,
                                     uint32_t E) const {
    if (KIND == RL_BANDIT_AGENT_RANDOM)  // IndexSpace::sample (spaces/index.rs:65-67)
      return (int)lane_gen_range(key, glane, pos, K);
    if (KIND == RL_BANDIT_AGENT_TABULAR_Q) {  // tabular.rs:222-232: the draw is taken whatever the rate
      const double u = rl_u64_to_unit_f64(lane_u64_at(key, glane, pos));
      pos += 2;
      if (u < ag.rate) return (int)lane_gen_range(key, glane, pos, K);
      int best = 0;  // the FIRST maximal value (ndarray-stats argmax)
      double best_v = value[0];
#pragma unroll
      for (int a = 1; a < K; ++a)
        if (value[a] > best_v) {
          best = a;
          best_v = value[a];
        }
      return best;
    }
    // ucb.rs:213-234.  The j-th pull of a trial has visit = 2 K + j, j < E while the handle follows its env's trials;
    // the index is held inside the table whatever the caller did to the env between two collections.
    uint64_t j = visit - 2 * K;
    if (j >= E) j = E - 1;
    const double log_squared_visit_count = ag.ln2[j];
    int best = 0;  // the LAST maximal index (utils/iter/cmp.rs:58)
    double best_v = 0.0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
      const double ucb = __builtin_sqrt(log_squared_visit_count / (double)count[a]) * ag.rate + value[a];
      if (a == 0 || ucb >= best_v) {
        best = a;
        best_v = ucb;
      }
    }
    return best;
  }
  // BatchUpdate::batch_update of the one step just taken (SerialActorAgent::update, min_update_size {1, 0})
  __device__ __forceinline__ void update(int action, double reward) {
    if (KIND == RL_BANDIT_AGENT_RANDOM) return;
    uint64_t cnt = 0;
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < K; ++a)
      if (a == action) {
        cnt = count[a];
        v = value[a];
      }
    cnt += 1;
    if (KIND == RL_BANDIT_AGENT_TABULAR_Q) {  // tabular.rs:159-180; a bandit step terminates: no successor value
      const double w = 1.0 / (double)cnt;
      v *= 1.0 - w;
      v += w * reward;
    } else {  // ucb.rs:146-160, reward_shift = -0.0, reward_scale_factor = 1.0 (rewards in [0, 1])
      const double scaled = (reward + (-0.0)) * 1.0;
      visit += 1;
      v += (scaled - v) / (double)cnt;
    }
#pragma unroll
    for (int a = 0; a < K; ++a) {
      count[a] = a == action ? cnt : count[a];
      value[a] = a == action ? v : value[a];
    }
  }
};

// BetaThompsonSamplingAgentConfig { num_samples } (src/agents/bandits/thompson_sampling.rs:95-136, 186-205; DESIGN.md
// §33): per arm a low and a high reward count, both 1 in a fresh agent; act draws, arm by arm, num_samples samples of
// Beta(high, low) (include/rl_beta.h) and takes the LAST maximal sum; update counts the reward on its side of 0.5.
// Here ln and exp ARE evaluated on the device: rl_log / rl_exp of rl_detmath.h, the bits the host computes.
// The draws are many — an OTS pull at four arms takes 80 u64s or more — so the lane keeps the ChaCha8 block it is
// reading: 16 words in registers, computed again only where pos >> 4 changes (pos is even: a block serves 8 draws).
template <int K>
struct InnerAgent<RL_BANDIT_AGENT_THOMPSON, K> {
  uint64_t low[K], high[K];
  uint32_t blk[16];
  uint64_t blk_at;  // the block index `blk` holds; ~0: none yet (word positions stay far below 2^68)

  __device__ __forceinline__ void load(const BanditAgentDev &ag, uint32_t i, size_t n) {
    blk_at = ~0ull;
#pragma unroll
    for (int w = 0; w < 16; ++w) blk[w] = 0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
      low[a] = ag.low[(size_t)a * n + i];
      high[a] = ag.high[(size_t)a * n + i];
    }
  }
  __device__ __forceinline__ void store(const BanditAgentDev &ag, uint32_t i, size_t n) const {
#pragma unroll
    for (int a = 0; a < K; ++a) {
      ag.low[(size_t)a * n + i] = low[a];
      ag.high[(size_t)a * n + i] = high[a];
    }
  }
  // BetaThompsonSamplingAgent::new (thompson_sampling.rs:95-110): one low and one high reward per arm
  __device__ __forceinline__ void fresh(const BanditAgentDev &) {
#pragma unroll
    for (int a = 0; a < K; ++a) low[a] = high[a] = 1;
  }
  // the next u64 of the lane's actor stream, low word first
  __device__ __forceinline__ uint64_t next_u64(const uint32_t *key, uint64_t glane, uint64_t &pos) {
    if ((pos >> 4) != blk_at) {
      blk_at = pos >> 4;
      rl_chacha_block(key, blk_at, glane, 4, blk);
    }
    uint32_t lo32 = 0, hi32 = 0;
#pragma unroll
    for (int k = 0; k < 16; k += 2)
      if (k == (int)(pos & 15)) {
        lo32 = blk[k];
        hi32 = blk[k + 1];
      }
    pos += 2;
    return ((uint64_t)hi32 << 32) | lo32;
  }
  __device__ __forceinline__ int act(const BanditAgentDev &ag, const uint32_t *key, uint64_t glane, uint64_t &pos,
                                     uint32_t) {
    int best = 0;  // the LAST maximal sum (Iterator::max_by, utils/iter/cmp.rs:68-74)
    double best_v = 0.0;
#pragma unroll 1
    for (int arm = 0; arm < K; ++arm) {  // one copy of the sampler's code; the counts come through selects
      uint64_t lo = 0, hi = 0;
#pragma unroll
      for (int a = 0; a < K; ++a)
        if (a == arm) {
          lo = low[a];
          hi = high[a];
        }
      rl_beta beta;
      rl_beta_new((double)hi, (double)lo, &beta);
      double sum = 0.0;
      for (uint32_t j = 0; j < ag.num_samples; ++j) {
        double w = 0.0;
        for (int attempt = 0; attempt < RL_BETA_MAX_ATTEMPTS; ++attempt) {
          const double u1 = rl_u64_to_open01_f64(next_u64(key, glane, pos));
          const double u2 = rl_u64_to_open01_f64(next_u64(key, glane, pos));
          if (rl_beta_attempt(&beta, u1, u2, &w)) break;
        }
        sum += rl_beta_result(&beta, w);
      }
      if (arm == 0 || sum >= best_v) {
        best = arm;
        best_v = sum;
      }
    }
    return best;
  }
  // thompson_sampling.rs:112-136: the reward against the midpoint of the declared interval [0, 1]
  __device__ __forceinline__ void update(int action, double reward) {
    const bool up = reward > 0.5;
#pragma unroll
    for (int a = 0; a < K; ++a) {
      high[a] += (a == action && up) ? 1 : 0;
      low[a] += (a == action && !up) ? 1 : 0;
    }
  }
};

template <int KIND, int D>
__global__ void __launch_bounds__(BA_BLOCK) k_meta_agent_rollout(CartPoleDev c, EnvStateDev st, TrajDev tr,
                                                                BanditAgentDev ag, uint64_t t_global) {
  constexpr int K = D - 4;
  const uint32_t i = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (i >= tr.n) return;  // (no barrier below)
  const size_t n = tr.n, T = tr.T, plane = (T + 1) * n;
  const uint64_t glane = c.lane_offset + i;
  MetaOps::State s;
  MetaOps::load(st, i, s);
  InnerAgent<KIND, K> agent;
  agent.load(ag, i, n);
  uint64_t pos = ag.pos[i];
  float f[D];
  for (size_t t = 0; t < T; ++t) {
    MetaOps::features<D>(c, s, f);
#pragma unroll
    for (int d = 0; d < D; ++d) tr.obs[d * plane + t * n + i] = f[d];
    // ResettingMetaAgent::initial_state (meta.rs:146-157) runs where the meta episode starts: the lane's state is that
    // of a trial's start — no inner episode done, no previous step, all E episodes left
    if (!s.inner_done && !s.prev_some && s.remaining == c.max_steps) agent.fresh(ag);
    // meta.rs:184-197: a finished inner episode -> some_element() = 0, nothing drawn; otherwise the inner actor acts
    const bool pull = !s.inner_done;
    int a = 0;
    if (pull) a = agent.act(ag, c.key_actor, glane, pos, c.max_steps);
    PullSink sink{TrajSink{tr, t * n + i, true}, 0.0f};
    lane_step<MetaOps, D>(c, s, a, glane, t_global + t, sink, f);
    // the update the next observation would trigger (meta.rs:166-182), taken here: the one after a trial's last pull
    // is then part of the state the handle shows, and is never observable by an action
    if (pull) agent.update(a, (double)sink.reward);
  }
  MetaOps::features<D>(c, s, f);
#pragma unroll
  for (int d = 0; d < D; ++d) tr.obs[d * plane + T * n + i] = f[d];
  MetaOps::store(st, i, s);
  agent.store(ag, i, n);
  ag.pos[i] = pos;
}

template <int KIND>
void launch_kind(rl_bandit_agent *agent, rl_env *env, rl_traj *traj) {
  const dim3 grid((traj->d.n + BA_BLOCK - 1) / BA_BLOCK), blk(BA_BLOCK);
#define ROLLOUT(D)                                                                                              \
  hipLaunchKernelGGL((k_meta_agent_rollout<KIND, D>), grid, blk, 0, env->eng->stream, env->dev, env->st, traj->d, \
                     agent->d, env->t_global)
  switch (env->D) {
    case 6: ROLLOUT(6); break;
    case 7: ROLLOUT(7); break;
    case 8: ROLLOUT(8); break;
    case 9: ROLLOUT(9); break;  // 5..12 arms: rl_env_create_meta_bandit_wide
    case 10: ROLLOUT(10); break;
    case 11: ROLLOUT(11); break;
    case 12: ROLLOUT(12); break;
    case 13: ROLLOUT(13); break;
    case 14: ROLLOUT(14); break;
    case 15: ROLLOUT(15); break;
    case 16: ROLLOUT(16); break;
    default: throw RlError(RL_ERR_UNSUPPORTED, "rl_bandit_agent_rollout: built for 2..12 arms (6..16 features)");
  }
#undef ROLLOUT
}

}  // namespace

void launch_bandit_agent_rollout(rl_bandit_agent *agent, rl_env *env, rl_traj *traj) {
  ProfScope ps(env->eng, RL_K_ROLLOUT);
  switch (agent->cfg.kind) {
    case RL_BANDIT_AGENT_RANDOM: launch_kind<RL_BANDIT_AGENT_RANDOM>(agent, env, traj); break;
    case RL_BANDIT_AGENT_TABULAR_Q: launch_kind<RL_BANDIT_AGENT_TABULAR_Q>(agent, env, traj); break;
    case RL_BANDIT_AGENT_THOMPSON: launch_kind<RL_BANDIT_AGENT_THOMPSON>(agent, env, traj); break;
    default: launch_kind<RL_BANDIT_AGENT_UCB1>(agent, env, traj); break;
  }
  RL_HIP_CHECK(hipGetLastError());
  env->t_global += traj->d.T;
}
