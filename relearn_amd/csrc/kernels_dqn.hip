// kernels_dqn.hip — DQN data path: epsilon-greedy collection straight into the HBM replay ring, and the minibatch
// builder (gather of the sampled episodes + value targets).
//
// Reference: DqnActor::act (src/torch/agents/dqn.rs:360-379), ReplayBuffer::write_step (src/agents/buffers/
// replay.rs:89-115), DqnAgent::batch_update_slice_refs sample_minibatch (dqn.rs:280-314), StepValueTarget
// (src/torch/agents/critics/mod.rs:203-229).
#include <memory>
#include <type_traits>

#include "bf16_tile.hpp"
#include "device_fns.hpp"
#include "dqn_lanes.hpp"
#include "env_lanes.hpp"
#include "kernels.hpp"
#include "policy_terms.hpp"
#include "replay.hpp"

// T env-actor steps per lane with the DQN actor (dqn_explores / dqn_random_action, else the greedy action); every step is
// appended to the lane's replay ring.
// The actor's generator (LaneActorRng, env_lanes.hpp) keeps its word position in HBM between launches.
// G threads per lane (G consecutive lanes of a wave) share the greedy branch's Q-network forward, as in the fused TRPO
// rollout (kernels_rollout.hip: a launch lasts T x the latency of one step, and most of a greedy step is the 128-unit
// forward); everything else — draws, physics, ring bookkeeping — is repeated by every thread of the group, thread 0
// stores.  The result does not depend on G (mlp_forward_group_lds).
// `Env`: CartPoleOps, or IndexOps (Chain, MemoryGame, the bandit: env_lanes.hpp).  An index lane reads word t_global + t of
// its env stream in step t (Chain's slip draw) and draws MemoryGame's initial states sequentially from ChainLane::env_pos:
// every thread of a lane's group repeats both, like the physics.
template <class Env, int D, int BLOCK, int G>
__global__ void __launch_bounds__(BLOCK) k_rollout_dqn(CartPoleDev c, EnvStateDev st, ReplayDev rp,
                                                       const float *__restrict__ qnet, int H, uint32_t T, uint64_t p_int,
                                                       int always_explore, uint8_t *__restrict__ flags_out,
                                                       uint32_t *__restrict__ range, uint64_t t_global) {
  __shared__ uint32_t words[16 * BLOCK];
  __shared__ __attribute__((aligned(16))) float pk[MLP_PK_FLOATS];  // the Q-network, one 8-float record per hidden unit
  // the collected observations' magnitude range, for the fused gradient kernel's range guard (bf16_tile.hpp): one fold
  // per wave and launch into words that are never reset — the range of everything ever collected bounds every minibatch
  // drawn from the store
  uint32_t r_lo = 0x7F7FFFFFu, r_hi = 0u;
  const uint32_t n = rp.N;
  mlp_pack_lds<D>(pk, qnet, H, threadIdx.x, BLOCK);
  __syncthreads();
  const uint32_t i0 = (blockIdx.x * BLOCK + threadIdx.x) / G;
  const int g = threadIdx.x % G;
  // lanes past the end follow lane n - 1 without storing: the group shuffles need every thread of a group
  const bool live = i0 < n;
  const uint32_t i = live ? i0 : n - 1;
  const bool writer = live && g == 0;
  const uint64_t lane = c.lane_offset + i;
  typename Env::State s;
  Env::load(st, i, s);
  LaneRing ring = ring_load(rp, i);
  LaneEpEnds eps{rp.ep_end, n, i, writer};
  LaneActorRng<BLOCK> rng{&words[threadIdx.x], c.key_actor, lane, rp.actor_pos[i], ~0ull};
  bool full = false;
  for (uint32_t t = 0; t < T; ++t) {
    float f[D];
    Env::template features<D>(c, s, f);
    int a;
    if (dqn_explores(rng, p_int, always_explore)) {
      a = dqn_random_action<2>(rng);
    } else {
      float z[2];
      mlp_forward_group_lds<D, G>(pk, H, g, f, z);
      a = z[1] > z[0] ? 1 : 0;  // argmax: first maximal index
    }
    // lane_step's rule (env_lanes.hpp) with the replay ring as its sink, written out: the ring may refuse the step, and
    // closes a lane the horizon cuts in its own way (DESIGN.md §25 on why these lines are not a sink struct)
    float reward;
    const int succ = Env::step(c, s, a, lane, t_global + t, reward);
    // the engine's horizon rule: a lane still mid-episode at the end of the launch closes its
    // episode as Interrupt(successor observation) and carries the env state on into the next collection
    const bool horizon_cut = succ == RL_SUCC_CONTINUE && t + 1 == T;
    const int succ_rec = horizon_cut ? RL_SUCC_INTERRUPT : succ;
    const uint32_t slot_abs = ring_write_step(ring, rp.C, rp.E, eps, succ_rec != RL_SUCC_CONTINUE);
    if (slot_abs == 0xffffffffu) {
      full = true;  // WriteExperienceError::Full: a single episode longer than the lane's capacity
      break;
    }
    const size_t o = (size_t)i * rp.C + slot_abs % rp.C;
#pragma unroll
    for (int d = 0; d < D; ++d) bt::range_accumulate(f[d], r_lo, r_hi);
    if (writer) {
      ReplayRec rec;
#pragma unroll
      for (int d = 0; d < 5; ++d) rec.x[d] = d < D ? f[d < D ? d : 0] : 0.0f;
      rec.reward = reward;
      rec.af = (uint32_t)a | (uint32_t)succ_rec << 8;
      rec_store(rp.rec + o, rec);
    }
    if (succ_rec == RL_SUCC_INTERRUPT) {
      Env::template features<D>(c, s, f);
#pragma unroll
      for (int d = 0; d < D; ++d) bt::range_accumulate(f[d], r_lo, r_hi);
      if (writer) {
#pragma unroll
        for (int d = 0; d < D; ++d) rp.next[o].x[d] = f[d];
      }
    }
    if (writer) flags_out[(size_t)t * n + i] = (uint8_t)succ_rec;
    if (succ != RL_SUCC_CONTINUE) Env::reset(c, s, lane);
  }
  if (range != nullptr) bt::range_fold_wave(range, blockIdx.x, r_lo, r_hi);  // (every thread of the wave is here)
  if (!writer) return;
  if (full) *rp.error = 1;
  ring_store(rp, i, ring);
  rp.actor_pos[i] = rng.pos;
  Env::store(st, i, s);
}

// ---------------------------------------------------------------- collection with an action-value module of any shape
// DqnConfig<MB> is generic over the module (src/torch/agents/dqn.rs:26-39).  A module the fused collection kernel is not
// built for (rl_mlp::general: several hidden layers, other activations, a wider layer) collects one launch sequence per
// step — observe, the module's layer kernels over all lanes (kernels_general.hip), then this kernel: DqnActor::act
// from the lane's actor stream with the greedy branch reading the module's outputs, the env step, the ring write — with
// the fused kernel's stream discipline, ring bookkeeping and horizon rule (above), one thread per lane.  `word`: the
// global step (t_global + t).  Features 5..7 of an observation wider than the 32-byte record go to the second record array
// (ReplayDev::hi).
template <class Env, int D, int BLOCK, int A>
__global__ void __launch_bounds__(BLOCK) k_dqn_lane_step(CartPoleDev c, EnvStateDev st, ReplayDev rp,
                                                         const float *__restrict__ q_values /* [A][n] */, uint64_t p_int,
                                                         int always_explore, int last_step,
                                                         uint8_t *__restrict__ flags_row, uint64_t word) {
  __shared__ uint32_t words[16 * BLOCK];
  const uint32_t n = rp.N;
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint64_t lane = c.lane_offset + i;
  typename Env::State s;
  Env::load(st, i, s);
  LaneRing ring = ring_load(rp, i);
  LaneEpEnds eps{rp.ep_end, n, i, true};
  LaneActorRng<BLOCK> rng{&words[threadIdx.x], c.key_actor, lane, rp.actor_pos[i], ~0ull};
  float f[D];
  Env::template features<D>(c, s, f);
  int a;
  if (dqn_explores(rng, p_int, always_explore)) {
    a = dqn_random_action<A>(rng);
  } else {
    float z[A];
#pragma unroll
    for (int q = 0; q < A; ++q) z[q] = q_values[(size_t)q * n + i];
    a = first_max_index<A>(z);  // argmax: first maximal index
  }
  float reward;  // (the step, its record and the horizon rule as in the fused kernel)
  const int succ = Env::step(c, s, a, lane, word, reward);
  const bool horizon_cut = succ == RL_SUCC_CONTINUE && last_step != 0;
  const int succ_rec = horizon_cut ? RL_SUCC_INTERRUPT : succ;
  const uint32_t slot_abs = ring_write_step(ring, rp.C, rp.E, eps, succ_rec != RL_SUCC_CONTINUE);
  if (slot_abs == 0xffffffffu) {  // WriteExperienceError::Full (the lane stops here; the host raises the error)
    *rp.error = 1;
    return;
  }
  const size_t o = (size_t)i * rp.C + slot_abs % rp.C;
  ReplayRec rec;
#pragma unroll
  for (int d = 0; d < 5; ++d) rec.x[d] = d < D ? f[d < D ? d : 0] : 0.0f;
  rec.reward = reward;
  rec.af = (uint32_t)a | (uint32_t)succ_rec << 8;
  rec_store(rp.rec + o, rec);
  if constexpr (D > 5) rp.hi[o] = make_float4(f[5], D > 6 ? f[D > 6 ? 6 : 0] : 0.0f, D > 7 ? f[D > 7 ? 7 : 0] : 0.0f, 0.0f);
  if (succ_rec == RL_SUCC_INTERRUPT) {
    Env::template features<D>(c, s, f);
#pragma unroll
    for (int d = 0; d < D; ++d) rp.next[o].x[d] = f[d];
  }
  flags_row[i] = (uint8_t)succ_rec;
  if (succ != RL_SUCC_CONTINUE) Env::reset(c, s, lane);
  ring_store(rp, i, ring);
  rp.actor_pos[i] = rng.pos;
  Env::store(st, i, s);
}

// one-step TD targets from the module's outputs at the successor observations (the gather left rewards where the
// targets go and the successor codes in `flag`): r + gamma * max_a Q(s'), 0 beyond a Terminate — the arithmetic of
// k_dqn_build_minibatch (amax, `scalar * tensor`, then `tensor + tensor`)
template <int A>
__global__ void k_dqn_td_targets(float *__restrict__ tgt, const uint8_t *__restrict__ flag,
                                 const float *__restrict__ q_next /* [A][n] */, uint32_t n, float gamma) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float vnext = 0.0f;
  if (flag[i] != RL_SUCC_TERMINATE) {
    float z[A];
#pragma unroll
    for (int q = 0; q < A; ++q) z[q] = q_next[(size_t)q * n + i];
    first_max_index<A>(z, vnext);
  }
  const float dn = gamma * vnext;
  tgt[i] = tgt[i] + dn;
}

// ---------------------------------------------------------------- the gather, for every minibatch builder
// one stored step: its observation (the record's features, 5..7 from the second record array when D > 5), action,
// successor code and reward
template <int D>
struct StoredStep {
  float x[D];
  uint32_t action, succ;
  float reward;
};
template <int D>
__device__ __forceinline__ StoredStep<D> step_load(const ReplayDev &rp, uint32_t lane, uint32_t slot) {
  const size_t o = (size_t)lane * rp.C + slot;
  const ReplayRec rec = rec_load(rp.rec + o);
  StoredStep<D> s;
#pragma unroll
  for (int d = 0; d < (D < 5 ? D : 5); ++d) s.x[d] = rec.x[d];
  if constexpr (D > 5) rec_load_hi<D>(rp, o, s.x);
  s.action = rec.af & 0xffu;
  s.succ = rec.af >> 8;
  s.reward = rec.reward;
  return s;
}
// the successor observation stored with the step in `slot` (meaningful after an Interrupt and at an episode's last step)
template <int D>
__device__ __forceinline__ void next_load(const ReplayDev &rp, uint32_t lane, uint32_t slot, float (&x)[D]) {
  const ReplayNext *__restrict__ nx = rp.next + (size_t)lane * rp.C + slot;
#pragma unroll
  for (int d = 0; d < D; ++d) x[d] = nx->x[d];
}
// the successor observation of step i (successor code `succ`) of the episode of `len` steps from ring step `start`: the
// stored one after an Interrupt or at the episode's last step, else the observation of the following step
template <int D>
__device__ __forceinline__ void successor_load(const ReplayDev &rp, uint32_t lane, uint32_t start, uint32_t len,
                                               uint32_t i, uint32_t succ, float (&x)[D]) {
  if (succ == RL_SUCC_INTERRUPT || i + 1 == len) {
    next_load<D>(rp, lane, (start + i) % rp.C, x);
  } else {
    const StoredStep<D> s1 = step_load<D>(rp, lane, (start + i + 1) % rp.C);
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = s1.x[d];
  }
}

// One minibatch, one workgroup per sampled episode: the episode's steps into the compact sample arrays (obs plane stride
// `out_plane`) and the value targets:
//   RewardToGo: G_t = r_t + gamma * G_{t+1} (f32 multiply, then add — packed.rs:312-342 arithmetic)
//   OneStepTd : r_t + gamma * max_a Q(s_{t+1}) from the fused module's forward; 0 beyond a Terminate
// (k_dqn_build_all with one minibatch computes the same reward-to-go targets; at config 3's shape, 4,337 episodes of 23
// steps on average, it takes 13 us against this kernel's 10 — profiles/dqn_one_path_parent_vs_this.jsonl — so the
// one-at-a-time builder keeps this scan.)
template <int D>
__global__ void __launch_bounds__(64) k_dqn_build_minibatch(ReplayDev rp, EpisodeLists ep, float *__restrict__ out_obs,
                                                            size_t out_plane, uint8_t *__restrict__ out_action,
                                                            float *__restrict__ out_target, float gamma,
                                                            int one_step_td, const float *__restrict__ qnet, int H) {
  __shared__ float rew[1024];
  __shared__ float carry;
  const uint32_t e = blockIdx.x;
  const uint32_t lane = ep.lane[e], start = ep.start[e], len = ep.len[e], off = ep.off[e];
  for (uint32_t i = threadIdx.x; i < len; i += 64) {
    const StoredStep<D> s = step_load<D>(rp, lane, (start + i) % rp.C);
#pragma unroll
    for (int d = 0; d < D; ++d) out_obs[d * out_plane + off + i] = s.x[d];
    out_action[off + i] = (uint8_t)s.action;
    if constexpr (D <= 5)  // (the forward below is the fused module's: a wider module's TD targets are k_dqn_td_targets')
    if (one_step_td) {
      float vnext = 0.0f;
      if (s.succ != RL_SUCC_TERMINATE) {
        float x[D], z[2];
        successor_load<D>(rp, lane, start, len, i, s.succ, x);
        mlp_forward_lane<D, 2>(qnet, H, x, z);
        vnext = z[1] > z[0] ? z[1] : z[0];  // amax(-1)
      }
      const float dn = gamma * vnext;
      out_target[off + i] = s.reward + dn;
    }
  }
  if (one_step_td) return;
  // reward-to-go: backwards in chunks of 1024 steps staged through LDS, scanned by one lane
  const ReplayRec *__restrict__ ring = rp.rec + (size_t)lane * rp.C;
  if (threadIdx.x == 0) carry = 0.0f;
  __syncthreads();
  for (uint32_t hi = len; hi > 0;) {
    const uint32_t lo = hi > 1024 ? hi - 1024 : 0, cnt = hi - lo;
    for (uint32_t i = threadIdx.x; i < cnt; i += 64) rew[i] = ring[(start + lo + i) % rp.C].reward;
    __syncthreads();
    if (threadIdx.x == 0) {
      float g = carry;
      bool first = hi == len;
      for (uint32_t i = cnt; i-- > 0;) {
        if (first) {
          g = rew[i];
          first = false;
        } else {
          float p = g * gamma;
          g = rew[i] + p;
        }
        rew[i] = g;
      }
      carry = g;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt; i += 64) out_target[off + lo + i] = rew[i];
    __syncthreads();
    hi = lo;
  }
}

// The minibatches of an update in ONE launch (reward-to-go targets do not depend on the network, so nothing in an update
// has to wait for them), or one of them (a recurrent agent's, and the gather behind which another module's one-step TD
// targets are formed): one wave per sampled episode, blockIdx.y = minibatch.  RewardToGo: G_t = r_t + gamma * G_{t+1} (f32 multiply, then add — packed.rs:312-342 arithmetic); the scan
// runs on broadcast values of one 64-step chunk at a time, last chunk first.  Minibatch b reads its lists at b * max_eps
// and lands at obs + b * obs_stride (plane stride 2 * its step count: the T = 1 trajectory layout the gradient kernels
// read), action / target + b * step_stride.
constexpr int BUILD_ALL_WAVES = 4;
template <int D>
__global__ void __launch_bounds__(BUILD_ALL_WAVES * 64)
    k_dqn_build_all(ReplayDev rp, EpisodeLists ep, uint32_t max_eps, const DqnCountsDev *__restrict__ counts,
                    float *__restrict__ out_obs, size_t obs_stride, uint8_t *__restrict__ out_action,
                    float *__restrict__ out_target, size_t step_stride, float gamma, uint8_t *__restrict__ out_flag) {
  // out_flag != NULL: one-step TD — the targets are formed later (they use the current network): the reward goes where
  // the target would, the successor code into out_flag, the successor observation into time slot 1 of the observation
  // planes
  const bool td = out_flag != nullptr;
  const uint32_t b = blockIdx.y, lane = threadIdx.x & 63;
  const uint32_t e = blockIdx.x * BUILD_ALL_WAVES + (threadIdx.x >> 6);
  const uint32_t n_eps = counts[b].n_eps, n_steps = counts[b].n_steps;
  if (e >= n_eps) return;
  const size_t eo = (size_t)b * max_eps + e;
  const uint32_t ln = ep.lane[eo], start = ep.start[eo], len = ep.len[eo], off = ep.off[eo];
  const size_t out_plane = (size_t)2 * n_steps;
  float *__restrict__ obs_b = out_obs + (size_t)b * obs_stride;
  uint8_t *__restrict__ act_b = out_action + (size_t)b * step_stride;
  float *__restrict__ tgt_b = out_target + (size_t)b * step_stride;
  float g = 0.0f;
  bool first = true;
  for (uint32_t hi = len; hi > 0;) {
    const uint32_t lo = hi > 64 ? hi - 64 : 0, cnt = hi - lo;
    const bool mine = lane < cnt;
    const uint32_t i = lo + (mine ? lane : 0);
    const StoredStep<D> s = step_load<D>(rp, ln, (start + i) % rp.C);
    float out = 0.0f;
    for (uint32_t k = cnt; k-- > 0;) {  // (uniform trip count; every lane carries the same g)
      const float r = __shfl(s.reward, (int)k, 64);
      if (first) {
        g = r;
        first = false;
      } else {
        const float p = g * gamma;
        g = r + p;
      }
      if (lane == k) out = g;
    }
    if (mine) {
#pragma unroll
      for (int d = 0; d < D; ++d) obs_b[d * out_plane + off + i] = s.x[d];
      act_b[off + i] = (uint8_t)s.action;
      tgt_b[off + i] = td ? s.reward : out;
      if (td) {
        out_flag[(size_t)b * step_stride + off + i] = (uint8_t)s.succ;
        float nx[D];
        successor_load<D>(rp, ln, start, len, i, s.succ, nx);
#pragma unroll
        for (int d = 0; d < D; ++d) obs_b[d * out_plane + n_steps + off + i] = nx[d];
      }
    }
    hi = lo;
  }
}

// ---------------------------------------------------------------- minibatch episode sampling
// sample_minibatch of DqnAgent::batch_update_slice_refs (dqn.rs:280-291):
//   iter::repeat(buffers).flatten().map(|buf| buf.episodes().get(Uniform::new(0, buf.num_episodes()).sample(rng)))
//       .take_while(|ep| { let take = total < minibatch_steps; total += ep.len(); take })
// The draws are sequential in the agent's Prng, but draw j is `next_u64` number j of the stream unless an earlier
// draw was rejected by UniformInt's widening-multiply test (probability < num_episodes / 2^64).  So candidate j is
// evaluated by thread j of a 1024-wide chunk from stream words [pos + 2j, pos + 2j + 2), episode lengths are
// prefix-summed, and the take_while cut is the first candidate whose running total reaches minibatch_steps.  If any
// candidate of a chunk is rejected, one thread replays that chunk onwards with the plain sequential algorithm.
// take_while evaluates (and consumes the draw of) the first episode it refuses: pos advances past it.
struct EpisodePick {
  uint32_t start, len;
  bool rejected, empty;
};

__device__ inline uint64_t agent_u64(const AgentKey &key, uint64_t word_pos) {
  uint32_t w[16];
  rl_chacha_block(key.w, word_pos >> 4, 0, 4, w);
  const uint32_t i = (uint32_t)(word_pos & 15);
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (k == (int)i) lo = w[k];
    if (k == (int)i + 1) hi = w[k];
  }
  if (i == 15) {  // the pair straddles two blocks
    rl_chacha_block(key.w, (word_pos >> 4) + 1, 0, 4, w);
    hi = w[0];
  }
  return ((uint64_t)hi << 32) | lo;
}

// Uniform::new(0usize, n).sample(rng) for the draw `v`, then Episodes::get (replay.rs:154-165)
// the fields of a lane's ring the pick needs (constant during an update: a workgroup may cache them)
struct LaneMeta {
  uint32_t n_eps, eh, head;  // stored episodes; ring index of the oldest (reduced mod E); first stored step
};
__device__ inline LaneMeta lane_meta(const ReplayDev &rp, uint32_t lane) {
  return LaneMeta{rp.ep_count[lane], rp.ep_head[lane] % rp.E, rp.head[lane]};  // ep_head counts up without wrapping
}

__device__ inline EpisodePick pick_episode(const ReplayDev &rp, uint32_t lane, const LaneMeta &lm, uint64_t v) {
  EpisodePick p{0, 0, false, false};
  const uint64_t n = lm.n_eps;
  if (n == 0) {
    p.empty = true;  // Uniform::new(0, 0) panics in the reference
    return p;
  }
  const uint64_t lo = v * n, hi = __umul64hi(v, n);
  if (lo > ~0ull - n) {  // ints_to_reject < n: only then can the draw fall outside the zone (the 64-bit division
                         // stays off the common path)
    const uint64_t ints_to_reject = (0ull - n) % n;  // (u64::MAX - range + 1) % range
    const uint64_t zone = ~0ull - ints_to_reject;
    if (lo > zone) {
      p.rejected = true;
      return p;
    }
  }
  const uint32_t idx = (uint32_t)hi, eh = lm.eh;
  // ring index (eh + idx) mod E: eh < E and idx < n <= E, one conditional subtraction
  const uint32_t r1 = eh + idx, r0 = r1 - 1;
  const uint32_t s1 = r1 >= rp.E ? r1 - rp.E : r1, s0 = (idx != 0 && r0 >= rp.E) ? r0 - rp.E : r0;
  const uint32_t head = lm.head;
  const uint32_t end = rp.ep_end[(size_t)s1 * rp.N + lane];
  const uint32_t prev = rp.ep_end[(size_t)(idx != 0 ? s0 : s1) * rp.N + lane];  // unconditional: both loads in flight
  const uint32_t start = idx == 0 ? head : prev;
  p.start = start;
  p.len = end - start;
  if (p.len == 0 || p.len > rp.C) p.empty = true;  // corrupt bookkeeping: never loop on it
  return p;
}

constexpr int SAMPLE_BLOCK = 1024;
constexpr int SAMPLE_CPT = 5;                            // candidates per thread and pass (consecutive)
constexpr int SAMPLE_CHUNK = SAMPLE_BLOCK * SAMPLE_CPT;  // 5,120: a 100 k-step minibatch of CartPole episodes is one pass
constexpr int SAMPLE_BLOCKS = SAMPLE_CHUNK / 8 + 1;      // ChaCha blocks a pass can touch (8 draws of 2 words per block)

// inclusive prefix sum of one value per thread over the workgroup (wave shuffles, then the 16 wave totals)
__device__ inline uint32_t block_inclusive_scan(uint32_t v, uint32_t *wave_tot, uint32_t tid) {
  const uint32_t lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)v, d, 64);
    if (lane >= (uint32_t)d) v += up;
  }
  if (lane == 63) wave_tot[wave] = v;
  __syncthreads();
  uint32_t base = 0;
#pragma unroll
  for (int w = 0; w < SAMPLE_BLOCK / 64; ++w) base += w < (int)wave ? wave_tot[w] : 0u;
  __syncthreads();  // wave_tot is reused by the next scan
  return base + v;
}

constexpr int SAMPLE_META_LANES = 4096;  // up to this many lanes the ring fields are cached in LDS (48 KB)

template <bool META_LDS>
__global__ void __launch_bounds__(SAMPLE_BLOCK) k_dqn_sample(ReplayDev rp, AgentKey key, uint64_t *agent_pos,
                                                             uint32_t minibatch_steps, uint32_t max_eps,
                                                             uint32_t *__restrict__ ep_lane,
                                                             uint32_t *__restrict__ ep_start,
                                                             uint32_t *__restrict__ ep_len,
                                                             uint32_t *__restrict__ ep_off, DqnCountsDev *counts,
                                                             int sequential, uint32_t n_batches) {
  __shared__ uint32_t words[SAMPLE_BLOCKS * 16];  // the pass's stretch of the agent's stream, one ChaCha block per thread
  __shared__ uint32_t wave_tot[SAMPLE_BLOCK / 64];
  __shared__ int s_flag[2];  // [0] rejected draw in this pass, [1] empty buffer
  __shared__ uint32_t s_last[2];  // episodes and steps the pass takes
  __shared__ uint64_t s_pos;      // stream position after a sequential replay (known to thread 0 only)
  __shared__ uint32_t meta[META_LDS ? 3 * SAMPLE_META_LANES : 3];
  const uint32_t tid = threadIdx.x;
  if (META_LDS)
    for (uint32_t l = tid; l < rp.N; l += SAMPLE_BLOCK) {
      const LaneMeta lm = lane_meta(rp, l);
      meta[3 * l] = lm.n_eps;
      meta[3 * l + 1] = lm.eh;
      meta[3 * l + 2] = lm.head;
    }
  auto meta_of = [&](uint32_t l) {
    return META_LDS ? LaneMeta{meta[3 * l], meta[3 * l + 1], meta[3 * l + 2]} : lane_meta(rp, l);
  };
  const int rp_error = *rp.error != 0 ? 1 : 0;
  uint64_t pos_now = *agent_pos;  // carried in registers from minibatch to minibatch
  // `n_batches` consecutive minibatches in one launch (the draws of minibatch b + 1 continue where b stopped);
  // minibatch b writes its lists at offset b * max_eps and its counts at counts[b]
  for (uint32_t batch = 0; batch < n_batches; ++batch, ep_lane += max_eps, ep_start += max_eps, ep_len += max_eps,
                ep_off += max_eps, ++counts) {
  __syncthreads();  // (first minibatch: the cached ring fields are in place)
  const uint64_t pos0 = pos_now;
  uint32_t total = 0;   // steps taken so far
  uint32_t n_eps = 0;   // episodes taken so far
  uint64_t draws = 0;   // u64 draws consumed so far
  bool done = false, fallback = sequential != 0;
  int err = 0;
  while (!done && !fallback) {
    if (tid < 2) s_flag[tid] = 0;
    // the stream words of candidates [draws, draws + CHUNK): word positions [first, first + 2 CHUNK)
    const uint64_t first = pos0 + 2 * draws, block0 = first >> 4;
    const uint32_t skew = (uint32_t)(first & 15);
    const uint32_t lane0 = (uint32_t)(draws % rp.N);
    if (tid < (uint32_t)SAMPLE_BLOCKS) {
      uint32_t w[16];
      rl_chacha_block(key.w, block0 + tid, 0, 4, w);
#pragma unroll
      for (int k = 0; k < 16; ++k) words[tid * 16 + k] = w[k];
    }
    __syncthreads();
    EpisodePick p[SAMPLE_CPT];
    uint32_t lanes[SAMPLE_CPT], mine = 0;
    bool rej = false, empty = false;
#pragma unroll
    for (int c = 0; c < SAMPLE_CPT; ++c) {
      const uint32_t jl = tid * SAMPLE_CPT + c;
      lanes[c] = (lane0 + jl) % rp.N;  // = (draws + jl) mod N without a 64-bit division per candidate
      const uint32_t wi = skew + 2 * jl;
      p[c] = pick_episode(rp, lanes[c], meta_of(lanes[c]), ((uint64_t)words[wi + 1] << 32) | words[wi]);
      rej |= p[c].rejected;
      empty |= p[c].empty;
      mine += p[c].len;
    }
    if (rej) s_flag[0] = 1;
    if (empty) s_flag[1] = 1;
    const uint32_t incl = block_inclusive_scan(mine, wave_tot, tid);  // (its barriers publish s_flag)
    if (s_flag[1]) {
      err = 2;
      break;
    }
    if (s_flag[0]) {
      fallback = true;
      break;
    }
    uint32_t before = total + incl - mine, took = 0;
#pragma unroll
    for (int c = 0; c < SAMPLE_CPT; ++c) {
      const bool take = before < minibatch_steps;
      const uint32_t slot = n_eps + tid * SAMPLE_CPT + c;
      if (take && slot < max_eps) {
        ep_lane[slot] = lanes[c];
        ep_start[slot] = p[c].start;
        ep_len[slot] = p[c].len;
        ep_off[slot] = before;
      }
      took += take ? 1u : 0u;
      before += take ? p[c].len : 0u;
    }
    // lengths are >= 1, so the taken candidates are a prefix of the pass (candidate 0 always belongs to it: the loop
    // would have ended otherwise); the thread that holds the prefix's last candidate publishes its size and steps
    const bool next_takes = tid + 1 < (uint32_t)SAMPLE_BLOCK && total + incl < minibatch_steps;
    if (took > 0 && !(took == (uint32_t)SAMPLE_CPT && next_takes)) {
      s_last[0] = tid * SAMPLE_CPT + took;
      s_last[1] = before - total;
    }
    __syncthreads();
    const uint32_t taken = s_last[0];
    total += s_last[1];
    n_eps += taken;
    if (taken < (uint32_t)SAMPLE_CHUNK) {
      draws += taken + 1;  // plus the refused candidate
      done = true;
    } else {
      draws += SAMPLE_CHUNK;
    }
    __syncthreads();
  }
  if (fallback && tid == 0) {
    // plain sequential restatement from candidate `draws` on (pos counts words: 2 per draw, more after rejections)
    uint64_t pos = pos0 + 2 * draws;
    uint64_t cand = draws;
    for (;;) {
      const uint32_t lane = (uint32_t)(cand % rp.N);
      EpisodePick p;
      for (;;) {
        p = pick_episode(rp, lane, meta_of(lane), agent_u64(key, pos));
        pos += 2;
        if (!p.rejected) break;
      }
      if (p.empty) {
        err = 2;
        break;
      }
      const bool take = total < minibatch_steps;
      if (!take) break;
      if (n_eps < max_eps) {
        ep_lane[n_eps] = lane;
        ep_start[n_eps] = p.start;
        ep_len[n_eps] = p.len;
        ep_off[n_eps] = total;
      }
      total += p.len;
      n_eps += 1;
      cand += 1;
    }
    s_pos = pos;
  }
  if (fallback) {  // (uniform)
    __syncthreads();
    pos_now = s_pos;  // thread 0's err / n_eps / total are the minibatch's; the others only need the position
  } else if (err == 0) {
    pos_now = pos0 + 2 * draws;
  }
  if (tid == 0) {
    counts->n_eps = n_eps;
    counts->n_steps = total;
    counts->error = err != 0 ? err : rp_error;
    counts->pad = 0;
  }
  }
  if (tid == 0) *agent_pos = pos_now;
}

// `stream`: the engine's stream, or the side stream an update draws its later minibatches on (not profiled there)
void launch_dqn_sample(rl_engine *eng, hipStream_t stream, const ReplayDev &rp, const AgentKey &key,
                       uint64_t *d_agent_pos, uint32_t minibatch_steps, uint32_t max_eps, const EpisodeLists &ep,
                       DqnCountsDev *d_counts, int sequential, uint32_t n_batches) {
  std::unique_ptr<ProfScope> ps;
  if (stream == eng->stream) ps.reset(new ProfScope(eng, RL_K_SMALL));
  const auto kernel = rp.N <= (uint32_t)SAMPLE_META_LANES ? k_dqn_sample<true> : k_dqn_sample<false>;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(SAMPLE_BLOCK), 0, stream, rp, key, d_agent_pos, minibatch_steps, max_eps,
                     ep.lane, ep.start, ep.len, ep.off, d_counts, sequential, n_batches);
  RL_HIP_CHECK(hipGetLastError());
}

static inline uint32_t cdiv_d(size_t a, size_t b) { return (uint32_t)((a + b - 1) / b); }

// The collection kernels are built per (env kind, D): `go(Env{}, D)` receives the env's ops struct and its feature count
// as types, as env_dispatch does for the standalone env kernels (kernels_rollout.hip).  CartPole lanes have 4 or 5
// features; index-env lanes (Chain, bandit: 5 or 6; MemoryGame(2, h): 2 + h [+ 1]) 4..`MAX_D`.
template <int D>
using FeatureCount = std::integral_constant<int, D>;
template <int MAX_D, class Go>
static void dqn_env_dispatch(const rl_env *env, const char *what, Go &&go) {
  if (env->kind == RL_ENV_TABULAR_MDP) {  // states [+ 1] = 2..8 features; the step-wise collection alone
    if constexpr (MAX_D >= 8) {
      switch (env->D) {
        case 2: go(MdpOps{}, FeatureCount<2>{}); return;
        case 3: go(MdpOps{}, FeatureCount<3>{}); return;
        case 4: go(MdpOps{}, FeatureCount<4>{}); return;
        case 5: go(MdpOps{}, FeatureCount<5>{}); return;
        case 6: go(MdpOps{}, FeatureCount<6>{}); return;
        case 7: go(MdpOps{}, FeatureCount<7>{}); return;
        case 8: go(MdpOps{}, FeatureCount<8>{}); return;
      }
    }
    throw RlError(RL_ERR_UNSUPPORTED, what);
  }
  const bool cartpole = env->kind == RL_ENV_CARTPOLE;
  // (meta lanes and any kind this function does not know are never collected by the index lanes' code)
  if (!cartpole && env->kind != RL_ENV_CHAIN && env->kind != RL_ENV_MEMORY && env->kind != RL_ENV_BANDIT)
    throw RlError(RL_ERR_UNSUPPORTED, what);
  if (env->D < 4 || env->D > (cartpole ? 5u : (uint32_t)MAX_D)) throw RlError(RL_ERR_UNSUPPORTED, what);
  if (cartpole) {
    if (env->D == 5) go(CartPoleOps{}, FeatureCount<5>{});
    else go(CartPoleOps{}, FeatureCount<4>{});
    return;
  }
  switch (env->D) {
    case 4: go(IndexOps{}, FeatureCount<4>{}); break;
    case 5: go(IndexOps{}, FeatureCount<5>{}); break;
    case 6: if constexpr (MAX_D >= 6) go(IndexOps{}, FeatureCount<6>{}); break;
    case 7: if constexpr (MAX_D >= 7) go(IndexOps{}, FeatureCount<7>{}); break;
    default: if constexpr (MAX_D >= 8) go(IndexOps{}, FeatureCount<8>{}); break;
  }
}
// ... and the kernels that read the store per feature count alone
template <class Go>
static void dqn_features_dispatch(uint32_t D, Go &&go) {
  switch (D) {
    case 2: go(FeatureCount<2>{}); break;  // (2 and 3: tabular-MDP lanes of two or three features)
    case 3: go(FeatureCount<3>{}); break;
    case 4: go(FeatureCount<4>{}); break;
    case 5: go(FeatureCount<5>{}); break;
    case 6: go(FeatureCount<6>{}); break;
    case 7: go(FeatureCount<7>{}); break;
    case 8: go(FeatureCount<8>{}); break;
    default: throw RlError(RL_ERR_UNSUPPORTED, "DQN replay store: 2..8 observation features");
  }
}

// ... and the kernels built per action count (FiniteSpace of 2..8 actions: rl_dqn_create_finite)
template <class Go>
static void dqn_actions_dispatch(uint32_t A, Go &&go) {
  switch (A) {
    case 2: go(std::integral_constant<int, 2>{}); break;
    case 3: go(std::integral_constant<int, 3>{}); break;
    case 4: go(std::integral_constant<int, 4>{}); break;
    case 5: go(std::integral_constant<int, 5>{}); break;
    case 6: go(std::integral_constant<int, 6>{}); break;
    case 7: go(std::integral_constant<int, 7>{}); break;
    case 8: go(std::integral_constant<int, 8>{}); break;
    default: throw RlError(RL_ERR_UNSUPPORTED, "DQN kernels: 2..8 actions");
  }
}

void launch_rollout_dqn(rl_env *env, const rl_mlp *qnet, const ReplayDev &rp, uint32_t T, uint64_t p_int,
                        int always_explore, uint8_t *d_flags, uint32_t *d_range) {
  ProfScope ps(env->eng, RL_K_ROLLOUT);
  // threads per lane: as many as keep the launch within one wave per SIMD (launch_rollout, kernels_rollout.hip); a
  // collection that always explores never runs the forward and keeps one thread per lane
  const uint64_t simds = 4ull * (uint64_t)env->eng->prop.multiProcessorCount, n = env->cfg.n_lanes;
  int G = 1;
  while (!always_explore && G < 16 && n * (uint64_t)(2 * G) <= simds * 64) G *= 2;
  if (env->eng->kernel_variant == 1) G = 1;
  dqn_env_dispatch<5>(env, "fused DQN collection: 4 or 5 observation features", [&](auto ops, auto d) {
    using Env = decltype(ops);
    constexpr int D = decltype(d)::value, BLOCK = 64;
#define ROLLOUT_DQN(GG)                                                                                                 \
  hipLaunchKernelGGL((k_rollout_dqn<Env, D, BLOCK, GG>), dim3(cdiv_d((size_t)n * GG, BLOCK)), dim3(BLOCK), 0,          \
                     env->eng->stream, env->dev, env->st, rp, qnet->d_params, (int)qnet->hidden, T, p_int,             \
                     always_explore, d_flags, d_range, env->t_global)
    switch (G) {
      case 16: ROLLOUT_DQN(16); break;
      case 8: ROLLOUT_DQN(8); break;
      case 4: ROLLOUT_DQN(4); break;
      case 2: ROLLOUT_DQN(2); break;
      default: ROLLOUT_DQN(1); break;
    }
#undef ROLLOUT_DQN
  });
  RL_HIP_CHECK(hipGetLastError());
}

void launch_rollout_dqn_general(rl_env *env, const rl_mlp *qnet, rl_traj *ws, float *d_q, const ReplayDev &rp, uint32_t T,
                                uint64_t p_int, int always_explore, uint8_t *d_flags) {
  ProfScope ps(env->eng, RL_K_ROLLOUT);
  constexpr int BLOCK = 64;
  const uint32_t n = (uint32_t)env->cfg.n_lanes;
  for (uint32_t t = 0; t < T; ++t) {
    if (!always_explore) {  // (a collection that always explores never reads the module)
      launch_env_observe(env, env->d_obs);                          // [D][n]
      launch_gen_forward(ws, qnet, env->d_obs, (size_t)n, n, d_q);  // [A][n]
    }
    dqn_env_dispatch<8>(env, "step-wise DQN collection: 4..8 observation features", [&](auto ops, auto d) {
      using Env = decltype(ops);
      constexpr int D = decltype(d)::value;
      // more than two actions: the index-env lanes (MemoryGame(k >= 3, h), the bandit of 3..8 arms) and tabular MDPs
      if constexpr (std::is_same<Env, IndexOps>::value || std::is_same<Env, MdpOps>::value) {
        if (env->A > 2) {
          dqn_actions_dispatch(env->A, [&](auto na) {
            constexpr int A = decltype(na)::value;
            if constexpr (A > 2)
              hipLaunchKernelGGL((k_dqn_lane_step<Env, D, BLOCK, A>), dim3(cdiv_d(n, BLOCK)), dim3(BLOCK), 0,
                                 env->eng->stream, env->dev, env->st, rp, d_q, p_int, always_explore, t + 1 == T ? 1 : 0,
                                 d_flags + (size_t)t * n, env->t_global + t);
          });
          return;
        }
      }
      hipLaunchKernelGGL((k_dqn_lane_step<Env, D, BLOCK, 2>), dim3(cdiv_d(n, BLOCK)), dim3(BLOCK), 0, env->eng->stream,
                         env->dev, env->st, rp, d_q, p_int, always_explore, t + 1 == T ? 1 : 0, d_flags + (size_t)t * n,
                         env->t_global + t);
    });
  }
  RL_HIP_CHECK(hipGetLastError());
}

void launch_dqn_td_targets(rl_engine *eng, float *d_target, const uint8_t *d_flag, const float *d_q_next, uint32_t n,
                           uint32_t n_actions, float gamma) {
  ProfScope ps(eng, RL_K_VALUES);
  if (n == 0) return;
  dqn_actions_dispatch(n_actions, [&](auto na) {
    hipLaunchKernelGGL(k_dqn_td_targets<decltype(na)::value>, dim3(cdiv_d(n, 256)), dim3(256), 0, eng->stream, d_target,
                       d_flag, d_q_next, n, gamma);
  });
}

void launch_dqn_build_minibatch(rl_engine *eng, const ReplayDev &rp, uint32_t n_eps, const EpisodeLists &ep, float *d_obs,
                                size_t out_plane, uint8_t *d_action, float *d_target, float gamma, int one_step_td,
                                const rl_mlp *qnet) {
  ProfScope ps(eng, RL_K_VALUES);
  if (n_eps == 0) return;
  if (one_step_td && rp.D > 5)  // (rl_dqn's general modules take launch_dqn_build_all + launch_dqn_td_targets)
    throw RlError(RL_ERR_UNSUPPORTED, "in-kernel one-step TD targets: 4 or 5 observation features");
  dqn_features_dispatch(rp.D, [&](auto d) {
    hipLaunchKernelGGL(k_dqn_build_minibatch<decltype(d)::value>, dim3(n_eps), dim3(64), 0, eng->stream, rp, ep, d_obs,
                       out_plane, d_action, d_target, gamma, one_step_td, qnet->d_params, (int)qnet->hidden);
  });
}

void launch_dqn_build_all(rl_engine *eng, const ReplayDev &rp, uint32_t n_batches, uint32_t widest_eps, uint32_t max_eps,
                          const EpisodeLists &ep, const DqnCountsDev *d_counts, float *d_obs, size_t obs_stride,
                          uint8_t *d_action, float *d_target, size_t step_stride, float gamma, uint8_t *d_flag) {
  ProfScope ps(eng, RL_K_VALUES);
  if (n_batches == 0 || widest_eps == 0) return;
  const dim3 grid(cdiv_d(widest_eps, BUILD_ALL_WAVES), n_batches), block(BUILD_ALL_WAVES * 64);
  dqn_features_dispatch(rp.D, [&](auto d) {
    hipLaunchKernelGGL(k_dqn_build_all<decltype(d)::value>, grid, block, 0, eng->stream, rp, ep, max_eps, d_counts, d_obs,
                       obs_stride, d_action, d_target, step_stride, gamma, d_flag);
  });
  RL_HIP_CHECK(hipGetLastError());
}

// ================================================================================================
// The DQN gradient on the bf16 matrix pipe: forward + MSE loss + backward of the 5-128-2 action-value MLP over one
// minibatch — mean((Q(s)[a] - target)^2), dqn.rs:316-326 — with the tile machinery of bf16_tile.hpp (exact three-piece
// products, f32 accumulation; kernels_critic.hip is the one-output version of this kernel).  The loss gradient reaches
// the hidden layer through row a_s of the output weights, so the masked sums over the samples come in two channels,
//   M_c[j][k] = sum_{s : a_s = c} [pre_sj > 0] g_s x~_sk,  g_s = 2 (Q(s)[a_s] - target_s) / B,
// (36 piece columns: one more accumulator set than fits beside the forward at two waves per SIMD — the kernel runs four
// waves per workgroup with the whole register file; a minibatch is ~3 tiles per wave, so latency, not issue, binds) and
//   dW1[j][k] = W2[0][j] M_0[j][k] + W2[1][j] M_1[j][k],   db1[j] likewise with k = 5,
//   dW2[c][j] = sum_k W~1[j][k] M_c[j][k],                  db2[c] = sum_{a_s = c} g_s.
// The forward carries both output chains (relu through |x|, as in the critic step) and picks Q(s)[a_s] per sample.
// ================================================================================================
constexpr int DQN_WAVES = 4;
constexpr int DQN_FLUSH = 16;  // f32 -> f64 flush period in tiles

// The kernel of the in-kernel one-step TD targets (given targets take k_critic_step_mfma<2>, kernels_critic.hip): the
// workspace holds rewards instead of targets (`adv`), successor codes (`flag`) and the successor observation in time
// slot 1 of the T = 1 layout; the one-step TD target r + gamma max_a Q(s') (0 beyond a Terminate; critics/mod.rs:
// 139-150, 203-229) comes from a second forward with the same parameters (torch's no_grad target of dqn.rs:299-311).
__global__ void __launch_bounds__(DQN_WAVES * 64)
    k_dqn_step_bf16(TrajDev tr, const float *__restrict__ params, const uint32_t *__restrict__ wimg,
                    double *__restrict__ slabA,
                    double *__restrict__ slabB, float two_over_B, uint32_t P, float gamma) {
  using bt::f32x16;
  using bt::Frag;
  constexpr int H = 128, NT = bt::NT, A = 2;
  constexpr int CH = H * 7;            // one channel's image: per hidden unit M[0..5] (slot 6 unused)
  constexpr int IMG = A * CH + A + 1;  // two channels, db2[0], db2[1], loss
  __shared__ float Ysh[DQN_WAVES][A][32][33];
  __shared__ double Acc[DQN_WAVES][IMG];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 31, hf = lane >> 5;
  const float *__restrict__ W2 = params + bt::PAR_W2, *__restrict__ b2 = params + bt::par_b2(A);
  const size_t B = (size_t)tr.T * tr.n;
  const size_t plane = (size_t)(tr.T + 1) * tr.n;
  double *acc64 = Acc[wave];
  bool flushed = false;  // (the wave's f64 image is not zeroed: its first flush stores, bt::flush)

  Frag fw[NT][3];
  float w2v[A][NT];
  float lv[A][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};  // the linear half of relu, per output
  const bool guard = blockIdx.x == 0 && wave == 0 && tr.range != nullptr;  // the numeric range guard (bf16_tile.hpp)
  float gxmin = 0.0f, gxmax = 0.0f;
  if (guard) bt::range_bounds(tr.range, lane, gxmin, gxmax);
  // (the 2^96-scaled pieces — relu' by conversion, bf16_tile.hpp; the |pre| chains take the scale back out — come
  // ready-made from the module's weight image, written by whoever wrote the parameters.  This is bt::load_weights
  // written out: through the helper the compiler keeps the fragments of this kernel, the one with the whole register
  // file, in other registers — 76 more moves and 2 % on a launch, measured.)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    bt::WRaw r;
    bt::wimg_load(wimg, t, lane, fw[t], r, 2);
    if (guard)  // (one wave sees all 128 units)
      bt::range_guard_img(r, hf, gxmin, gxmax, tr.range_err + bt::GUARD_POLICY, bt::range_veto(tr.range, bt::GUARD_POLICY));
#pragma unroll
    for (int a = 0; a < A; ++a) {
      const float w2 = r.w2[a];
      lv[a][0] = __builtin_fmaf(w2, r.wa, lv[a][0]);
      lv[a][1] = __builtin_fmaf(w2, r.wb, lv[a][1]);
      lv[a][2] = __builtin_fmaf(w2, r.wc, lv[a][2]);
      w2v[a][t] = bt::FWD_UNSCALE * w2;
    }
  }
#pragma unroll
  for (int a = 0; a < A; ++a)
#pragma unroll
    for (int q = 0; q < 3; ++q) lv[a][q] = bt::half_sum(lv[a][q]);
  const float b20 = b2[0], b21 = b2[1];
  f32x16 dm[A][NT];
#pragma unroll
  for (int a = 0; a < A; ++a)
#pragma unroll
    for (int t = 0; t < NT; ++t) dm[a][t] = (f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double loss64 = 0.0, db64[A] = {0.0, 0.0};
  float loss32 = 0.0f, db32[A] = {0.0f, 0.0f};
  bt::wave_lds_fence();

  Frag selb[2];
  bt::sel_frags(lane, selb);
  const size_t n_tiles = (B + 31) / 32;
  const size_t wave_id = (size_t)blockIdx.x * DQN_WAVES + wave, n_waves = (size_t)gridDim.x * DQN_WAVES;
  int since_flush = 0;
  struct TileOp {
    float xa, xb, xc, tgt;
    float na, nb, nc;  // the successor observation
    int act, succ;
    bool valid;
  };
  const uint32_t B32 = (uint32_t)B, plane32 = (uint32_t)plane;
  auto load_tile = [&](size_t g) {  // (branch-free: padding lanes read sample B - 1 and are zeroed)
    TileOp o;
    const uint32_t sidx = (uint32_t)g * 32u + (uint32_t)n;
    o.valid = g < n_tiles && sidx < B32;
    const uint32_t sc = o.valid ? sidx : B32 - 1;
    const float xa = tr.obs[(uint32_t)(2 * hf) * plane32 + sc], xb = tr.obs[(uint32_t)(2 * hf + 1) * plane32 + sc];
    const float xc = tr.obs[4u * plane32 + sc], tg = tr.adv[sc];  // (the minibatch workspace keeps its targets in `adv`)
    const int act = (int)tr.action[sc];
    o.xa = o.valid ? xa : 0.0f;
    o.xb = o.valid ? xb : 0.0f;
    o.xc = o.valid ? xc : 0.0f;
    o.tgt = o.valid ? tg : 0.0f;
    o.act = o.valid ? act : 0;
    const uint32_t s1 = B32 + sc;  // time slot 1
    const float na = tr.obs[(uint32_t)(2 * hf) * plane32 + s1], nb = tr.obs[(uint32_t)(2 * hf + 1) * plane32 + s1];
    const float nc = tr.obs[4u * plane32 + s1];
    const int succ = (int)tr.flag[sc];
    o.na = o.valid ? na : 0.0f;
    o.nb = o.valid ? nb : 0.0f;
    o.nc = o.valid ? nc : 0.0f;
    o.succ = o.valid ? succ : RL_SUCC_TERMINATE;
    return o;
  };
  auto flush_all = [&]() {
    bt::flush(dm[0], acc64, 7, n, hf, !flushed);
    bt::flush(dm[1], acc64 + CH, 7, n, hf, !flushed);
    flushed = true;
    loss64 += (double)loss32;
    db64[0] += (double)db32[0];
    db64[1] += (double)db32[1];
    loss32 = db32[0] = db32[1] = 0.0f;
  };

  TileOp op = load_tile(wave_id);
  for (size_t g = wave_id; g < n_tiles; g += n_waves) {
    const TileOp next = load_tile(g + n_waves);
    Frag ga[NT][2];
    // both action values of one observation per sample lane; `masks`: keep relu' of this forward for the backward
    auto forward = [&](float xa, float xb, float xc, bool masks, float (&qv)[A]) {
      Frag fa[3];
      bt::input_frags(xa, xb, xc, op.valid, hf, fa);
      float yp[A][16];
#pragma unroll
      for (int a = 0; a < A; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) yp[a][r] = 0.0f;
      f32x16 c = bt::layer1(fa, fw[0]);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f32x16 cn = c;
        if (t + 1 < NT) cn = bt::layer1(fa, fw[t + 1]);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float ab = __builtin_fabsf(c[r]);
          yp[0][r] = __builtin_fmaf(ab, w2v[0][t], yp[0][r]);
          yp[1][r] = __builtin_fmaf(ab, w2v[1][t], yp[1][r]);
        }
        if (masks) bt::mask_tile(c, ga[t]);
        c = cn;
      }
      // both outputs: transpose the 16 partial sums per lane through LDS (row = sample, column = source lane)
#pragma unroll
      for (int a = 0; a < A; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) Ysh[wave][a][(r & 3) + 8 * (r >> 2) + 4 * hf][n] = yp[a][r];
      bt::wave_lds_fence();
#pragma unroll
      for (int a = 0; a < A; ++a) {
        float part = bt::row_sum16(&Ysh[wave][a][n][hf * 16]);
        float lin = lv[a][0] * xa;
        lin = __builtin_fmaf(lv[a][1], xb, lin);
        lin = __builtin_fmaf(lv[a][2], hf == 0 ? xc : 1.0f, lin);
        part = part + lin;
        float p0, p1;
        bt::both_halves(part, p0, p1);
        qv[a] = 0.5f * (p0 + p1) + (a == 0 ? b20 : b21);
      }
      bt::wave_lds_fence();  // Ysh is rewritten by the next forward
    };
    float qn[A];
    forward(op.na, op.nb, op.nc, false, qn);
    const float vnext = op.succ == RL_SUCC_TERMINATE ? 0.0f : (qn[1] > qn[0] ? qn[1] : qn[0]);  // amax(-1)
    const float dn = gamma * vnext;
    const float tgt = op.tgt + dn;  // (op.tgt holds the reward)
    float qv[A];
    forward(op.xa, op.xb, op.xc, true, qv);
    const float d = (op.act == 0 ? qv[0] : qv[1]) - tgt;
    const float gq = op.valid ? d * two_over_B : 0.0f;
    const float g0 = op.act == 0 ? gq : 0.0f, g1 = op.act == 0 ? 0.0f : gq;
    if (hf == 0 && op.valid) {
      loss32 = __builtin_fmaf(d, d, loss32);
      db32[0] = db32[0] + g0;
      db32[1] = db32[1] + g1;
    }
    Frag ub[2];
    bt::piece_frags_mfma(g0, op.xa, op.xb, op.xc, hf, selb, ub);
    bt::backward(ga, ub, dm[0]);
    bt::piece_frags_mfma(g1, op.xa, op.xb, op.xc, hf, selb, ub);
    bt::backward(ga, ub, dm[1]);
    if (++since_flush == DQN_FLUSH) {
      since_flush = 0;
      flush_all();
    }
    op = next;
  }
  if (since_flush != 0 || !flushed) flush_all();  // (nothing left when the last tile ended a flush period; a wave
                                                  // without tiles still defines its image)
  const double l = bt::owner_sum(loss64, hf), s0 = bt::owner_sum(db64[0], hf), s1 = bt::owner_sum(db64[1], hf);
  if (lane == 0) {
    acc64[A * CH] = s0;
    acc64[A * CH + 1] = s1;
    acc64[A * CH + 2] = l;
  }
  __syncthreads();
  auto tot = [&](int src) { return bt::image_sum<DQN_WAVES>(Acc, src); };
  for (uint32_t p = threadIdx.x; p < P; p += DQN_WAVES * 64) {
    double s;
    if (p < bt::par_b2(A)) {
      s = bt::grad_entry<2>(p, params, [&](int c, int j, int k) { return tot(c * CH + j * 7 + k); },
                            [&](int c, int j) { return (double)W2[c * H + j]; });
    } else {
      s = tot(A * CH + (int)(p - bt::par_b2(A)));  // db2[0], db2[1]
    }
    slabA[(size_t)blockIdx.x * P + p] = s;
  }
  if (threadIdx.x < 4) slabB[(size_t)blockIdx.x * 4 + threadIdx.x] = threadIdx.x == 0 ? tot(A * CH + 2) : 0.0;
}

// returns false when the kernel is not built for this shape (the caller falls back to the f32 passes)
bool launch_dqn_step_bf16(rl_traj *mb, const rl_mlp *qnet, uint64_t B_total, float gamma) {
  if (!fused_5_128_fits(mb, qnet, 2)) return false;  // (rl_dqn_create takes feed-forward modules only)
  const uint32_t *wimg = wimg_ensure(qnet);
  ProfScope ps(mb->eng, RL_K_POLICY_FUSED);
  mb->nbV2 = fused_grid(mb, DQN_WAVES);  // slab rows of this launch (the slabs are sized for any grid up to 8 x CUs)
  const TrajDev d = fused_traj_dev(mb, mb->guard_next_policy);
  hipLaunchKernelGGL(k_dqn_step_bf16, dim3(mb->nbV2), dim3(DQN_WAVES * 64), 0, mb->eng->stream, d, qnet->d_params,
                     wimg, mb->slabA, mb->slabB, 2.0f / (float)B_total, (uint32_t)qnet->P, gamma);
  RL_HIP_CHECK(hipGetLastError());
  return true;
}

// rl_dqn_replay_read: the store's step data in the documented plane layouts ([D][C][N] features, [C][N] the rest; lane
// fastest) out of the records — a test / inspection path
__global__ void __launch_bounds__(256) k_replay_planes(ReplayDev rp, int field, void *__restrict__ out) {
  const size_t cn = (size_t)rp.C * rp.N;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= cn) return;
  const uint32_t lane = (uint32_t)(idx % rp.N), slot = (uint32_t)(idx / rp.N);
  const size_t o = (size_t)lane * rp.C + slot;
  if (field == RL_REPLAY_OBS) {
    for (uint32_t d = 0; d < rp.D && d < 5; ++d) static_cast<float *>(out)[d * cn + idx] = rp.rec[o].x[d];
    if (rp.D > 5) {  // (the second record array exists)
      const float4 h = rp.hi[o];
      for (uint32_t d = 5; d < rp.D; ++d) static_cast<float *>(out)[d * cn + idx] = d == 5 ? h.x : d == 6 ? h.y : h.z;
    }
  } else if (field == RL_REPLAY_NEXT_OBS) {
    for (uint32_t d = 0; d < rp.D; ++d) static_cast<float *>(out)[d * cn + idx] = rp.next[o].x[d];
  } else if (field == RL_REPLAY_ACTION) {
    static_cast<uint8_t *>(out)[idx] = (uint8_t)(rp.rec[o].af & 0xffu);
  } else if (field == RL_REPLAY_FLAG) {
    static_cast<uint8_t *>(out)[idx] = (uint8_t)(rp.rec[o].af >> 8);
  } else {
    static_cast<float *>(out)[idx] = rp.rec[o].reward;
  }
}

void launch_replay_planes(rl_engine *eng, const ReplayDev &rp, int field, void *d_out) {
  const size_t cn = (size_t)rp.C * rp.N;
  hipLaunchKernelGGL(k_replay_planes, dim3(cdiv_d(cn, 256)), dim3(256), 0, eng->stream, rp, field, d_out);
  RL_HIP_CHECK(hipGetLastError());
}

// ================================================================================================
// Recurrent action-value modules (rl_dqn_create_recurrent): the sampled episodes as a trajectory-shaped workspace.
// seq_packed(observations) runs every sampled episode from the zero state over all of its steps (dqn.rs:293-326), so a
// minibatch of n_eps episodes is laid out as n_eps lane columns of T = its longest episode: column e holds episode e in
// slots 0 .. len_e - 1, the teacher-forced forward / backward of kernels_seq_stack.hip run on it as on any trajectory.
// A padding slot (t >= len_e) holds a zero observation and the successor code Terminate: the state restarts behind it,
// nothing flows back through it, and the terms below give it dz = 0 and no share in the loss or its divisor.
// ================================================================================================

// the longest episode of each minibatch of a draw -> counts[b].pad (read back with the counts)
__global__ void __launch_bounds__(256) k_dqn_longest(EpisodeLists ep, uint32_t max_eps,
                                                     DqnCountsDev *__restrict__ counts) {
  __shared__ uint32_t red[256];
  const uint32_t b = blockIdx.x, n_eps = counts[b].n_eps < max_eps ? counts[b].n_eps : max_eps;
  uint32_t m = 0;
  for (uint32_t e = threadIdx.x; e < n_eps; e += 256) {
    const uint32_t l = ep.len[(size_t)b * max_eps + e];
    m = l > m ? l : m;
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x + s] > red[threadIdx.x] ? red[threadIdx.x + s] : red[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[b].pad = red[0];
}

// the gather: one thread per slot b = t * n + e of the workspace (`given`: the compact targets of the episode-after-episode
// arrays — reward-to-go; NULL: the slot's reward, to which k_dqn_seq_td_targets adds the successor's value)
template <int D>
__global__ void __launch_bounds__(256) k_dqn_build_seq(ReplayDev rp, EpisodeLists ep, TrajDev tr,
                                                       const float *__restrict__ given) {
  const uint32_t n = tr.n, T = tr.T;
  const size_t B = (size_t)T * n, plane = (size_t)(T + 1) * n;
  const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const uint32_t e = (uint32_t)(b % n), t = (uint32_t)(b / n);
  StoredStep<D> s{};  // (a padding slot: a zero observation, action 0, no reward ...
  s.succ = RL_SUCC_TERMINATE;  // ... and the state restarts behind it)
  float tgt = 0.0f;
  if (t < ep.len[e]) {
    const uint32_t lane = ep.lane[e], slot = (ep.start[e] + t) % rp.C;
    s = step_load<D>(rp, lane, slot);
    tgt = given != nullptr ? given[ep.off[e] + t] : s.reward;
    if (s.succ == RL_SUCC_INTERRUPT) {
      float nx[D];
      next_load<D>(rp, lane, slot, nx);
#pragma unroll
      for (int d = 0; d < D; ++d) tr.term_obs[(size_t)d * B + b] = nx[d];
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    tr.obs[(size_t)d * plane + b] = s.x[d];
    if (t + 1 == T) tr.obs[(size_t)d * plane + B + e] = 0.0f;  // (slot T: never read — no column ends on Continue)
  }
  tr.action[b] = (uint8_t)s.action;
  tr.flag[b] = (uint8_t)s.succ;
  tr.reward[b] = s.reward;
  tr.adv[b] = tgt;
}

// one-step TD targets (critics/mod.rs:101-148) from the forward over the workspace: the module has run over the episode
// plus one slot — the successor observation of an Interrupt (succ) — so V_ext[t + 1] = amax of the next slot's outputs,
// of the successor outputs after an Interrupt, 0 after a Terminate; target = r + gamma * V_ext[t + 1] with
// k_dqn_td_targets' arithmetic (`scalar * tensor`, then add).  Also into the episode-after-episode array (`compact`).
template <int A>
__global__ void __launch_bounds__(256) k_dqn_seq_td_targets(TrajDev tr, EpisodeLists ep, const float *__restrict__ out,
                                                            const float *__restrict__ succ, float gamma,
                                                            float *__restrict__ compact) {
  const uint32_t n = tr.n;
  const size_t B = (size_t)tr.T * n;
  const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const uint32_t e = (uint32_t)(b % n), t = (uint32_t)(b / n);
  if (t >= ep.len[e]) return;
  const uint8_t f = tr.flag[b];
  float vnext = 0.0f;
  // (a Continue slot has a successor slot in its own column: an episode's last step never continues — the second test
  // only keeps a corrupt store from reading past the planes)
  if (f != RL_SUCC_TERMINATE && (f == RL_SUCC_INTERRUPT || t + 1 < tr.T)) {
    const float *__restrict__ src = f == RL_SUCC_INTERRUPT ? succ + b : out + b + n;
    float z[A];
#pragma unroll
    for (int q = 0; q < A; ++q) z[q] = src[(size_t)q * B];
    first_max_index<A>(z, vnext);
  }
  const float dn = gamma * vnext;
  const float tgt = tr.reward[b] + dn;
  tr.adv[b] = tgt;
  compact[ep.off[e] + t] = tgt;
}

// the DQN terms over the output planes q [A][B] (PASS_DQN of policy_terms.hpp): dz[a] = [a == action] 2 (Q_a - target)
// / n_steps, zero on padding, and the f64 sum of (Q_a - target)^2 through slab B
template <int A>
__global__ void __launch_bounds__(256) k_dqn_seq_terms(TrajDev tr, EpisodeLists ep, const float *__restrict__ q,
                                                       float *__restrict__ dz, double *__restrict__ slabB,
                                                       float two_over_B) {
  __shared__ double red[256];
  const uint32_t n = tr.n;
  const size_t B = (size_t)tr.T * n;
  double s0 = 0.0;
  for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < B; b += (size_t)gridDim.x * 256) {
    const uint32_t e = (uint32_t)(b % n), t = (uint32_t)(b / n);
    const bool valid = t < ep.len[e];
    const int act = tr.action[b];
    float z[A];
#pragma unroll
    for (int a = 0; a < A; ++a) z[a] = q[(size_t)a * B + b];
    const float dq = select_action<A>(z, act) - tr.adv[b];
    const float g = dq * two_over_B;
#pragma unroll
    for (int a = 0; a < A; ++a) dz[(size_t)a * B + b] = valid && act == a ? g : 0.0f;
    if (valid) s0 += (double)(dq * dq);
  }
  const double t0 = block_sum<256>(s0, red);
  if (threadIdx.x == 0) {
    slabB[blockIdx.x * 4 + 0] = t0;
    slabB[blockIdx.x * 4 + 1] = 0.0;
    slabB[blockIdx.x * 4 + 2] = 0.0;
    slabB[blockIdx.x * 4 + 3] = 0.0;
  }
}

void launch_dqn_longest(rl_engine *eng, const EpisodeLists &ep, uint32_t max_eps, DqnCountsDev *d_counts,
                        uint32_t n_batches) {
  ProfScope ps(eng, RL_K_SMALL);
  if (n_batches == 0) return;
  hipLaunchKernelGGL(k_dqn_longest, dim3(n_batches), dim3(256), 0, eng->stream, ep, max_eps, d_counts);
  RL_HIP_CHECK(hipGetLastError());
}

void launch_dqn_build_seq(rl_traj *seq, const ReplayDev &rp, const EpisodeLists &ep, const float *d_given) {
  ProfScope ps(seq->eng, RL_K_VALUES);
  const size_t B = (size_t)seq->d.T * seq->d.n;
  dqn_features_dispatch(rp.D, [&](auto d) {
    hipLaunchKernelGGL(k_dqn_build_seq<decltype(d)::value>, dim3(cdiv_d(B, 256)), dim3(256), 0, seq->eng->stream, rp, ep,
                       seq->d, d_given);
  });
  RL_HIP_CHECK(hipGetLastError());
}

void launch_dqn_seq_td_targets(rl_traj *seq, const EpisodeLists &ep, uint32_t n_actions, float gamma, float *d_compact) {
  ProfScope ps(seq->eng, RL_K_VALUES);
  const size_t B = (size_t)seq->d.T * seq->d.n;
  dqn_actions_dispatch(n_actions, [&](auto na) {
    hipLaunchKernelGGL(k_dqn_seq_td_targets<decltype(na)::value>, dim3(cdiv_d(B, 256)), dim3(256), 0, seq->eng->stream,
                       seq->d, ep, seq->seq.out, seq->seq.succ, gamma, d_compact);
  });
  RL_HIP_CHECK(hipGetLastError());
}

void launch_dqn_seq_terms(rl_traj *seq, const EpisodeLists &ep, uint32_t n_actions, uint64_t B_total) {
  ProfScope ps(seq->eng, RL_K_POLICY_PASS);
  dqn_actions_dispatch(n_actions, [&](auto na) {
    hipLaunchKernelGGL(k_dqn_seq_terms<decltype(na)::value>, dim3(seq->nbB), dim3(256), 0, seq->eng->stream, seq->d, ep,
                       seq->seq.out, seq->dz, seq->slabB, 2.0f / (float)B_total);
  });
  RL_HIP_CHECK(hipGetLastError());
}
