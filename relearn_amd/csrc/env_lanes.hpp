// env_lanes.hpp — one env per lane, device code only: the lane state of every env kind, the `Env` policy structs the
// kernels are written over, the one statement of "step a lane and record it" (lane_step), the sinks a record goes to,
// and word `w` of a lane's ChaCha stream (stream_word, LaneActorRng).  DESIGN.md §25 lists who calls what.
//
// Adding an env to a kernel is one ops struct here and one instantiation there.  An ops struct gives
//   State                              the lane's registers
//   load / store (st, i, s)            the lane's words of the struct-of-arrays state in HBM
//   features<D>(c, s, f)               the observation's features
//   step(c, s, a, glane, word, reward) Environment::step + the step-limit tail -> RL_SUCC_*; `word` is the global step
//                                      (an env that draws in its step reads that word of the lane's env stream)
//   reset(c, s, glane)                 Environment::initial_state from the lane's env stream
// Arithmetic contract: device_fns.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/rl_chacha.h"
#include "../../include/rl_detmath.h"
#include "../../include/rl_normal.h"
#include "engine.hpp"

// ---------------------------------------------------------------- word `w` of a lane's ChaCha stream
// uncached: the block is recomputed on every call (kernels that take one word per launch or per step of a tile)
__device__ __forceinline__ uint32_t stream_word(const uint32_t *key, uint64_t stream, uint64_t word) {
  uint32_t w[16];
  rl_chacha_block(key, word >> 4, stream, 4, w);
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k == (int)(word & 15)) v = w[k];
  return v;
}

// cached: sequential per-lane generator, ChaCha8(key), stream = global lane id, next word `pos` (the `rng_actor: Prng` of
// Steps, src/simulation/steps.rs:15-28; a fused rollout starts it at t_global, the DQN collection keeps it in HBM between
// launches).  The current 16-word block is parked in a lane-private LDS column (no bank conflicts: threads are consecutive
// in the fastest dimension) and regenerated every 16 words.
template <int BLOCK>
struct LaneActorRng {
  uint32_t *col;  // &lds[threadIdx.x], stride BLOCK
  const uint32_t *key;
  uint64_t lane, pos, cur_block;
  // the column holds the block of word `pos`
  __device__ void fill() {
    const uint64_t blk = pos >> 4;
    if (blk != cur_block) {
      uint32_t w[16];
      rl_chacha_block(key, blk, lane, 4, w);
#pragma unroll
      for (int k = 0; k < 16; ++k) col[k * BLOCK] = w[k];
      cur_block = blk;
    }
  }
  // word `pos` after fill() (a kernel that fills before a barrier and draws after it)
  __device__ uint32_t take() {
    const uint32_t v = col[(uint32_t)(pos & 15) * BLOCK];
    pos += 1;
    return v;
  }
  __device__ uint32_t next_u32() {
    fill();
    return take();
  }
  // BlockRng::next_u64: two consecutive words, low first
  __device__ uint64_t next_u64() {
    const uint64_t lo = next_u32();
    const uint64_t hi = next_u32();
    return (hi << 32) | lo;
  }
};

// ---------------------------------------------------------------- CartPole physics
// InternalPhysicalConstants::{next_state, angular_acceleration, normal_force}
// (reference src/envs/cartpole.rs:306-446).  f64 throughout, operation order preserved.
__device__ __forceinline__ double cp_angular_acceleration(const CartPoleDev &c, double thdot, double applied_force,
                                                          double signed_cart_friction, double w2, double sin_a,
                                                          double cos_a) {
  double alpha =
      (-applied_force - c.mass_length_pole * w2 * (sin_a + signed_cart_friction * cos_a)) * c.inv_total_mass;
  double beta = c.friction_pole * thdot / c.mass_length_pole;
  double numerator = c.gravity * sin_a + cos_a * (alpha + c.gravity * signed_cart_friction) - beta;
  double denominator =
      c.length_half_pole * (4.0 / 3.0 - c.mass_pole * cos_a * c.inv_total_mass * (cos_a - signed_cart_friction));
  return numerator / denominator;
}

__device__ __forceinline__ double cp_normal_force(const CartPoleDev &c, double acc, double w2, double sin_a,
                                                  double cos_a) {
  return c.total_weight - c.mass_length_pole * (acc * sin_a + w2 * cos_a);
}

struct LaneState {
  double x, xdot, th, thdot;
  uint32_t nv_pos;
  uint32_t steps_remaining;
  uint32_t reset_count;
};

// CartPole::step (cartpole.rs:128-154) + Wrapped<_, StepLimit>::step tail (wrappers/step_limit.rs:216-222).
// Returns the successor code; on Continue/Interrupt `s` holds the next state.
__device__ __forceinline__ int cp_step(const CartPoleDev &c, LaneState &s, int action) {
  double applied_force = action == 0 ? -c.action_force : c.action_force;
  double signed_cart_friction = s.nv_pos ? c.friction_cart : -c.friction_cart;
  double sin_a, cos_a;
  rl_sincos(s.th, &sin_a, &cos_a);
  double w2 = s.thdot * s.thdot;
  double acc = cp_angular_acceleration(c, s.thdot, applied_force, signed_cart_friction, w2, sin_a, cos_a);
  double nf = cp_normal_force(c, acc, w2, sin_a, cos_a);
  uint32_t nv_pos = (rl_f64_bits(nf * s.xdot) >> 63) ? 0u : 1u;  // is_sign_positive
  if (nv_pos != s.nv_pos) {
    signed_cart_friction = -signed_cart_friction;
    acc = cp_angular_acceleration(c, s.thdot, applied_force, signed_cart_friction, w2, sin_a, cos_a);
    nf = cp_normal_force(c, acc, w2, sin_a, cos_a);
  }
  double force_pole = c.mass_length_pole * (w2 * sin_a + acc * cos_a);
  double force_friction = -signed_cart_friction * nf;
  double net_force = applied_force + force_pole + force_friction;
  double cart_acc = net_force * c.inv_total_mass;
  double xdot = s.xdot + c.time_step * cart_acc;
  double x = s.x + c.time_step * xdot;
  double thdot = s.thdot + c.time_step * acc;
  double th = s.th + c.time_step * s.thdot;
  bool terminal = __builtin_fabs(x) > c.max_pos || __builtin_fabs(th) > c.max_angle;
  if (terminal) return RL_SUCC_TERMINATE;
  s.x = x;
  s.xdot = xdot;
  s.th = th;
  s.thdot = thdot;
  s.nv_pos = nv_pos;
  if (c.limit_kind != RL_LIMIT_NONE) {
    s.steps_remaining -= 1;
    if (s.steps_remaining == 0) return RL_SUCC_INTERRUPT;
  }
  return RL_SUCC_CONTINUE;
}

// features_out of StepLimitObsSpace<CartPolePhysicalStateSpace> (spaces/interval.rs:108-116,
// wrappers/step_limit.rs:127-140,194-200): each field `as f32`, `remaining` last.
template <int D>
__device__ __forceinline__ void cp_features(const CartPoleDev &c, const LaneState &s, float (&f)[D]) {
  f[0] = (float)s.x;
  f[1] = (float)s.xdot;
  f[2] = (float)s.th;
  f[3] = (float)s.thdot;
  if (D == 5) f[4] = (float)((double)s.steps_remaining / (double)c.max_steps);
}

// CartPole::initial_state (cartpole.rs:103-115) from the lane's env stream: reset k reads words [8k, 8k+8).
// Of the lane it reads `reset_count` alone and writes every field.
__device__ __forceinline__ void cp_reset(const CartPoleDev &c, LaneState &s, uint64_t global_lane) {
  uint32_t w[16];
  uint32_t k = s.reset_count;
  rl_chacha_block(c.key_env, (uint64_t)(k >> 1), global_lane, 4, w);
  // the upper or the lower half of the block by a bit select per word (v_bfi_b32): an index that depends on the lane
  // would put the block into scratch memory
  const uint32_t hi = 0u - (k & 1u);
  uint32_t v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (w[8 + i] & hi) | (w[i] & ~hi);
  s.x = rl_uniform_f64_from_u64(((uint64_t)v[1] << 32) | v[0], c.init_low, c.init_scale);
  s.xdot = rl_uniform_f64_from_u64(((uint64_t)v[3] << 32) | v[2], c.init_low, c.init_scale);
  s.th = rl_uniform_f64_from_u64(((uint64_t)v[5] << 32) | v[4], c.init_low, c.init_scale);
  s.thdot = rl_uniform_f64_from_u64(((uint64_t)v[7] << 32) | v[6], c.init_low, c.init_scale);
  s.nv_pos = 1;
  s.steps_remaining = c.max_steps;
  s.reset_count = k + 1;
}

__device__ __forceinline__ void lane_load(const EnvStateDev &st, uint32_t i, LaneState &s) {
  s.x = st.x[i];
  s.xdot = st.xdot[i];
  s.th = st.th[i];
  s.thdot = st.thdot[i];
  s.nv_pos = st.nv_pos[i];
  s.steps_remaining = st.steps_remaining[i];
  s.reset_count = st.reset_count[i];
}

__device__ __forceinline__ void lane_store(const EnvStateDev &st, uint32_t i, const LaneState &s) {
  st.x[i] = s.x;
  st.xdot[i] = s.xdot;
  st.th[i] = s.th;
  st.thdot[i] = s.thdot;
  st.nv_pos[i] = (uint8_t)s.nv_pos;
  st.steps_remaining[i] = s.steps_remaining;
  st.reset_count[i] = s.reset_count;
}

// ---------------------------------------------------------------- lanes of the IndexSpace-observation envs
// Chain (chain.rs), MemoryGame (memory.rs) and the deterministic bandit (bandits.rs) share the lane code: `c.mem_actions`
// == 0 selects Chain, `c.bandit` the bandit (launch-uniform branches).  MemoryGame keeps (current_state, initial_state)
// and the word position of the lane's env stream: its only random draw is `rng.gen_range(0..num_actions)` in
// initial_state, taken SEQUENTIALLY from the lane's stream like one worker's env Prng in the reference (a rejection
// loop, so the number of words per reset is not fixed).
struct ChainLane {
  uint32_t state, steps_remaining, reset_count;
  uint32_t initial;   // MemoryGame: the state the episode started in
  uint64_t env_pos;   // MemoryGame: next unread word of the lane's env stream (always even: u64 draws only)
};

__device__ __forceinline__ void chain_load(const EnvStateDev &st, uint32_t i, ChainLane &s) {
  s.state = (uint32_t)st.x[i];
  s.initial = (uint32_t)st.xdot[i];
  s.env_pos = (uint64_t)st.th[i];
  s.steps_remaining = st.steps_remaining[i];
  s.reset_count = st.reset_count[i];
}

__device__ __forceinline__ void chain_store(const EnvStateDev &st, uint32_t i, const ChainLane &s) {
  st.x[i] = (double)s.state;
  st.xdot[i] = (double)s.initial;
  st.th[i] = (double)s.env_pos;  // exact below 2^53 words
  st.steps_remaining[i] = s.steps_remaining;
  st.reset_count[i] = s.reset_count;
}

// features of StepLimit-wrapped IndexSpace observations: one-hot (spaces/index.rs:104-116) [+ remaining]
template <int D>
__device__ __forceinline__ void chain_features(const CartPoleDev &c, const ChainLane &s, float (&f)[D]) {
#pragma unroll
  for (int d = 0; d < D; ++d) f[d] = (uint32_t)d == s.state ? 1.0f : 0.0f;
  if (D == 6) f[5] = (float)((double)s.steps_remaining / (double)c.max_steps);
}

// the same for any number of states (MemoryGame::new(num_actions, history_len): D = num_actions + history_len [+ 1]):
// the remaining-steps feature follows the one-hot.  The standalone env kernels use it; the fused rollouts are built for
// five states and keep chain_features.
template <int D>
__device__ __forceinline__ void index_features(const CartPoleDev &c, const ChainLane &s, float (&f)[D]) {
#pragma unroll
  for (int d = 0; d < D; ++d) f[d] = (uint32_t)d == s.state ? 1.0f : 0.0f;
  if (c.limit_kind == RL_LIMIT_VISIBLE) f[D - 1] = (float)((double)s.steps_remaining / (double)c.max_steps);
}

// rand 0.8.5 `gen_range(0..range)` for u64/usize (UniformInt::sample_single): widening multiply, accept when the low
// half is inside the zone `(range << leading_zeros(range)) - 1`; every attempt reads one u64 = stream words
// (pos, pos + 1), low word first.  The loop ends with probability 1; 64 attempts bound it (each fails w.p. <= 1/2).
// (the block is the purpose here: both words of an attempt come from one)
__device__ __forceinline__ uint32_t lane_gen_range(const uint32_t *key, uint64_t glane, uint64_t &pos, uint64_t range) {
  const uint64_t zone = (range << __clzll((long long)range)) - 1;
  uint64_t hi = 0;
  for (int attempt = 0; attempt < 64; ++attempt) {
    uint32_t w[16];
    rl_chacha_block(key, pos >> 4, glane, 4, w);
    uint32_t lo32 = 0, hi32 = 0;
#pragma unroll
    for (int k = 0; k < 16; k += 2)
      if (k == (int)(pos & 15)) {
        lo32 = w[k];
        hi32 = w[k + 1];
      }
    pos += 2;
    const uint64_t v = ((uint64_t)hi32 << 32) | lo32;
    hi = __umul64hi(v, range);
    if (v * range <= zone) break;
  }
  return (uint32_t)hi;
}

__device__ __forceinline__ void chain_reset(const CartPoleDev &c, ChainLane &s, uint64_t glane) {
  if (c.mem_actions) {  // MemoryGame::initial_state (memory.rs:87-90)
    s.state = lane_gen_range(c.key_env, glane, s.env_pos, c.mem_actions);
    s.initial = s.state;
  } else {
    s.state = 0;  // Chain::initial_state (chain.rs:75-77), no random draw
  }
  s.steps_remaining = c.max_steps;
  s.reset_count += 1;
}

// Chain::step (chain.rs:83-105) / MemoryGame::step (memory.rs:96-114) + the step-limit tail; `word` is the lane's
// env-stream word for this global step (Chain's slip draw)
__device__ __forceinline__ int chain_step(const CartPoleDev &c, ChainLane &s, int action, uint32_t word,
                                          float &reward) {
  if (c.bandit) {  // Bandit::step (bandits.rs:66-77): Deterministic::sample draws nothing
    reward = c.bandit_r[action & 7];
    return RL_SUCC_TERMINATE;
  }
  if (c.mem_actions) {
    if (s.state == c.chain_size - 1) {  // the last of num_actions + history_len states: the answer step
      reward = (uint32_t)action == s.initial ? 1.0f : -1.0f;
      return RL_SUCC_TERMINATE;  // passes through the step limit untouched (step_limit.rs:216-222)
    }
    s.state = s.state < c.mem_actions ? c.mem_actions : s.state + 1;
    reward = 0.0f;
  } else {
    if (rl_u32_to_unit_f32(word) < 0.2f) action = 1 - action;  // Move::invert
    if (action == 0) {  // Move::Left
      s.state = 0;
      reward = 2.0f;
    } else if (s.state == c.chain_size - 1) {
      reward = 10.0f;
    } else {
      s.state += 1;
      reward = 0.0f;
    }
  }
  if (c.limit_kind != RL_LIMIT_NONE) {
    s.steps_remaining -= 1;
    if (s.steps_remaining == 0) return RL_SUCC_INTERRUPT;
  }
  return RL_SUCC_CONTINUE;
}

// ---------------------------------------------------------------- the env side of a kernel, by env kind
struct CartPoleOps {
  using State = LaneState;
  static __device__ __forceinline__ void load(const EnvStateDev &st, uint32_t i, State &s) { lane_load(st, i, s); }
  static __device__ __forceinline__ void store(const EnvStateDev &st, uint32_t i, const State &s) { lane_store(st, i, s); }
  template <int D>
  static __device__ __forceinline__ void features(const CartPoleDev &c, const State &s, float (&f)[D]) {
    cp_features<D>(c, s, f);
  }
  static __device__ __forceinline__ int step(const CartPoleDev &c, State &s, int a, uint64_t, uint64_t, float &reward) {
    reward = 1.0f;  // Reward(1.0) as f32: CartPole::step (cartpole.rs:140)
    return cp_step(c, s, a);
  }
  static __device__ __forceinline__ void reset(const CartPoleDev &c, State &s, uint64_t glane) { cp_reset(c, s, glane); }
};

// index envs of any state count (the standalone env kernels)
struct IndexOps {
  using State = ChainLane;
  static __device__ __forceinline__ void load(const EnvStateDev &st, uint32_t i, State &s) { chain_load(st, i, s); }
  static __device__ __forceinline__ void store(const EnvStateDev &st, uint32_t i, const State &s) { chain_store(st, i, s); }
  template <int D>
  static __device__ __forceinline__ void features(const CartPoleDev &c, const State &s, float (&f)[D]) {
    index_features<D>(c, s, f);
  }
  // Environment::step; the slip draw of global step `word` is word `word` of the lane's env stream
  static __device__ __forceinline__ int step(const CartPoleDev &c, State &s, int a, uint64_t glane, uint64_t word,
                                             float &reward) {
    return chain_step(c, s, a, stream_word(c.key_env, glane, word), reward);
  }
  static __device__ __forceinline__ void reset(const CartPoleDev &c, State &s, uint64_t glane) { chain_reset(c, s, glane); }
};

// ... of five states (the fused rollouts): the features alone differ
struct ChainOps : IndexOps {
  template <int D>
  static __device__ __forceinline__ void features(const CartPoleDev &c, const State &s, float (&f)[D]) {
    chain_features<D>(c, s, f);
  }
};

// ---------------------------------------------------------------- meta-bandit lanes (RL_ENV_META_BANDIT)
// Wrapped<MetaEnv<D>, TrialEpisodeLimit> (src/envs/meta.rs:128-203, 541-617) over Bandit<_> (src/envs/bandits.rs:58-78),
// D = UniformBernoulliBandits (bandits.rs:96-106, 170-181), OneHotBandits (bandits.rs:229-243) or the reference's test
// distribution RoundRobinDeterministicBandits (src/envs/testing.rs:108-160; the good arm of a lane's j-th trial is
// j mod k).  An inner episode is one arm pull; a trial of E inner episodes is 2 E - 1 steps (pull, restart, pull, ...)
// and ends in an Interrupt.  Every draw is one u64 taken SEQUENTIALLY from the lane's env stream (`env_pos`, always
// even), low word first: at a trial's start k uniform means / one gen_range(0..k) / nothing, per pull of a Bernoulli arm
// one u64 unless its mean is exactly 1.0 (rl_bernoulli_*, rl_chacha.h); deterministic arms and the restart step draw
// nothing.  The k means are not kept: `arms` is the word position they were drawn at, and a pull recomputes the mean of
// the pulled arm from the u64 at arms + 2 a (one ChaCha block; the same bits, hence the same mean).
struct MetaLane {
  uint64_t arms;     // UniformBernoulli: word position of arm 0's mean; OneHot / RoundRobin: the arm whose reward is 1
  uint64_t env_pos;  // next unread word of the lane's env stream
  float prev_reward;     // prev_step_obs: Some(InnerStepObs { action, feedback }) when prev_some
  uint32_t prev_action;
  uint32_t prev_some;
  uint32_t inner_done;   // inner_successor is Terminate (a bandit's step always terminates)
  uint32_t remaining;    // inner episodes left in the trial
  uint32_t reset_count;
};

// the u64 at even word position `pos` of the lane's stream: the block is pos >> 4, and because `pos` is even both words
// lie in it.  Every position a meta lane asks for is even: env_pos starts at 0 and moves by 2 per u64 (a trial's k means
// move it by 2 k — at k >= 8 a whole block or more, so arm a's mean at arms + 2 a may lie a block or two behind arm 0's:
// the block is taken from the position asked for, never from `arms`).
__device__ __forceinline__ uint64_t lane_u64_at(const uint32_t *key, uint64_t glane, uint64_t pos) {
  uint32_t w[16];
  rl_chacha_block(key, pos >> 4, glane, 4, w);
  uint32_t lo32 = 0, hi32 = 0;
#pragma unroll
  for (int k = 0; k < 16; k += 2)
    if (k == (int)(pos & 15)) {
      lo32 = w[k];
      hi32 = w[k + 1];
    }
  return ((uint64_t)hi32 << 32) | lo32;
}

struct MetaOps {
  using State = MetaLane;
  static __device__ __forceinline__ void load(const EnvStateDev &st, uint32_t i, State &s) {
    s.arms = (uint64_t)st.x[i];
    s.env_pos = (uint64_t)st.xdot[i];
    s.prev_reward = (float)st.th[i];
    const uint32_t b = st.nv_pos[i];
    s.inner_done = b & 1u;
    s.prev_some = (b >> 1) & 1u;
    s.prev_action = (b >> 2) & 15u;  // bits 2-5: up to 12 arms (at 2..4 arms the byte is the one two bits gave)
    s.remaining = st.steps_remaining[i];
    s.reset_count = st.reset_count[i];
  }
  static __device__ __forceinline__ void store(const EnvStateDev &st, uint32_t i, const State &s) {
    st.x[i] = (double)s.arms;  // exact below 2^53 words
    st.xdot[i] = (double)s.env_pos;
    st.th[i] = (double)s.prev_reward;
    st.nv_pos[i] = (uint8_t)(s.inner_done | (s.prev_some << 1) | (s.prev_action << 2));
    st.steps_remaining[i] = s.remaining;
    st.reset_count[i] = s.reset_count;
  }
  // MetaObservationSpace features (meta.rs:357-363; OptionSpace: spaces/option.rs:87-114; field order of the derived
  // ProductSpace: relearn_derive/src/space.rs:457-512), D = k + 4:
  //   [inner is None] [prev is None] [one-hot(prev action), k] [prev reward] [episode_done]
  // (the singleton inner observation has no feature of its own; the k + 1 entries behind a None marker are zero)
  template <int D>
  static __device__ __forceinline__ void features(const CartPoleDev &, const State &s, float (&f)[D]) {
    f[0] = s.inner_done ? 1.0f : 0.0f;
    f[1] = s.prev_some ? 0.0f : 1.0f;
#pragma unroll
    for (int a = 0; a < D - 4; ++a) f[2 + a] = s.prev_some && (uint32_t)a == s.prev_action ? 1.0f : 0.0f;
    f[D - 2] = s.prev_some ? s.prev_reward : 0.0f;
    f[D - 1] = s.inner_done ? 1.0f : 0.0f;
  }
  // MetaEnv::step (meta.rs:165-202), then the TrialEpisodeLimit tail (meta.rs:596-616).  `word` is unused: the draws
  // are sequential.
  static __device__ __forceinline__ int step(const CartPoleDev &c, State &s, int a, uint64_t glane, uint64_t,
                                             float &reward) {
    if (s.inner_done) {  // the action is ignored: a new inner episode (Bandit::initial_state draws nothing)
      s.inner_done = 0;
      s.prev_some = 0;
      s.prev_action = 0;
      s.prev_reward = 0.0f;
      reward = 0.0f;  // neutral_outer
      return RL_SUCC_CONTINUE;
    }
    float r;
    if (c.meta_dist == RL_BANDITS_UNIFORM_BERNOULLI) {  // Bandit::step (bandits.rs:66-77) on a Bernoulli arm
      const double p = rl_uniform_f64_from_u64(lane_u64_at(c.key_env, glane, s.arms + 2ull * (uint32_t)a), c.init_low,
                                               c.init_scale);
      if (rl_bernoulli_always(p)) {
        r = 1.0f;
      } else {
        const uint64_t v = lane_u64_at(c.key_env, glane, s.env_pos);
        s.env_pos += 2;
        r = rl_bernoulli_from_u64(v, rl_bernoulli_p_int(p)) ? 1.0f : 0.0f;
      }
    } else {  // Deterministic::sample draws nothing
      r = (uint64_t)(uint32_t)a == s.arms ? 1.0f : 0.0f;
    }
    s.prev_some = 1;
    s.prev_action = (uint32_t)a;
    s.prev_reward = r;
    s.inner_done = 1;
    reward = r;
    s.remaining -= 1;
    return s.remaining == 0 ? RL_SUCC_INTERRUPT : RL_SUCC_CONTINUE;
  }
  // TrialEpisodeLimit / MetaEnv::initial_state (meta.rs:580-589, 141-150): sample_environment, then the inner
  // initial_state (no draw)
  static __device__ __forceinline__ void reset(const CartPoleDev &c, State &s, uint64_t glane) {
    if (c.meta_dist == RL_BANDITS_UNIFORM_BERNOULLI) {  // BernoulliBandit::uniform: k means, one u64 each
      s.arms = s.env_pos;
      s.env_pos += 2ull * c.meta_arms;
    } else if (c.meta_dist == RL_BANDITS_ONE_HOT) {  // rng.gen_range(0..num_arms)
      s.arms = lane_gen_range(c.key_env, glane, s.env_pos, c.meta_arms);
    } else {  // RoundRobin: the lane's trial count mod k
      s.arms = s.reset_count % c.meta_arms;
    }
    s.inner_done = 0;
    s.prev_some = 0;
    s.prev_action = 0;
    s.prev_reward = 0.0f;
    s.remaining = c.max_steps;
    s.reset_count += 1;
  }
};

// ---------------------------------------------------------------- tabular-MDP lanes (RL_ENV_TABULAR_MDP)
// TabularMdp<_, Normal<f64>> (src/envs/mdps.rs:12-85) under the index lanes' step limit: one MDP of S states and A actions
// shared by all lanes, given as tables (CartPoleDev::mdp: cum f32 [S][A][S], the running sums of the successor rows;
// mean and stddev f64 [S][A]).  The lane is MemoryGame's — state index, env-stream word position, step limit — and so
// are its columns and its one-hot features.  A step draws SEQUENTIALLY from the lane's env stream at `env_pos` (always
// even): one u64 for the successor, always; then, unless the row's stddev is 0, the polar normal of include/rl_normal.h,
// 4 words per attempt.  The table index depends on the lane's state: these are vector loads through the CU's vector
// cache (the tables are at most 3 KiB), nothing is staged.
// TabularMdp::step's two draws, stated once for the lanes of one shared MDP (MdpOps) and the lanes that each have their own
// (MetaMdpOps).
// s' = #{ j < bound - 1 : cum[j] <= u }: a compare-add per entry under the launch-uniform bound, no register indexing; the
// count cannot leave 0 .. bound - 1, and u == cum[j] goes to the bucket after j.  `cum_at(j)` is entry j of the row.
// ROW: the most entries a row has — 8, and 16 on the meta-MDP lanes of nine and ten states (MetaMdpWideOps).
template <uint32_t ROW = 8, class CumAt>
__device__ __forceinline__ uint32_t mdp_successor_count(CumAt cum_at, uint32_t bound, float u) {
  uint32_t next = 0;
#pragma unroll
  for (uint32_t j = 0; j < ROW - 1; ++j)
    if (j + 1 < bound) next += cum_at(j) <= u ? 1u : 0u;
  return next;
}
// mean + stddev z, formed in f64, with z the polar normal of rl_normal_sample drawn at `pos` over the lane's block select:
// 4 words per attempt, at most 64 attempts.  Always drawn, whatever the stddev.  The one statement of the lanes' normal:
// a reward is this value (where its stddev is not 0), a sampled MDP's mean is, and the standard normal itself is it at
// (0, 1) — 0 + 1 z is z.  (Kept in one function body: with the loop a call further in, k_env_step<MdpOps, ..> takes a
// register more.)
__device__ __forceinline__ double lane_normal_affine(const uint32_t *key, uint64_t glane, uint64_t &pos, double mean,
                                                     double stddev) {
  double z = 0.0;
  for (int attempt = 0; attempt < RL_NORMAL_MAX_ATTEMPTS; ++attempt) {
    const uint64_t w1 = lane_u64_at(key, glane, pos);
    const uint64_t w2 = lane_u64_at(key, glane, pos + 2);
    pos += 4;
    if (rl_normal_attempt(w1, w2, &z)) break;
  }
  return mean + stddev * z;
}

struct MdpOps {
  using State = ChainLane;
  static __device__ __forceinline__ void load(const EnvStateDev &st, uint32_t i, State &s) { chain_load(st, i, s); }
  static __device__ __forceinline__ void store(const EnvStateDev &st, uint32_t i, const State &s) { chain_store(st, i, s); }
  template <int D>
  static __device__ __forceinline__ void features(const CartPoleDev &c, const State &s, float (&f)[D]) {
    index_features<D>(c, s, f);
  }
  // TabularMdp::step (mdps.rs:73-84), then the step-limit tail.  `word` is unused: the draws are sequential.
  static __device__ __forceinline__ int step(const CartPoleDev &c, State &s, int a, uint64_t glane, uint64_t,
                                             float &reward) {
    const uint32_t S = c.mdp.states;
    // (a state or an action outside the tables cannot come from a step or a checked action; rl_env_set_state checks too:
    // the clamps keep the loads inside the tables whatever the columns hold)
    const uint32_t st = s.state < S ? s.state : S - 1;
    const uint32_t ac = (uint32_t)a < c.mdp.actions ? (uint32_t)a : c.mdp.actions - 1;
    const uint32_t row = st * c.mdp.actions + ac;
    const float u = rl_u32_to_unit_f32((uint32_t)lane_u64_at(c.key_env, glane, s.env_pos));
    s.env_pos += 2;
    const float *__restrict__ cum = c.mdp.cum + (size_t)row * S;
    const uint32_t next = mdp_successor_count([&](uint32_t j) { return cum[j]; }, S, u);
    const double mean = c.mdp.mean[row], stddev = c.mdp.stddev[row];
    double r = mean;  // a stddev of 0 draws nothing
    if (stddev != 0.0) r = lane_normal_affine(c.key_env, glane, s.env_pos, mean, stddev);
    reward = (float)r;
    s.state = next;
    if (c.limit_kind != RL_LIMIT_NONE) {
      s.steps_remaining -= 1;
      if (s.steps_remaining == 0) return RL_SUCC_INTERRUPT;
    }
    return RL_SUCC_CONTINUE;
  }
  // TabularMdp::initial_state (mdps.rs:65-67): state 0, no draw
  static __device__ __forceinline__ void reset(const CartPoleDev &c, State &s, uint64_t) {
    s.state = 0;
    s.initial = 0;
    s.steps_remaining = c.max_steps;
    s.reset_count += 1;
  }
};

// ---------------------------------------------------------------- meta-MDP lanes (RL_ENV_META_MDP)
// Wrapped<MetaEnv<Wrapped<DirichletRandomMdps, LatentStepLimit>>, TrialEpisodeLimit> (src/envs/meta.rs:128-203, 541-617;
// mdps.rs:87-171; wrappers/step_limit.rs:13-89): every lane draws its own TabularMdp at a trial's start and keeps its
// tables in device memory (CartPoleDev::mm: cum f32 [n][S*A][8], rows padded with 1.0f; mean f64 [n][S*A]; indexed by the
// LOCAL lane, the streams by the global one).  An inner episode is L steps of TabularMdp::step and ends in the limit's
// Interrupt(state), which keeps the state; the step after it ignores its action and starts the next inner episode; a
// trial of E inner episodes is E (L + 1) - 1 steps and ends in an Interrupt.  Every draw is taken SEQUENTIALLY from the
// lane's env stream at `env_pos` (always even).
struct MetaMdpLane {
  uint64_t env_pos;      // next unread word of the lane's env stream
  uint32_t state;        // the inner state
  uint32_t inner_left;   // inner steps remaining (LatentStepLimit)
  float prev_reward;     // prev_step_obs: Some(InnerStepObs { action, feedback }) when prev_some
  uint32_t prev_action;
  uint32_t prev_some;
  uint32_t inner_done;   // inner_successor is Interrupt(state)
  uint32_t remaining;    // inner episodes left in the trial
  uint32_t reset_count;
};

// Gamma(alpha, 1) = rl_gamma_sample (include/rl_normal.h) over the lane's block select, draw for draw
__device__ __forceinline__ double lane_gamma_sample_ge1(double alpha, const uint32_t *key, uint64_t glane, uint64_t &pos) {
  if (alpha == 1.0) {
    const double u = rl_u64_to_open01_f64(lane_u64_at(key, glane, pos));
    pos += 2;
    return -rl_log(u);
  }
  const double d = alpha - 1.0 / 3.0;
  const double cc = 1.0 / __builtin_sqrt(9.0 * d);
  double g = 0.0;
  for (int attempt = 0; attempt < RL_NORMAL_MAX_ATTEMPTS; ++attempt) {
    const double x = lane_normal_affine(key, glane, pos, 0.0, 1.0);
    const double u = rl_u64_to_open01_f64(lane_u64_at(key, glane, pos));
    pos += 2;
    if (rl_gamma_attempt(d, cc, x, u, &g)) break;
  }
  return g;
}
__device__ __forceinline__ double lane_gamma_sample(double alpha, const uint32_t *key, uint64_t glane, uint64_t &pos) {
  if (alpha < 1.0) {  // (launch-uniform)
    const double g = lane_gamma_sample_ge1(alpha + 1.0, key, glane, pos);
    const double u = rl_u64_to_open01_f64(lane_u64_at(key, glane, pos));
    pos += 2;
    return g * rl_exp(rl_log(u) / alpha);
  }
  return lane_gamma_sample_ge1(alpha, key, glane, pos);
}

// DirichletRandomMdps::sample_environment (mdps.rs:151-170) into the lane's tables, in rl_random_mdps_sample's order; moves
// `pos` behind the last word read: S A (S + 1) variates, once per trial.  The row's S gammas stay in registers: every draw
// is selected into its place (v_cndmask per entry), the loops over a row's entries are unrolled under the launch-uniform S.
// ROW: the floats of a stored row, the constant bound of every loop over a row's entries — 8 (one 32-byte sector, S <= 8)
// or 16 (64 bytes, S = 9..10); a row is ROW / 4 aligned 16-byte stores.
template <uint32_t ROW>
__device__ __forceinline__ void meta_mdp_sample_tables(const CartPoleDev &c, uint64_t glane, uint64_t &pos) {
  const uint32_t S = c.mm.states, rows = S * c.mm.actions;
  const size_t local = (size_t)(glane - c.lane_offset);
  float *cum = c.mm.cum + local * rows * ROW;
  double *mean = c.mm.mean + local * rows;
  const double alpha = c.mm_prior.alpha;
  for (uint32_t row = 0; row < rows; ++row) {
    double g[ROW] = {};
    double sum = 0.0;
    for (uint32_t j = 0; j < S; ++j) {
      const double gj = lane_gamma_sample(alpha, c.key_env, glane, pos);
      sum = sum + gj;
#pragma unroll
      for (uint32_t k = 0; k < ROW; ++k) g[k] = k == j ? gj : g[k];
    }
    float p[ROW] = {};
    float cs[ROW];  // behind S: the padding no draw reaches
#pragma unroll
    for (uint32_t k = 0; k < ROW; ++k) cs[k] = 1.0f;
    rl_dirichlet_row_normalise(g, sum, S, ROW, p);
    rl_mdp_row_cumulative(p, S, ROW, cs);
    float4 *out = reinterpret_cast<float4 *>(cum + (size_t)row * ROW);  // (hipMalloc'd and 32- or 64-byte rows: aligned)
#pragma unroll
    for (uint32_t q = 0; q < ROW / 4; ++q) out[q] = make_float4(cs[4 * q], cs[4 * q + 1], cs[4 * q + 2], cs[4 * q + 3]);
    // Normal::new(reward_prior_mean, reward_prior_stddev).sample: always drawn, as the host sampler does
    mean[row] = lane_normal_affine(c.key_env, glane, pos, c.mm_prior.reward_prior_mean, c.mm_prior.reward_prior_stddev);
  }
}

// The lanes' ops at a row class: ROW = 8 is MetaMdpOps (S <= 8), ROW = 16 MetaMdpWideOps (S = 9..10), both below.
template <uint32_t ROW>
struct MetaMdpRowOps {
  using State = MetaMdpLane;
  // columns: x the inner state, thdot the inner steps remaining, xdot env_pos, th the prev reward; the byte as on MetaOps
  static __device__ __forceinline__ void load(const EnvStateDev &st, uint32_t i, State &s) {
    s.state = (uint32_t)st.x[i];
    s.env_pos = (uint64_t)st.xdot[i];
    s.prev_reward = (float)st.th[i];
    s.inner_left = (uint32_t)st.thdot[i];
    const uint32_t b = st.nv_pos[i];
    s.inner_done = b & 1u;
    s.prev_some = (b >> 1) & 1u;
    s.prev_action = (b >> 2) & 15u;
    s.remaining = st.steps_remaining[i];
    s.reset_count = st.reset_count[i];
  }
  static __device__ __forceinline__ void store(const EnvStateDev &st, uint32_t i, const State &s) {
    st.x[i] = (double)s.state;
    st.xdot[i] = (double)s.env_pos;  // exact below 2^53 words
    st.th[i] = (double)s.prev_reward;
    st.thdot[i] = (double)s.inner_left;
    st.nv_pos[i] = (uint8_t)(s.inner_done | (s.prev_some << 1) | (s.prev_action << 2));
    st.steps_remaining[i] = s.remaining;
    st.reset_count[i] = s.reset_count;
  }
  // MetaObservationSpace features (meta.rs:357-363) with the inner observation's one-hot, D = S + A + 4:
  //   [inner is None] [one-hot(inner state), S] [prev is None] [one-hot(prev action), A] [prev reward] [episode_done]
  // (the inner observation is never None: an inner episode ends in Interrupt(state), whose state stays observable; the
  // A + 1 entries behind a prev-None marker are zero).  S is launch-uniform: the position tests are scalar.
  template <int D>
  static __device__ __forceinline__ void features(const CartPoleDev &c, const State &s, float (&f)[D]) {
    const uint32_t S = c.mm.states;
    f[0] = 0.0f;
#pragma unroll
    for (uint32_t d = 1; d < (uint32_t)D - 2; ++d) {
      float v;
      if (d <= S) v = d - 1 == s.state ? 1.0f : 0.0f;
      else if (d == S + 1) v = s.prev_some ? 0.0f : 1.0f;
      else v = s.prev_some && d - S - 2 == s.prev_action ? 1.0f : 0.0f;
      f[d] = v;
    }
    f[D - 2] = s.prev_some ? s.prev_reward : 0.0f;
    f[D - 1] = s.inner_done ? 1.0f : 0.0f;
  }
  // MetaEnv::step (meta.rs:165-202) over Wrapped<TabularMdp, LatentStepLimit>::step, then the TrialEpisodeLimit tail
  // (meta.rs:596-616).  `word` is unused: the draws are sequential.
  static __device__ __forceinline__ int step(const CartPoleDev &c, State &s, int a, uint64_t glane, uint64_t,
                                             float &reward) {
    if (s.inner_done) {  // the action is ignored: a new inner episode (TabularMdp::initial_state draws nothing)
      s.state = 0;
      s.inner_left = c.mm.inner_steps;
      s.inner_done = 0;
      s.prev_some = 0;
      s.prev_action = 0;
      s.prev_reward = 0.0f;
      reward = 0.0f;  // neutral_outer
      return RL_SUCC_CONTINUE;
    }
    const uint32_t S = c.mm.states, A = c.mm.actions;
    // (the clamps keep the loads inside the lane's tables whatever the columns hold, as on MdpOps)
    const uint32_t st = s.state < S ? s.state : S - 1;
    const uint32_t ac = (uint32_t)a < A ? (uint32_t)a : A - 1;
    const size_t row = (size_t)(glane - c.lane_offset) * (S * A) + st * A + ac;
    const float u = rl_u32_to_unit_f32((uint32_t)lane_u64_at(c.key_env, glane, s.env_pos));
    s.env_pos += 2;
    // the row is one 32-byte sector (ROW 16: two), padded with 1.0f: ROW / 4 16-byte loads and no bound that depends on S
    const float4 *rowp = reinterpret_cast<const float4 *>(c.mm.cum + row * ROW);
    float cs[ROW];
#pragma unroll
    for (uint32_t q = 0; q < ROW / 4; ++q) {
      const float4 v = rowp[q];
      cs[4 * q] = v.x;
      cs[4 * q + 1] = v.y;
      cs[4 * q + 2] = v.z;
      cs[4 * q + 3] = v.w;
    }
    const uint32_t next = mdp_successor_count<ROW>([&](uint32_t j) { return cs[j]; }, ROW, u);
    const double mean = c.mm.mean[row], stddev = c.mm_prior.reward_stddev;
    double rd = mean;  // a stddev of 0 draws nothing
    if (stddev != 0.0) rd = lane_normal_affine(c.key_env, glane, s.env_pos, mean, stddev);
    const float r = (float)rd;
    s.state = next;
    s.prev_some = 1;
    s.prev_action = ac;
    s.prev_reward = r;
    reward = r;
    s.inner_left -= 1;
    if (s.inner_left == 0) {  // the inner limit's Interrupt(state)
      s.inner_done = 1;
      s.remaining -= 1;
      if (s.remaining == 0) return RL_SUCC_INTERRUPT;
    }
    return RL_SUCC_CONTINUE;
  }
  // TrialEpisodeLimit / MetaEnv::initial_state (meta.rs:580-589, 141-150): sample_environment, then the inner
  // initial_state (state 0, no draw)
  static __device__ __forceinline__ void reset(const CartPoleDev &c, State &s, uint64_t glane) {
    meta_mdp_sample_tables<ROW>(c, glane, s.env_pos);
    s.state = 0;
    s.inner_left = c.mm.inner_steps;
    s.inner_done = 0;
    s.prev_some = 0;
    s.prev_action = 0;
    s.prev_reward = 0.0f;
    s.remaining = c.max_steps;
    s.reset_count += 1;
  }
};
// S <= 8 (rl_env_create_meta_mdp): rows of eight floats.  A struct of its own name, so that its kernels keep theirs.
struct MetaMdpOps : MetaMdpRowOps<8> {};
// S = 9..10 (rl_env_create_meta_mdp_wide): rows of sixteen floats, 64 bytes in four 16-byte loads; the successor is the
// count of cum[j] <= u over j < 15
struct MetaMdpWideOps : MetaMdpRowOps<16> {};

// ---------------------------------------------------------------- PartitionGame lanes (RL_ENV_PARTITION)
// PartitionGame (src/envs/partition.rs:86-130) under the index lanes' step limit.  A lane: the supervisor's axis (0..9),
// the element ([bool; 10], bit j = element[j]), the feedback Option<(previous element, its label)>.  Every draw is taken
// SEQUENTIALLY from the lane's env stream at `env_pos`, which stays even: initial_state takes gen_range(0..10) over usize
// (lane_gen_range: whole u64s) and then the element; a step takes the next element.  An element is `rng.gen()` of
// [bool; 10]: ten gen::<bool>() in index order, each one next_u32 whose sign bit is the value, `(x as i32) < 0` — ten
// words.  rand's source is not at hand here: that this equals rand 0.8.5's Standard for bool and for arrays (index order,
// one word per bool) rests on a check against its source (distributions/other.rs), as rl_beta.h says of its sampler.
// The lane's columns: x = the packed word below (< 2^26, exact in a double), th = env_pos as on MemoryGame lanes,
// steps_remaining and reset_count their own; xdot, thdot and nv_pos are not used.
struct PartitionLane {
  uint64_t env_pos;      // next unread word of the lane's env stream (always even)
  uint32_t axis;         // Supervisor::AxisAligned(axis)
  uint32_t element;      // bits 0-9
  uint32_t fb_element;   // feedback: Some((fb_element, fb_label)) when fb_some
  uint32_t fb_label;     // Classification: Left 0, Right 1
  uint32_t fb_some;
  uint32_t steps_remaining, reset_count;
};

// the sign bits of the sixteen words of block `block` of the lane's stream, bit k = word k: constant register indices only
__device__ __forceinline__ uint32_t lane_block_signs(const uint32_t *key, uint64_t glane, uint64_t block) {
  uint32_t w[16];
  rl_chacha_block(key, block, glane, 4, w);
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) m |= (w[k] >> 31) << k;
  return m;
}
// [bool; 10] at word position `pos`: bit j = the sign of word pos + j.  The ten words lie in the block of `pos` when
// (pos & 15) <= 6 and run into the next one otherwise: each block is taken from the position asked for, the two sign masks
// are joined into one 32-bit word and the ten bits shifted out of it — no register array is indexed by the lane's position.
__device__ __forceinline__ uint32_t lane_bool10_at(const uint32_t *key, uint64_t glane, uint64_t pos) {
  const uint32_t k0 = (uint32_t)(pos & 15);
  uint32_t signs = lane_block_signs(key, glane, pos >> 4);
  if (k0 > 6) signs |= lane_block_signs(key, glane, (pos >> 4) + 1) << 16;
  return (signs >> k0) & 0x3FFu;
}

struct PartitionOps {
  using State = PartitionLane;
  static __device__ __forceinline__ void load(const EnvStateDev &st, uint32_t i, State &s) {
    const uint32_t p = (uint32_t)st.x[i];
    s.element = p & 0x3FFu;
    s.fb_element = (p >> 10) & 0x3FFu;
    s.fb_label = (p >> 20) & 1u;
    s.fb_some = (p >> 21) & 1u;
    s.axis = (p >> 22) & 15u;
    s.env_pos = (uint64_t)st.th[i];
    s.steps_remaining = st.steps_remaining[i];
    s.reset_count = st.reset_count[i];
  }
  static __device__ __forceinline__ void store(const EnvStateDev &st, uint32_t i, const State &s) {
    st.x[i] = (double)(s.element | (s.fb_element << 10) | (s.fb_label << 20) | (s.fb_some << 21) | (s.axis << 22));
    st.th[i] = (double)s.env_pos;  // exact below 2^53 words
    st.steps_remaining[i] = s.steps_remaining;
    st.reset_count[i] = s.reset_count;
  }
  // TupleSpace2<PowerSpace<BooleanSpace, 10>, OptionSpace<TupleSpace2<PowerSpace<..>, IndexedTypeSpace<Classification>>>>
  // (spaces/tuple.rs, power.rs, option.rs:95-109, indexed_type.rs:175-187, boolean.rs:132-140), D = 23 [+ 1]:
  //   [element, 10] [feedback is None] [previous element, 10] [one-hot label: Left, Right] [+ remaining]
  // (the 12 entries behind a None marker are zero; `remaining` as the index lanes write it)
  template <int D>
  static __device__ __forceinline__ void features(const CartPoleDev &c, const State &s, float (&f)[D]) {
    static_assert(D == 23 || D == 24, "PartitionGame lanes have 23 features, 24 under a visible limit");
    const uint32_t fb = s.fb_some ? s.fb_element : 0u;
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      f[j] = (s.element >> j) & 1u ? 1.0f : 0.0f;
      f[11 + j] = (fb >> j) & 1u ? 1.0f : 0.0f;
    }
    f[10] = s.fb_some ? 0.0f : 1.0f;
    f[21] = s.fb_some && s.fb_label == 0u ? 1.0f : 0.0f;
    f[22] = s.fb_some && s.fb_label == 1u ? 1.0f : 0.0f;
    if constexpr (D == 24) f[23] = (float)((double)s.steps_remaining / (double)c.max_steps);
  }
  // PartitionGame::step (partition.rs:107-129), then the step-limit tail.  `word` is unused: the draws are sequential.
  static __device__ __forceinline__ int step(const CartPoleDev &c, State &s, int a, uint64_t glane, uint64_t,
                                             float &reward) {
    const uint32_t label = (s.element >> s.axis) & 1u;  // Supervisor::classify: Right when element[axis]
    reward = (uint32_t)a == label ? 1.0f : -1.0f;
    s.fb_some = 1;
    s.fb_element = s.element;
    s.fb_label = label;
    s.element = lane_bool10_at(c.key_env, glane, s.env_pos);
    s.env_pos += 10;
    if (c.limit_kind != RL_LIMIT_NONE) {
      s.steps_remaining -= 1;
      if (s.steps_remaining == 0) return RL_SUCC_INTERRUPT;
    }
    return RL_SUCC_CONTINUE;
  }
  // PartitionGame::initial_state (partition.rs:93-101): the axis, then the element; feedback None
  static __device__ __forceinline__ void reset(const CartPoleDev &c, State &s, uint64_t glane) {
    s.axis = lane_gen_range(c.key_env, glane, s.env_pos, 10);
    s.element = lane_bool10_at(c.key_env, glane, s.env_pos);
    s.env_pos += 10;
    s.fb_some = 0;
    s.fb_element = 0;
    s.fb_label = 0;
    s.steps_remaining = c.max_steps;
    s.reset_count += 1;
  }
};

// ---------------------------------------------------------------- one step of a lane, recorded
// Environment::step, the step's record, the successor observation of a cut episode, the auto-reset: the rule every
// stepping kernel follows, in this order.  `sink` is the kernel's part — where the record goes:
//   record(action, reward, succ)   the step
//   successor(f)                   the features of the state an Interrupt leaves behind, written BEFORE the reset
// `f` is scratch: the feature registers of the kernel, which has no use for their content across the step; the caller
// forms the features the next step starts from.  Returns `succ`.
// (Three kernels write these lines out over the same `Env`: k_rollout_cartpole with TrajSink, and the two DQN collection
// kernels, whose replay ring records a lane the horizon cuts as an Interrupt while the env carries its episode on and may
// refuse a step — DESIGN.md §25 has the compiler's reasons.)
template <class Env, int D, class Sink>
__device__ __forceinline__ int lane_step(const CartPoleDev &c, typename Env::State &s, int action, uint64_t glane,
                                         uint64_t word, Sink &sink, float (&f)[D]) {
  float reward;
  const int succ = Env::step(c, s, action, glane, word, reward);
  sink.record(action, reward, succ);
  if (succ == RL_SUCC_INTERRUPT) {
    Env::template features<D>(c, s, f);
    sink.successor(f);
  }
  if (succ != RL_SUCC_CONTINUE) Env::reset(c, s, glane);
  return succ;
}

// slot `o` = t * n + lane of a trajectory's time-major planes; `on` false: a thread that follows a lane without storing
// (a group's other threads, lanes past the end)
struct TrajSink {
  const TrajDev &tr;
  size_t o;
  bool on;
  __device__ __forceinline__ void record(int action, float reward, int succ) const {
    if (on) {
      tr.action[o] = (uint8_t)action;
      tr.reward[o] = reward;
      tr.flag[o] = (uint8_t)succ;
    }
  }
  template <int D>
  __device__ __forceinline__ void successor(const float (&f)[D]) const {
    if (on) {
#pragma unroll
      for (int d = 0; d < D; ++d) tr.term_obs[(size_t)d * tr.T * tr.n + o] = f[d];
    }
  }
};

// the env's own step buffers ([n] per field): lane i.  The successor observation goes to its [D][n] buffer; the record is
// held for the kernel, which writes it behind the next observation
struct EnvBufSink {
  float *__restrict__ term_obs;
  uint32_t n, i;
  float reward;
  int succ;
  __device__ __forceinline__ void record(int, float r, int sc) {
    reward = r;
    succ = sc;
  }
  template <int D>
  __device__ __forceinline__ void successor(const float (&f)[D]) const {
#pragma unroll
    for (int d = 0; d < D; ++d) term_obs[(size_t)d * n + i] = f[d];
  }
};
