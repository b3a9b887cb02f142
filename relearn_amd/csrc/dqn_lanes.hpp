// dqn_lanes.hpp — what the DQN collection kernels share (device code only): the replay store's step record, the actor's
// two draws, and the lane's episode table.  kernels_dqn.hip (feed-forward action-value modules) and kernels_seq_stack.hip
// (recurrent ones, k_stack_collect_dqn) are written over these lines.
#pragma once

#include "env_lanes.hpp"
#include "replay.hpp"

// one step record: two 16-byte accesses
__device__ __forceinline__ ReplayRec rec_load(const ReplayRec *__restrict__ p) {
  const uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1];
  ReplayRec r;
  r.x[0] = __uint_as_float(a.x), r.x[1] = __uint_as_float(a.y), r.x[2] = __uint_as_float(a.z), r.x[3] = __uint_as_float(a.w);
  r.x[4] = __uint_as_float(b.x), r.reward = __uint_as_float(b.y), r.af = b.z, r.pad = b.w;
  return r;
}
__device__ __forceinline__ void rec_store(ReplayRec *__restrict__ p, const ReplayRec &r) {
  reinterpret_cast<uint4 *>(p)[0] = make_uint4(__float_as_uint(r.x[0]), __float_as_uint(r.x[1]), __float_as_uint(r.x[2]),
                                               __float_as_uint(r.x[3]));
  reinterpret_cast<uint4 *>(p)[1] = make_uint4(__float_as_uint(r.x[4]), __float_as_uint(r.reward), r.af, 0u);
}

// features 5..D of the step at record index `o` (observations wider than the record: ReplayDev::hi), one 16-byte load
template <int D>
__device__ __forceinline__ void rec_load_hi(const ReplayDev &rp, size_t o, float (&x)[D]) {
  static_assert(D > 5 && D <= 8, "the second record array holds features 5, 6 and 7");
  const float4 h = rp.hi[o];
  x[5] = h.x;
  if (D > 6) x[D > 6 ? 6 : 0] = h.y;
  if (D > 7) x[D > 7 ? 7 : 0] = h.z;
}

// DqnActor::act (dqn.rs:360-379) from the lane's sequential actor stream:
//   if rng.gen_bool(eps) { action_space.sample(rng) = gen_range(0..2) } else { argmax_a Q(obs)[a] }
// The draws are here; the greedy branch is the kernel's (the first maximal index of its action values).
template <class Rng>
__device__ __forceinline__ bool dqn_explores(Rng &rng, uint64_t p_int, int always_explore) {
  bool explore = always_explore != 0;
  if (!explore) explore = rl_bernoulli_from_u64(rng.next_u64(), p_int) != 0;  // Bernoulli::sample (rl_chacha.h)
  return explore;
}
template <class Rng>
__device__ __forceinline__ int dqn_random_action(Rng &rng) {
  // UniformInt::sample_single(0, 2): widening multiply by 2, zone = (2 << 62) - 1
  for (;;) {
    const uint64_t v = rng.next_u64();
    const uint64_t lo = v << 1, hi = v >> 63;
    if (lo <= 0x7fffffffffffffffull) return (int)hi;
  }
}

// the lane's episode table; `writer` false: a thread that follows the lane (it reads the table, the lane's writer writes)
struct LaneEpEnds {
  uint32_t *base;
  uint32_t N, lane;
  bool writer;
  __device__ uint32_t get(uint32_t k) const { return base[(size_t)k * N + lane]; }
  __device__ void set(uint32_t k, uint32_t v) {
    if (writer) base[(size_t)k * N + lane] = v;
  }
};
