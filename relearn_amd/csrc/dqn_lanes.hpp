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
//   if rng.gen_bool(eps) { action_space.sample(rng) = gen_range(0..A) } else { argmax_a Q(obs)[a] }
// The draws are here, and the rule of the greedy branch (first_max_index); the action values are the kernel's.
template <class Rng>
__device__ __forceinline__ bool dqn_explores(Rng &rng, uint64_t p_int, int always_explore) {
  bool explore = always_explore != 0;
  if (!explore) explore = rl_bernoulli_from_u64(rng.next_u64(), p_int) != 0;  // Bernoulli::sample (rl_chacha.h)
  return explore;
}
template <int A, class Rng>
__device__ __forceinline__ int dqn_random_action(Rng &rng) {
  // FiniteSpace::sample = gen_range(0..A): UniformInt::sample_single(0, A) of rand 0.8.5 for u64 — a widening multiply
  // by A, accepted when the low half is within zone = (A << A.leading_zeros()) - 1, else the next word (lane_gen_range,
  // env_lanes.hpp, is this rule on the env stream).  A = 2: lo = v << 1, hi = v >> 63, zone = (2 << 62) - 1.
  static_assert(A >= 2 && A <= 8, "finite action spaces of 2..8 actions");
  constexpr uint64_t range = (uint64_t)A;
  constexpr uint64_t zone = (range << __builtin_clzll(range)) - 1;
  for (;;) {
    const uint64_t v = rng.next_u64();
    uint64_t lo, hi;
    if constexpr ((range & (range - 1)) == 0) {  // a power of two: the product's halves are shifts (A = 2: the code as it was)
      constexpr int sh = __builtin_ctzll(range);
      lo = v << sh, hi = v >> (64 - sh);
    } else {
      lo = v * range, hi = __umul64hi(v, range);
    }
    if (lo <= zone) return (int)hi;
  }
}

// argmax(-1) of A action values: the first maximal index (a later value replaces the choice only when strictly larger),
// and amax(-1) with it.  An unrolled compare-select chain: nothing is indexed dynamically.  A = 2: `z[1] > z[0] ? 1 : 0`
// and `z[1] > z[0] ? z[1] : z[0]`.
template <int A>
__device__ __forceinline__ int first_max_index(const float (&z)[A], float &zmax) {
  int best = 0;
  zmax = z[0];
#pragma unroll
  for (int a = 1; a < A; ++a) {
    const bool up = z[a] > zmax;
    best = up ? a : best;
    zmax = up ? z[a] : zmax;
  }
  return best;
}
template <int A>
__device__ __forceinline__ int first_max_index(const float (&z)[A]) {
  float zmax;
  return first_max_index<A>(z, zmax);
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
