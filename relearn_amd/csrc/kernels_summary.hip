// kernels_summary.hip — OnlineStepsSummary::push (src/simulation/summary.rs:198-214) for every lane of a pushed
// trajectory, as a streaming segmented reduction over the time-major reward / flag planes.
//
// k_summary_chunks: a workgroup of 256 threads covers Q lane quads x K time chunks (Q * K = 256).  A thread reads 4
// adjacent lanes over C = ceil(T / K) steps (one u32 of flags and one float4 of rewards per step where the lane count
// allows) and reduces its chunk two-pass — sums, then means, then squared residuals, re-reading the chunk (no f64
// divide per step; a constant plane gives exactly sigma = 0) — into
//   - step-reward statistics over its 4 x C steps,
//   - statistics of the episodes that begin and end inside the chunk,
//   - per lane a segment record: the prefix up to and including the first episode end (the whole chunk when none
//     ends), a has-end bit, and the suffix after the last end.
// The Q threads of chunk 0 then walk their lanes' K segment records in time order from the lane's carry (the episode in
// progress), push every episode that ends at a chunk's first end, and write the carry back.  A fixed tree in LDS merges
// the 256 threads' statistics (Chan et al.) into one record per workgroup.
// k_summary_finish: one workgroup merges the workgroup records in workgroup order and adds the result to the
// summary's accumulator.  No atomics: the result depends on the inputs and the lane count only.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "summary.hpp"

namespace {

constexpr uint32_t SUM_THREADS = 256;
constexpr uint32_t SUM_HAS_END = 0x80000000u;

// reward[t][lane] and flag[t][lane] planes
struct PlaneSrc {
  const float *reward;
  const uint8_t *flag;
  uint32_t n;
  int vec;  // n % 4 == 0 and aligned planes: one float4 and one u32 per step and quad
  __device__ void lanes(uint32_t, int) {}
  __device__ void load(uint32_t t, uint32_t lane0, int nvalid, float r[4], uint32_t f[4]) const {
    const size_t o = (size_t)t * n + lane0;
    if (vec) {
      const float4 v = *reinterpret_cast<const float4 *>(reward + o);
      const uint32_t w = *reinterpret_cast<const uint32_t *>(flag + o);
      r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
      for (int j = 0; j < 4; ++j) f[j] = (w >> (8 * j)) & 0xffu;
    } else {
      for (int j = 0; j < 4; ++j) {
        r[j] = j < nvalid ? reward[o + j] : 0.0f;
        f[j] = j < nvalid ? flag[o + j] : 0u;
      }
    }
  }
};

// the last DQN collection: flag[t][lane] plus the reward of the replay record it wrote, ring slot
// (total - T + t) mod C in the uint32 arithmetic of the collecting kernel (replay.hpp ring_write_step)
struct RingSrc {
  const ReplayRec *rec;
  const uint32_t *total;
  const uint8_t *flag;
  uint32_t n, C, T;
  uint32_t base[4];
  __device__ void lanes(uint32_t lane0, int nvalid) {
    for (int j = 0; j < 4; ++j) base[j] = j < nvalid ? total[lane0 + j] - T : 0u;
  }
  __device__ void load(uint32_t t, uint32_t lane0, int nvalid, float r[4], uint32_t f[4]) const {
    for (int j = 0; j < 4; ++j) {
      r[j] = j < nvalid ? rec[(size_t)(lane0 + j) * C + (base[j] + t) % C].reward : 0.0f;
      f[j] = j < nvalid ? flag[(size_t)t * n + lane0 + j] : 0u;
    }
  }
};

// OnlineMeanVariance::push (src/utils/stats.rs:127-134)
__device__ inline void mv_push(rl_mean_variance &s, double v) {
  const double pre = v - s.mean;
  s.count += 1;
  s.mean = s.mean + pre / (double)s.count;
  const double post = v - s.mean;
  s.squared_residual_sum = s.squared_residual_sum + pre * post;
}

__device__ inline void tree_merge(rl_steps_summary *red, uint32_t tid) {
  for (uint32_t s = SUM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = ss_merge(red[tid], red[tid + s]);
    __syncthreads();
  }
}

template <class Src>
__global__ __launch_bounds__(SUM_THREADS) void k_summary_chunks(Src src, uint32_t n, uint32_t T, uint32_t K,
                                                                 uint32_t C, uint64_t *__restrict__ carry_len,
                                                                 double *__restrict__ carry_ret,
                                                                 rl_steps_summary *__restrict__ part) {
  __shared__ rl_steps_summary red[SUM_THREADS];
  __shared__ double pre_ret[SUM_THREADS * 4], suf_ret[SUM_THREADS * 4];
  __shared__ uint32_t pre_len[SUM_THREADS * 4], suf_len[SUM_THREADS * 4];
  const uint32_t tid = threadIdx.x, Q = SUM_THREADS / K;
  const uint32_t qi = tid % Q, chunk = tid / Q;
  const uint64_t lane0_64 = ((uint64_t)blockIdx.x * Q + qi) * 4u;
  const int nvalid = lane0_64 < n ? (int)min<uint64_t>(4u, n - lane0_64) : 0;
  const uint32_t lane0 = nvalid > 0 ? (uint32_t)lane0_64 : 0u;
  const uint32_t t0 = min(chunk * C, T);
  const uint32_t t1 = nvalid > 0 ? min(t0 + C, T) : t0;
  src.lanes(lane0, nvalid);

  // pass 1: sums, segment records
  double step_sum = 0.0, len_sum = 0.0, ret_sum = 0.0;
  uint64_t n_eps = 0;
  uint32_t cur_len[4] = {0, 0, 0, 0}, first_len[4] = {0, 0, 0, 0};
  double cur_ret[4] = {0.0, 0.0, 0.0, 0.0}, first_ret[4] = {0.0, 0.0, 0.0, 0.0};
  bool ended[4] = {false, false, false, false};
  for (uint32_t t = t0; t < t1; ++t) {
    float r[4];
    uint32_t f[4];
    src.load(t, lane0, nvalid, r, f);
    for (int j = 0; j < 4; ++j) {
      if (j >= nvalid) continue;
      const double rv = (double)r[j];
      step_sum += rv;
      cur_len[j] += 1;
      cur_ret[j] += rv;
      if (f[j] != RL_SUCC_CONTINUE) {
        if (ended[j]) {
          n_eps += 1;
          len_sum += (double)cur_len[j];
          ret_sum += cur_ret[j];
        } else {
          first_len[j] = cur_len[j];
          first_ret[j] = cur_ret[j];
          ended[j] = true;
        }
        cur_len[j] = 0;
        cur_ret[j] = 0.0;
      }
    }
  }
  for (int j = 0; j < 4; ++j) {
    const uint32_t i = tid * 4 + j;
    pre_len[i] = ended[j] ? first_len[j] | SUM_HAS_END : cur_len[j];
    pre_ret[i] = ended[j] ? first_ret[j] : cur_ret[j];
    suf_len[i] = ended[j] ? cur_len[j] : 0u;
    suf_ret[i] = ended[j] ? cur_ret[j] : 0.0;
  }

  // pass 2: squared residuals about the chunk's means (the chunk is read again: L2 / MALL hits)
  const uint64_t n_steps = (uint64_t)(t1 - t0) * (uint32_t)max(nvalid, 0);
  const double step_mean = n_steps ? step_sum / (double)n_steps : 0.0;
  const double len_mean = n_eps ? len_sum / (double)n_eps : 0.0;
  const double ret_mean = n_eps ? ret_sum / (double)n_eps : 0.0;
  double step_srs = 0.0, len_srs = 0.0, ret_srs = 0.0;
  for (int j = 0; j < 4; ++j) {
    cur_len[j] = 0;
    cur_ret[j] = 0.0;
    ended[j] = false;
  }
  for (uint32_t t = t0; t < t1; ++t) {
    float r[4];
    uint32_t f[4];
    src.load(t, lane0, nvalid, r, f);
    for (int j = 0; j < 4; ++j) {
      if (j >= nvalid) continue;
      const double rv = (double)r[j];
      const double d = rv - step_mean;
      step_srs += d * d;
      cur_len[j] += 1;
      cur_ret[j] += rv;
      if (f[j] != RL_SUCC_CONTINUE) {
        if (ended[j]) {
          const double dl = (double)cur_len[j] - len_mean, dr = cur_ret[j] - ret_mean;
          len_srs += dl * dl;
          ret_srs += dr * dr;
        }
        ended[j] = true;
        cur_len[j] = 0;
        cur_ret[j] = 0.0;
      }
    }
  }
  rl_steps_summary mine;
  mine.step_reward = rl_mean_variance{step_mean, step_srs, n_steps};
  mine.episode_reward = rl_mean_variance{ret_mean, ret_srs, n_eps};
  mine.episode_length = rl_mean_variance{len_mean, len_srs, n_eps};
  __syncthreads();

  // chunk 0 of every quad: its lanes' chunks in time order from the carry; the episodes that end at a chunk's first end
  if (chunk == 0) {
    rl_mean_variance bl{0.0, 0.0, 0}, br{0.0, 0.0, 0};
    for (int j = 0; j < nvalid; ++j) {
      const uint32_t lane = lane0 + j;
      uint64_t L = carry_len[lane];
      double R = carry_ret[lane];
      for (uint32_t k = 0; k < K; ++k) {
        const uint32_t i = (k * Q + qi) * 4 + j;
        const uint32_t pl = pre_len[i];
        L += pl & ~SUM_HAS_END;
        R += pre_ret[i];
        if (pl & SUM_HAS_END) {
          mv_push(bl, (double)L);
          mv_push(br, R);
          L = suf_len[i];
          R = suf_ret[i];
        }
      }
      carry_len[lane] = L;
      carry_ret[lane] = R;
    }
    mine.episode_length = mv_merge(mine.episode_length, bl);
    mine.episode_reward = mv_merge(mine.episode_reward, br);
  }
  red[tid] = mine;
  __syncthreads();
  tree_merge(red, tid);
  if (tid == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(SUM_THREADS) void k_summary_finish(const rl_steps_summary *__restrict__ part, uint32_t G,
                                                                rl_steps_summary *__restrict__ acc) {
  __shared__ rl_steps_summary red[SUM_THREADS];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (G + SUM_THREADS - 1) / SUM_THREADS;
  const uint32_t lo = min(tid * per, G), hi = min(lo + per, G);
  rl_steps_summary x{};
  for (uint32_t i = lo; i < hi; ++i) x = ss_merge(x, part[i]);
  red[tid] = x;
  __syncthreads();
  tree_merge(red, tid);
  if (tid == 0) *acc = ss_merge(*acc, red[0]);
}

// K (power of two, <= 64) time chunks per lane quad: enough threads to cover the device at small lane counts, chunks of
// at least 4 steps
struct SumPlan {
  uint32_t K, C, G;
};
SumPlan summary_plan(uint64_t n, uint32_t T) {
  const uint64_t quads = (n + 3) / 4;
  uint32_t K = 1;
  while (K < 64 && quads * K < 65536 && (T + 2 * K - 1) / (2 * K) >= 4) K *= 2;
  SumPlan p;
  p.K = K;
  p.C = (T + K - 1) / K;
  const uint32_t Q = SUM_THREADS / K;
  p.G = (uint32_t)((quads + Q - 1) / Q);
  return p;
}

template <class Src>
void launch_summary(rl_summary *s, const Src &src, uint32_t T) {
  if (T == 0 || s->n == 0) return;
  const SumPlan p = summary_plan(s->n, T);
  if (p.G > s->max_groups) throw RlError(RL_ERR_INVALID_ARGUMENT, "summary: workgroup records exceed the workspace");
  hipStream_t st = s->eng->stream;
  hipLaunchKernelGGL(k_summary_chunks<Src>, dim3(p.G), dim3(SUM_THREADS), 0, st, src, (uint32_t)s->n, T, p.K, p.C,
                     s->carry_len, s->carry_ret, s->part);
  hipLaunchKernelGGL(k_summary_finish, dim3(1), dim3(SUM_THREADS), 0, st, s->part, p.G, s->acc);
}

}  // namespace

void launch_summary_planes(rl_summary *s, const float *reward, const uint8_t *flag, uint32_t T) {
  PlaneSrc src;
  src.reward = reward;
  src.flag = flag;
  src.n = (uint32_t)s->n;
  src.vec = s->n % 4 == 0 && ((uintptr_t)reward % 16) == 0 && ((uintptr_t)flag % 4) == 0;
  launch_summary(s, src, T);
}

void launch_summary_replay(rl_summary *s, const ReplayRec *rec, const uint32_t *total, uint32_t C,
                           const uint8_t *flag, uint32_t T) {
  RingSrc src;
  src.rec = rec;
  src.total = total;
  src.flag = flag;
  src.n = (uint32_t)s->n;
  src.C = C;
  src.T = T;
  for (int j = 0; j < 4; ++j) src.base[j] = 0;
  launch_summary(s, src, T);
}
