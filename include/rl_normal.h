/* rl_normal.h — the engine's standard-normal and Gamma(alpha, 1) samplers, shared by the kernels, host callers and the
 * tests.
 *
 * Part of the published contract of the relearn-mi355x C ABI (include/relearn_hip.h): the tabular-MDP lanes
 * (rl_env_create_tabular_mdp; src/envs/mdps.rs:73-84 draws `Normal<f64>::sample`) draw their rewards, and
 * rl_random_mdps_sample (DirichletRandomMdps::sample_environment, mdps.rs:151-170) its Dirichlet rows and reward means,
 * with exactly these functions, so a host caller reproduces a lane's rewards from (seed, lane, word position) alone.
 *
 * Provenance.  The reference samples with `rand_distr` 0.4.3 (ziggurat normals, alias tables), whose source is not part
 * of this project's inputs.  What is stated here is a BUILD-DEFINED sampler, as rl_beta.h is: the same distributions, not
 * the crate's bits.
 *
 * Standard normal, Marsaglia's polar method.  One attempt takes two u64 of the stream (two words each, low word first):
 *   u = 2 open01(first) - 1;  v = 2 open01(second) - 1;  s = u u + v v
 *   reject when s >= 1 or s == 0;  otherwise z = u sqrt(-2 ln(s) / s)      (the second variate, v ..., is discarded)
 * open01 = rl_u64_to_open01_f64: an odd multiple of 2^-53, so u and v are odd multiples of 2^-52 and s == 0 cannot occur
 * (the test is kept: it is the method's).  The loop is BOUNDED: after RL_NORMAL_MAX_ATTEMPTS = 64 attempts the last
 * attempt's z is taken as it is, accepted or not.  That value comes from s >= 1: for s == 1 it is u * sqrt(-0.0) = a zero,
 * for s > 1 the square root of a negative number, a NaN.  An attempt rejects with probability 1 - pi / 4 = 0.2146, so the
 * bound is reached with probability 1.7e-43 per sample.  A sample consumes 4 x attempts words.
 *
 * Gamma(alpha, 1), alpha > 0:
 *   alpha == 1   -ln(open01(one u64))                                                                     2 words
 *   alpha > 1    Marsaglia-Tsang without the squeeze: d = alpha - 1/3, c = 1 / sqrt(9 d); one attempt draws a normal x
 *                (above), then one u64 for u = open01; v = (1 + c x)^3; accept when v > 0 and
 *                ln(u) < x x / 2 + d - d v + d ln(v); the sample is d v.  Bounded likewise: the 64th attempt's d v is
 *                taken as it is (it may then be negative, or NaN where the normal was).
 *   alpha < 1    Gamma(alpha + 1) * exp(ln(open01(one u64)) / alpha): the Gamma first, then the u64
 *
 * C99, integer and IEEE +,-,*,/ and sqrt only over rl_log / rl_exp; no FMA, no trigonometry; built with
 * -ffp-contract=off everywhere.
 */
#ifndef RL_NORMAL_H
#define RL_NORMAL_H

#include <stdint.h>

#include "rl_chacha.h"
#include "rl_detmath.h"

#define RL_NORMAL_MAX_ATTEMPTS 64

/* the u64 at even word position `pos` of the ChaCha8 stream (key, stream).  The plain form for host callers: one block
 * function per u64.  The kernels select the pair without indexing the block (lane_u64_at, env_lanes.hpp). */
RL_HD uint64_t rl_normal_u64_at(const uint32_t key[8], uint64_t stream, uint64_t pos) {
  uint32_t blk[16];
  rl_chacha_block(key, pos >> 4, stream, 4, blk);
  return ((uint64_t)blk[(pos & 15) + 1] << 32) | blk[pos & 15];
}

/* One attempt of the polar method: writes z, returns 1 when it is accepted. */
RL_HD int rl_normal_attempt(uint64_t w1, uint64_t w2, double *z_out) {
  const double u = 2.0 * rl_u64_to_open01_f64(w1) - 1.0;
  const double v = 2.0 * rl_u64_to_open01_f64(w2) - 1.0;
  const double s = u * u + v * v;
  *z_out = u * __builtin_sqrt(-2.0 * rl_log(s) / s);
  return !(s >= 1.0 || s == 0.0);
}

/* One standard normal from the stream at word `*pos` (even), which advances by 4 per attempt. */
RL_HD double rl_normal_sample(const uint32_t key[8], uint64_t stream, uint64_t *pos) {
  double z = 0.0;
  for (int attempt = 0; attempt < RL_NORMAL_MAX_ATTEMPTS; ++attempt) {
    const uint64_t w1 = rl_normal_u64_at(key, stream, *pos);
    const uint64_t w2 = rl_normal_u64_at(key, stream, *pos + 2);
    *pos += 4;
    if (rl_normal_attempt(w1, w2, &z)) break;
  }
  return z;
}

/* One attempt of Marsaglia-Tsang for shape d + 1/3 > 1: writes d v, returns 1 when it is accepted. */
RL_HD int rl_gamma_attempt(double d, double c, double x, double u, double *g_out) {
  const double t = 1.0 + c * x;
  const double v = t * t * t;
  *g_out = d * v;
  if (!(v > 0.0)) return 0;
  return rl_log(u) < x * x / 2.0 + d - d * v + d * rl_log(v);
}

/* Gamma(alpha, 1) for alpha >= 1 */
RL_HD double rl_gamma_sample_ge1(double alpha, const uint32_t key[8], uint64_t stream, uint64_t *pos) {
  if (alpha == 1.0) {
    const double u = rl_u64_to_open01_f64(rl_normal_u64_at(key, stream, *pos));
    *pos += 2;
    return -rl_log(u);
  }
  const double d = alpha - 1.0 / 3.0;
  const double c = 1.0 / __builtin_sqrt(9.0 * d);
  double g = 0.0;
  for (int attempt = 0; attempt < RL_NORMAL_MAX_ATTEMPTS; ++attempt) {
    const double x = rl_normal_sample(key, stream, pos);
    const double u = rl_u64_to_open01_f64(rl_normal_u64_at(key, stream, *pos));
    *pos += 2;
    if (rl_gamma_attempt(d, c, x, u, &g)) break;
  }
  return g;
}

/* Gamma(alpha, 1), alpha > 0 */
RL_HD double rl_gamma_sample(double alpha, const uint32_t key[8], uint64_t stream, uint64_t *pos) {
  if (alpha < 1.0) {
    const double g = rl_gamma_sample_ge1(alpha + 1.0, key, stream, pos);
    const double u = rl_u64_to_open01_f64(rl_normal_u64_at(key, stream, *pos));
    *pos += 2;
    return g * rl_exp(rl_log(u) / alpha);
  }
  return rl_gamma_sample_ge1(alpha, key, stream, pos);
}

/* A Dirichlet row from its S Gamma draws and their f64 sum (DirichletRandomMdps::sample_environment, mdps.rs:151-170):
 * p[j] = (float)(g[j] / sum).  `cap` >= S bounds the loop: a kernel gives a constant, so that the loop unrolls and the
 * arrays stay in registers; a host caller gives S.  Entries at and behind S are not touched. */
RL_HD void rl_dirichlet_row_normalise(const double *g, double sum, uint32_t S, uint32_t cap, float *p) {
  for (uint32_t j = 0; j < cap; ++j)
    if (j < S) p[j] = (float)(g[j] / sum);
}

/* The f32 running sums of a successor row as the tabular-MDP lanes read them (relearn::TabularMdp, rl_env_create_tabular_mdp
 * and the lanes of rl_env_create_meta_mdp): cum[j] = p[0] + .. + p[j] in index order, and from the row's last successor of
 * positive probability on (a row without one: from 0 on) the entries are exactly 1 — no draw reaches 1, so the rounding of
 * the running sum opens no bucket behind that successor.  `cap` as above. */
RL_HD void rl_mdp_row_cumulative(const float *p, uint32_t S, uint32_t cap, float *cum) {
  float acc = 0.0f;
  for (uint32_t j = 0; j < cap; ++j)
    if (j < S) {
      acc = acc + p[j];
      cum[j] = acc;
    }
  int tail = 1; /* no successor of positive probability behind this one */
  for (uint32_t j = cap; j-- > 0;)
    if (j < S) {
      if (tail) cum[j] = 1.0f;
      if (p[j] > 0.0f) tail = 0;
    }
}

#endif /* RL_NORMAL_H */
