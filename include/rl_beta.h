/* rl_beta.h — the engine's Beta(alpha, beta) sampler, shared by the kernels, host callers and the tests.
 *
 * Part of the published contract of the relearn-mi355x C ABI (include/relearn_hip.h): the Thompson-sampling baseline
 * (RL_BANDIT_AGENT_THOMPSON; src/agents/bandits/thompson_sampling.rs:186-205 draws `Beta::new(high, low).sample(rng)`)
 * draws its posterior samples with exactly these functions, so a host caller reproduces a lane's actions from
 * (seed, lane, word position) alone.
 *
 * Provenance.  The reference samples with `rand_distr` 0.4.3 (relearn_experiments/Cargo.lock), whose source is not part
 * of this project's inputs.  What is stated here is a BUILD-DEFINED sampler, as the Prng stream layout is: Cheng's
 * 1978 algorithms BB (min(alpha, beta) > 1) and BC (otherwise) in the operation order that, to the best of the
 * project's knowledge, is the crate's.  Bit-equality with the crate is CONDITIONAL on a check against its source, and
 * even then holds only up to ln / exp: the crate calls the platform's `f64::ln` / `f64::exp`, so the reference itself
 * is not reproducible across libms; here both are rl_log / rl_exp (rl_detmath.h), the same bits on host and device.
 *
 * Beta::new(alpha, beta), all f64:
 *   (a, b, switched) = alpha < beta ? (alpha, beta, false) : (beta, alpha, true)
 *   a > 1.0  -> BB: A = a + b; B = sqrt((A - 2) / (2 a b - A)); G = a + 1 / B
 *   else     -> BC: (a, b, switched) = (b, a, !switched); A = a + b; B = 1 / b; delta = 1 + a - b;
 *                   kappa1 = delta (1/18/4 + 3/18/4 b) / (a B - 14/18); kappa2 = 0.25 + (0.5 + 0.25 / delta) b
 *               (the constants are the doubles of those literal expressions, evaluated left to right)
 * One attempt takes u1, then u2, each rl_u64_to_open01_f64 of one u64 of the stream (two words, low word first), and
 * starts, in both algorithms, with v = B ln(u1 / (1 - u1)); w = a exp(v)  (a pure function of u1: an attempt that
 * rejects before it would need them has the same outcome).
 *   BB: z = u1 u1 u2; r = G v - LN4; s = a + r - w; accept if s + 1 + LN5 >= 5 z; else t = ln z, accept if s >= t;
 *       else accept unless r + A ln(A / (b + w)) < t
 *   BC: u1 < 0.5: y = u1 u2; z = u1 y; reject if 0.25 u2 + z - y >= kappa1
 *       else:     z = u1 u1 u2; accept if z <= 0.25; reject if z >= kappa2
 *       then:     accept unless A (ln(A / (b + w)) + v) - LN4 < ln z
 * The sample of an accepted w: switched ? b / (b + w) : (w == inf ? 1.0 : w / (b + w)).
 * The rejection loop is BOUNDED: after RL_BETA_MAX_ATTEMPTS = 64 attempts the last attempt's w is taken whether it was
 * accepted or not (no kernel spins on data).  That is part of the definition; at 1.0 to 1.45 attempts per sample for
 * the integer parameters an agent's counts give, the bound is reached with probability below 1e-20 per sample.
 * A sample therefore consumes 4 x attempts words.
 *
 * C99, integer and IEEE +,-,*,/ and sqrt only; built with -ffp-contract=off everywhere.
 */
#ifndef RL_BETA_H
#define RL_BETA_H

#include <stdint.h>

#include "rl_chacha.h"
#include "rl_detmath.h"

#define RL_BETA_MAX_ATTEMPTS 64
#define RL_BETA_LN4 1.3862943611198906 /* rl_log(4.0), bits 0x3ff62e42fefa39ef (tests/test_detmath_f64.py) */
#define RL_BETA_LN5 1.6094379124341003 /* rl_log(5.0), bits 0x3ff9c041f7ed8d33 */

typedef struct {
  double a, b;           /* after the switches */
  double A, B;           /* alpha + beta; BB: the sqrt term, BC: 1 / b */
  double G;              /* BB: a + 1 / B */
  double kappa1, kappa2; /* BC */
  int32_t bb;            /* 1: algorithm BB, 0: BC */
  int32_t switched;
} rl_beta;

RL_HD void rl_beta_new(double alpha, double beta, rl_beta *p) {
  double a = alpha < beta ? alpha : beta;
  double b = alpha < beta ? beta : alpha;
  int32_t switched = alpha < beta ? 0 : 1;
  p->G = 0.0;
  p->kappa1 = 0.0;
  p->kappa2 = 0.0;
  if (a > 1.0) {
    p->bb = 1;
    p->A = a + b;
    p->B = __builtin_sqrt((p->A - 2.0) / (2.0 * a * b - p->A));
    p->G = a + 1.0 / p->B;
  } else {
    const double t = a;
    a = b;
    b = t;
    switched = !switched;
    p->bb = 0;
    p->A = a + b;
    p->B = 1.0 / b;
    const double delta = 1.0 + a - b;
    p->kappa1 = delta * (1.0 / 18.0 / 4.0 + 3.0 / 18.0 / 4.0 * b) / (a * p->B - 14.0 / 18.0);
    p->kappa2 = 0.25 + (0.5 + 0.25 / delta) * b;
  }
  p->a = a;
  p->b = b;
  p->switched = switched;
}

/* One attempt: writes w, returns 1 when it is accepted. */
RL_HD int rl_beta_attempt(const rl_beta *p, double u1, double u2, double *w_out) {
  const double v = p->B * rl_log(u1 / (1.0 - u1));
  const double w = p->a * rl_exp(v);
  *w_out = w;
  double z;
  if (p->bb) {
    z = u1 * u1 * u2;
    const double r = p->G * v - RL_BETA_LN4;
    const double s = p->a + r - w;
    if (s + 1.0 + RL_BETA_LN5 >= 5.0 * z) return 1;
    const double t = rl_log(z);
    if (s >= t) return 1;
    return !(r + p->A * rl_log(p->A / (p->b + w)) < t);
  }
  if (u1 < 0.5) {
    const double y = u1 * u2;
    z = u1 * y;
    if (0.25 * u2 + z - y >= p->kappa1) return 0;
  } else {
    z = u1 * u1 * u2;
    if (z <= 0.25) return 1;
    if (z >= p->kappa2) return 0;
  }
  return !(p->A * (rl_log(p->A / (p->b + w)) + v) - RL_BETA_LN4 < rl_log(z));
}

RL_HD double rl_beta_result(const rl_beta *p, double w) {
  if (p->switched) return p->b / (p->b + w);
  return w == rl_f64_from_bits(0x7ff0000000000000ULL) ? 1.0 : w / (p->b + w);
}

/* One sample from the ChaCha8 stream (key, stream) at word `*pos` (even), which advances by 4 per attempt.  The plain
 * form for host callers: one block function per u64.  The kernels keep the current block (kernels_bandit_agent.hip). */
RL_HD uint64_t rl_beta_u64_at(const uint32_t key[8], uint64_t stream, uint64_t pos) {
  uint32_t blk[16];
  rl_chacha_block(key, pos >> 4, stream, 4, blk);
  return ((uint64_t)blk[(pos & 15) + 1] << 32) | blk[pos & 15];
}

RL_HD double rl_beta_sample(const rl_beta *p, const uint32_t key[8], uint64_t stream, uint64_t *pos) {
  double w = 0.0;
  for (int attempt = 0; attempt < RL_BETA_MAX_ATTEMPTS; ++attempt) {
    const double u1 = rl_u64_to_open01_f64(rl_beta_u64_at(key, stream, *pos));
    const double u2 = rl_u64_to_open01_f64(rl_beta_u64_at(key, stream, *pos + 2));
    *pos += 4;
    if (rl_beta_attempt(p, u1, u2, &w)) break;
  }
  return rl_beta_result(p, w);
}

#endif /* RL_BETA_H */
