"""The restatement of the Thompson-sampling baseline (tests/thompson_ref.py) held to facts that do not come from it:
its transcription of rl_log / rl_exp against the compiled header bit for bit on the inputs the sampler forms, its Beta
sampler against the header's compiled one bit for bit (values and words consumed) on ChaCha streams, the sampler's
distribution against the closed-form Beta CDF for integer parameters, the words an agent's pull draws — and the
library's exports, defaults and refusals as far as they go without a GPU.  CPU only."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import meta_lanes_ref as M
import oracle as O
import relearn_amd as ra
import thompson_ref as TR

L = O.lib()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(1, 1), (1, 2), (2, 1), (1, 5), (5, 1), (2, 2), (2, 3), (3, 2), (7, 2), (2, 9), (11, 11), (1, 30), (40, 3)]
PAIR_IDS = ["%d-%d" % p for p in PAIRS]
N_KS = 40000
N_EQUAL = 1500  # samples per pair drawn by the Python restatement as well

PROBE_C = r'''
#include <stdint.h>
#include "include/rl_beta.h"
void probe_exp(const double *x, int n, double *y) { for (int i = 0; i < n; ++i) y[i] = rl_exp(x[i]); }
void probe_log(const double *x, int n, double *y) { for (int i = 0; i < n; ++i) y[i] = rl_log(x[i]); }
/* n samples of Beta(alpha, beta) from the stream (seed, stream) at word 0; pos[i] = the word position after sample i */
void probe_beta(double alpha, double beta, uint64_t seed, uint64_t stream, int n, double *x, uint64_t *pos) {
  uint32_t key[8];
  rl_beta p;
  uint64_t at = 0;
  rl_seed_from_u64(seed, key);
  rl_beta_new(alpha, beta, &p);
  for (int i = 0; i < n; ++i) {
    x[i] = rl_beta_sample(&p, key, stream, &at);
    pos[i] = at;
  }
}
void probe_beta_new(double alpha, double beta, double *out) {
  rl_beta p;
  rl_beta_new(alpha, beta, &p);
  out[0] = p.a; out[1] = p.b; out[2] = p.A; out[3] = p.B; out[4] = p.G; out[5] = p.kappa1; out[6] = p.kappa2;
  out[7] = (double)p.bb; out[8] = (double)p.switched;
}
'''


@pytest.fixture(scope="module")
def probe():
    d = tempfile.mkdtemp()
    src = os.path.join(d, "probe.c")
    open(src, "w").write(PROBE_C)
    so = os.path.join(d, "probe.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c99", "-pedantic", "-Wall",
                           "-Wextra", "-Werror", "-I", ROOT, src, "-o", so, "-lm"])
    return C.CDLL(so)


def apply(fn, x):
    x = np.ascontiguousarray(x, np.float64)
    y = np.zeros_like(x)
    fn(x.ctypes.data_as(C.c_void_p), len(x), y.ctypes.data_as(C.c_void_p))
    return y


def c_samples(probe, alpha, beta, seed, stream, n):
    x, pos = np.zeros(n), np.zeros(n, np.uint64)
    probe.probe_beta(C.c_double(alpha), C.c_double(beta), C.c_uint64(seed), C.c_uint64(stream), n,
                     x.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p))
    return x, pos


@pytest.fixture(scope="module")
def drawn(probe):
    """per pair: N_KS samples of the compiled sampler and the word position after each — computed once, shared"""
    return {p: c_samples(probe, float(p[0]), float(p[1]), 100 + i, 7 + i, N_KS) for i, p in enumerate(PAIRS)}


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ------------------------------------------------------------------------------------------------ the transcription
def test_transcription_of_log_and_exp_equals_the_header(probe):
    """more than 1e5 inputs, formed as the sampler forms them: u / (1 - u), u1^2 u2, A / (b + w), v in +-40 — and the
    special values"""
    rng = np.random.default_rng(21)
    n = 30000
    words = rng.integers(0, 1 << 64, size=(3, n), dtype=np.uint64)
    u1, u2, u3 = (np.array([TR.open01(int(w)) for w in row]) for row in words)
    v = rng.uniform(-40.0, 40.0, n)
    w = np.array([TR.rl_exp(t) for t in v])
    A = rng.integers(2, 60, n).astype(np.float64)
    b = rng.integers(1, 40, n).astype(np.float64)
    log_in = np.concatenate([u1 / (1.0 - u1), u1 * u1 * u2, A / (b + w), u3,
                             [0.0, -0.0, -1.0, np.inf, np.nan, 1.0, 5e-324, 4.0, 5.0]])
    exp_in = np.concatenate([v, rng.uniform(-745.0, 709.0, n), np.log(u1 / (1.0 - u1)) * rng.uniform(0.02, 1.0, n),
                             [np.nan, np.inf, -np.inf, 0.0, -0.0, 710.0, -746.0, -740.0]])
    assert len(log_in) + len(exp_in) >= 100000
    assert same_bits(apply(probe.probe_log, log_in), [TR.rl_log(float(t)) for t in log_in])
    assert same_bits(apply(probe.probe_exp, exp_in), [TR.rl_exp(float(t)) for t in exp_in])
    assert same_bits(apply(probe.probe_exp, v), w)
    assert same_bits([TR.LN4, TR.LN5], apply(probe.probe_log, [4.0, 5.0]))


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_parameters_equal_the_header(probe, pair):
    out = np.zeros(9)
    probe.probe_beta_new(C.c_double(pair[0]), C.c_double(pair[1]), out.ctypes.data_as(C.c_void_p))
    b = TR.Beta(float(pair[0]), float(pair[1]))
    assert b.bb == (min(pair) > 1) and out[7] == float(b.bb) and out[8] == float(b.switched)
    assert same_bits(out[:4], [b.a, b.b, b.A, b.B])
    if b.bb:
        assert same_bits(out[4], b.G)
    else:
        assert same_bits(out[5:7], [b.kappa1, b.kappa2])
        assert b.a >= b.b and b.switched == (pair[0] < pair[1])  # BC: a is the larger parameter
    if b.bb:
        assert b.a <= b.b and b.switched == (pair[0] >= pair[1])


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_sampler_equals_the_header_bit_for_bit(drawn, pair):
    """values and words consumed, sample by sample; words per sample = 4 x attempts; the bound is not reached"""
    x, pos = drawn[pair]
    i = PAIRS.index(pair)
    rng = O.Prng()
    L.oracle_prng_seed_from_u64(C.byref(rng), 100 + i)
    L.oracle_prng_set_stream(C.byref(rng), 7 + i)
    L.oracle_prng_set_word_pos(C.byref(rng), 0)
    beta = TR.Beta(float(pair[0]), float(pair[1]))
    before = 0
    for j in range(N_EQUAL):
        got, attempts = beta.sample(C.byref(rng))
        after = int(L.oracle_prng_word_pos(C.byref(rng)))
        assert TR.bits(got) == TR.bits(float(x[j])) and after == int(pos[j]), j
        assert after - before == 4 * attempts and attempts < TR.MAX_ATTEMPTS
        before = after


def beta_cdf(x, a, b):
    """I_x(a, b) for integer a, b: sum_{j=a}^{a+b-1} C(a+b-1, j) x^j (1-x)^(a+b-1-j)"""
    m = a + b - 1
    return sum(math.comb(m, j) * x ** j * (1.0 - x) ** (m - j) for j in range(a, m + 1))


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_kolmogorov_smirnov_against_the_closed_form(drawn, pair):
    """N = 40,000 samples of the compiled sampler (the restatement's, by the test above) against I_x(a, b): D below
    1.95 / sqrt(N), the 0.1 % critical value; deterministic at the fixed seed.  A wrong constant or a missed switch of
    the parameters gives D > 0.05"""
    x, pos = drawn[pair]
    assert np.all(x > 0.0) and np.all(x < 1.0)
    xs = np.sort(x)
    cdf = beta_cdf(xs, *pair)
    n = len(xs)
    D = max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(0, n) / n))
    words = np.diff(np.concatenate([[0], pos.astype(np.int64)]))
    print("Beta(%d, %d): D = %.4f, %.3f attempts per sample, most %d" % (pair + (D, words.mean() / 4, words.max() // 4)))
    assert D < 1.95 / math.sqrt(n)
    assert np.all(words % 4 == 0) and words.min() >= 4
    assert words.max() < 4 * TR.MAX_ATTEMPTS  # no sample reached the bound
    assert words.mean() / 4 < 1.6


def test_a_missed_switch_is_seen(drawn):
    """the bar's power, on data: the samples of Beta(7, 2) against the CDF of Beta(2, 7) are far off"""
    xs = np.sort(drawn[(7, 2)][0])
    n = len(xs)
    assert np.max(np.abs(np.arange(1, n + 1) / n - beta_cdf(xs, 2, 7))) > 0.05


# ------------------------------------------------------------------------------------------------ the agent
@pytest.mark.parametrize("k", [2, 3, 4])
def test_words_of_a_fresh_agents_pull(k):
    """counts (1, 1) on every arm, num_samples 1: a pull draws k samples, so at least 4 k words, 4 per attempt"""
    agents = TR.ThompsonAgentLanes(6, k, 1, seed_actor=10)
    env = M.MetaLanes(6, k, 5, M.UNIFORM_BERNOULLI, seed_env=9)
    planes = agents.rollout(env, 1)
    st = agents.state()
    assert np.all(st["pos"] >= 4 * k) and np.all(st["pos"] % 4 == 0)
    assert list(st["pos"]) == [4 * a.attempts for a in agents.inner]
    # the one pull counted on its side of 0.5
    hit = planes["reward"][0] > 0.5
    assert np.array_equal(st["high"].sum(axis=0), k + hit) and np.array_equal(st["low"].sum(axis=0), k + ~hit)


def test_more_samples_more_words_and_a_trial_restarts_the_counts():
    n, k, E = 4, 3, 4
    agents = TR.ThompsonAgentLanes(n, k, 10, seed_actor=11)
    env = M.MetaLanes(n, k, E, M.ONE_HOT, seed_env=12)
    planes = agents.rollout(env, 2 * E - 1)  # one whole trial
    assert np.all(planes["flag"][-1] == M.INTERRUPT) and np.all(planes["action"][1::2] == 0)
    st = agents.state()
    assert np.all(st["pos"] >= 4 * 10 * k * E)
    assert np.all(st["low"].sum(axis=0) + st["high"].sum(axis=0) == 2 * k + E)  # E pulls counted
    agents.rollout(env, 1)  # the next trial's first pull: a fresh agent, one pull counted
    st = agents.state()
    assert np.all(st["low"].sum(axis=0) + st["high"].sum(axis=0) == 2 * k + 1)


def test_last_maximal_sum_wins(monkeypatch):
    """act on given samples (exact binary fractions): sums 0.0 + x1 + x2 per arm in arm order, the LAST maximum"""
    for samples, want in (([0.25, 0.25, 0.5, 0.0, 0.125, 0.125], 1), ([0.5, 0.25, 0.25, 0.5, 0.75, 0.0], 2),
                          ([0.5, 0.5, 0.25, 0.5, 0.75, 0.0], 0)):
        seq = iter(samples)
        monkeypatch.setattr(TR.Beta, "sample", lambda self, rng: (next(seq), 1))
        agent = TR.ThompsonInner(3, 2)
        assert agent.act(None) == want and agent.attempts == 6


# ------------------------------------------------------------------------------------------------ the library, no GPU
def test_library_exports_and_defaults():
    ra.build()
    lib = ra.lib()
    assert ra.BANDIT_AGENT_THOMPSON == 4 and ra.BANDIT_AGENT_KINDS["thompson"] == 4
    assert (ra.BANDIT_STATE_LOW_COUNTS, ra.BANDIT_STATE_HIGH_COUNTS) == (5, 6)
    t = ra.bandit_agent_config_default("thompson")  # BetaThompsonSamplingAgentConfig::default: num_samples 1
    assert (t.kind, t.reserved, t.exploration_rate, t.initial_action_count, t.initial_action_value) == (4, 0, 0.0, 1, 0.0)
    cfg = ra.BanditAgentConfig()
    assert lib.rl_bandit_agent_config_default(C.c_int32(4), C.byref(cfg)) == ra.OK and cfg.kind == 4
    for bad in (3, 5, -1):  # 3 stays unassigned
        assert lib.rl_bandit_agent_config_default(C.c_int32(bad), C.byref(cfg)) == ra.ERR_INVALID_ARGUMENT
        assert b"unknown kind" in lib.rl_last_error(None)
    assert lib.rl_bandit_agent_config_default(C.c_int32(4), None) == ra.ERR_INVALID_ARGUMENT
    h = C.c_void_p()
    assert lib.rl_bandit_agent_create(None, C.byref(t), C.byref(h)) == ra.ERR_INVALID_ARGUMENT


def test_headers_compile_as_c99():
    """the three contract headers the sampler spans, as strict C99"""
    src = os.path.join(tempfile.mkdtemp(), "h.c")
    open(src, "w").write('#include "include/rl_beta.h"\n#include "include/relearn_hip.h"\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", ROOT,
                           "-fsyntax-only", src])
