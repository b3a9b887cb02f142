"""Python restatement of the tabular-MDP lanes and of the host sampler that makes random ones (test infrastructure, not
a test): `TabularMdp<_, Normal<f64>>` (src/envs/mdps.rs:12-85) under the index lanes' step limit, and
`DirichletRandomMdps::sample_environment` (mdps.rs:151-170), as include/relearn_hip.h and include/rl_normal.h state them:

  normal         Marsaglia's polar method, two u64 per attempt, at most 64 attempts, the 64th taken as it is
  gamma          alpha == 1: -ln(open01); alpha > 1: Marsaglia-Tsang without the squeeze; alpha < 1: the boost
  sample_mdp     per (s, a) row-major: S gammas normalised in f64 and cast to f32, then the row's reward mean
  MdpLane        state 0 at a reset (no draw); a step draws one u64 for the successor (always), then the reward's normal
                 unless the row's stddev is 0; the step-limit tail of the index lanes

One stream is one Prng of the oracle's binding (oracle_prng_seed_from_u64, _set_stream, _set_word_pos), consumed
sequentially; rl_log / rl_exp / open01 are tests/thompson_ref.py's transcriptions.  Nothing here shares code with the
library under test."""
import ctypes as C
import math

import numpy as np

import oracle as O
from thompson_ref import open01, rl_exp, rl_log

L = O.lib()
CONTINUE, TERMINATE, INTERRUPT = 0, 1, 2
LIMIT_NONE, LIMIT_LATENT, LIMIT_VISIBLE = 0, 1, 2
MAX_ATTEMPTS = 64
F32 = np.float32


def make_rng(seed, stream, word_pos=0):
    rng = O.Prng()
    L.oracle_prng_seed_from_u64(C.byref(rng), seed)
    L.oracle_prng_set_stream(C.byref(rng), stream)
    L.oracle_prng_set_word_pos(C.byref(rng), word_pos)
    return rng


def next_u64(rng):
    return int(L.oracle_prng_next_u64(C.byref(rng)))


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else float("nan")  # IEEE: correctly rounded; the square root of a negative is a NaN


def normal_attempt(w1, w2):
    """-> (accepted, z)"""
    u = 2.0 * open01(w1) - 1.0
    v = 2.0 * open01(w2) - 1.0
    s = u * u + v * v
    z = u * _sqrt(-2.0 * rl_log(s) / s)
    return not (s >= 1.0 or s == 0.0), z


def normal(rng):
    """-> (z, attempts); 4 words per attempt; at the bound the last attempt's z is taken"""
    z = 0.0
    for attempt in range(MAX_ATTEMPTS):
        w1 = next_u64(rng)
        w2 = next_u64(rng)
        ok, z = normal_attempt(w1, w2)
        if ok:
            break
    return z, attempt + 1


def gamma_ge1(alpha, rng):
    if alpha == 1.0:
        return -rl_log(open01(next_u64(rng)))
    d = alpha - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    g = 0.0
    for _ in range(MAX_ATTEMPTS):
        x, _n = normal(rng)
        u = open01(next_u64(rng))
        t = 1.0 + c * x
        v = t * t * t
        g = d * v
        if v > 0.0 and rl_log(u) < x * x / 2.0 + d - d * v + d * rl_log(v):
            break
    return g


def gamma(alpha, rng):
    """Gamma(alpha, 1), alpha > 0"""
    if alpha < 1.0:
        g = gamma_ge1(alpha + 1.0, rng)
        u = open01(next_u64(rng))
        return g * rl_exp(rl_log(u) / alpha)
    return gamma_ge1(alpha, rng)


def sample_mdp(num_states, num_actions, alpha, prior_mean, prior_stddev, seed, stream):
    """DirichletRandomMdps::sample_environment -> (transitions [S][A][S] f32, reward_mean [S][A] f64)"""
    rng = make_rng(seed, stream)
    S, A = num_states, num_actions
    tr = np.zeros((S, A, S), F32)
    mean = np.zeros((S, A), np.float64)
    for s in range(S):
        for a in range(A):
            g = [gamma(alpha, rng) for _ in range(S)]
            total = 0.0
            for x in g:
                total = total + x
            for j in range(S):
                tr[s, a, j] = F32(g[j] / total)
            z, _n = normal(rng)
            mean[s, a] = prior_mean + prior_stddev * z
    return tr, mean


def cumulative(transitions):
    """the table the lanes read: the f32 running sum of every row in index order; from the row's last successor of
    positive probability on, exactly 1 (no draw reaches 1: a zero-probability successor is never reached)"""
    tr = np.asarray(transitions, F32)
    S, A, _ = tr.shape
    cum = np.zeros_like(tr)
    for s in range(S):
        for a in range(A):
            acc = F32(0.0)
            last = 0
            for j in range(S):
                acc = F32(acc + tr[s, a, j])
                cum[s, a, j] = acc
                if tr[s, a, j] > 0.0:
                    last = j
            cum[s, a, last:] = 1.0
    return cum


def unit_f32(word):
    """rand 0.8 Standard f32 of one 32-bit word: exact in f32 (and in a Python float)"""
    return float(word >> 8) * 5.9604644775390625e-08


def successor(cum_row, u):
    """#{ j < S - 1 : cum[j] <= u }"""
    return sum(1 for j in range(len(cum_row) - 1) if float(cum_row[j]) <= u)


class MdpLane:
    """one lane: state, the word position of its env stream, the step limit"""

    def __init__(self, tables, limit, max_steps, seed_env, global_lane):
        self.cum, self.mean, self.stddev = tables
        self.S = self.cum.shape[0]
        self.limit, self.max_steps = limit, max_steps
        self.seed, self.stream = seed_env, global_lane
        self.rng = make_rng(seed_env, global_lane)
        self.env_pos = 0
        self.reset_count = 0
        self.reset()

    def reset(self):
        self.state = 0  # TabularMdp::initial_state: no draw
        self.remaining = self.max_steps if self.limit != LIMIT_NONE else 0
        self.reset_count += 1

    def set(self, state, env_pos, remaining, reset_count):
        self.state, self.env_pos, self.remaining, self.reset_count = int(state), int(env_pos), int(remaining), int(reset_count)
        self.rng = make_rng(self.seed, self.stream, self.env_pos)

    def obs_features(self):
        D = self.S + (1 if self.limit == LIMIT_VISIBLE else 0)
        f = np.zeros(D, F32)
        f[self.state] = 1.0
        if self.limit == LIMIT_VISIBLE:
            f[D - 1] = F32(float(self.remaining) / float(self.max_steps))
        return f

    def step(self, action):
        """-> (reward f32, successor kind); on Interrupt the lane holds the successor state (observe it, then reset())"""
        s, a = self.state, int(action)
        w = next_u64(self.rng)
        self.env_pos += 2
        self.last_u = unit_f32(w & 0xFFFFFFFF)
        nxt = successor(self.cum[s, a], self.last_u)
        mean, sd = float(self.mean[s, a]), float(self.stddev[s, a])
        r = mean
        if sd != 0.0:
            z, attempts = normal(self.rng)
            self.env_pos += 4 * attempts
            r = mean + sd * z
        self.state = nxt
        kind = CONTINUE
        if self.limit != LIMIT_NONE:
            self.remaining -= 1
            if self.remaining == 0:
                kind = INTERRUPT
        return F32(r), kind


class MdpLanes:
    """n lanes of one MDP stepped the way the library's env handle steps them"""

    def __init__(self, n, transitions, reward_mean, reward_stddev=None, limit=LIMIT_NONE, max_steps=0, lane_offset=0,
                 seed_env=0):
        tr = np.asarray(transitions, F32)
        mean = np.asarray(reward_mean, np.float64)
        sd = np.ones_like(mean) if reward_stddev is None else np.asarray(reward_stddev, np.float64)
        self.n, self.S, self.A = n, tr.shape[0], tr.shape[1]
        self.D = self.S + (1 if limit == LIMIT_VISIBLE else 0)
        tables = (cumulative(tr), mean, sd)
        self.lanes = [MdpLane(tables, limit, max_steps, seed_env, lane_offset + i) for i in range(n)]

    def observe(self):
        return np.stack([lane.obs_features() for lane in self.lanes], axis=1)  # [D][n]

    def state(self):
        """(state, env_pos, steps_remaining, reset_count), each [n]"""
        return tuple(np.array([getattr(lane, k) for lane in self.lanes], np.uint64)
                     for k in ("state", "env_pos", "remaining", "reset_count"))

    def step(self, actions):
        """-> reward [n] f32, flag [n] u8, next observation [D][n], interrupt successor [D][n] (zero where not cut)"""
        reward = np.zeros(self.n, F32)
        flag = np.zeros(self.n, np.uint8)
        term = np.zeros((self.D, self.n), F32)
        for i, lane in enumerate(self.lanes):
            r, f = lane.step(int(actions[i]))
            reward[i], flag[i] = r, f
            if f == INTERRUPT:
                term[:, i] = lane.obs_features()
            if f != CONTINUE:
                lane.reset()
        return reward, flag, self.observe(), term

    def replay(self, actions):
        """actions [T][n] -> a trajectory's planes: obs [D][T+1][n], reward, flag [T][n], term_obs [D][T][n]"""
        T = actions.shape[0]
        obs = np.zeros((self.D, T + 1, self.n), F32)
        term = np.zeros((self.D, T, self.n), F32)
        reward = np.zeros((T, self.n), F32)
        flag = np.zeros((T, self.n), np.uint8)
        obs[:, 0] = self.observe()
        for t in range(T):
            reward[t], flag[t], obs[:, t + 1], term[:, t] = self.step(actions[t])
        return {"obs": obs, "reward": reward, "flag": flag, "term_obs": term}


def finite_horizon_values(transitions, reward_mean, horizon):
    """f64 dynamic programming over `horizon` steps from state 0 -> (optimal, uniform-random) expected episode reward"""
    P = np.asarray(transitions, np.float64)
    R = np.asarray(reward_mean, np.float64)
    v_opt = np.zeros(P.shape[0])
    v_uni = np.zeros(P.shape[0])
    for _ in range(horizon):
        v_opt = (R + P @ v_opt).max(axis=1)
        v_uni = (R + P @ v_uni).mean(axis=1)
    return float(v_opt[0]), float(v_uni[0])
