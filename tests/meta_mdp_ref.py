"""Python restatement of the meta-MDP lanes (test infrastructure, not a test):
`MetaEnv::new(DirichletRandomMdps{..}.wrap(LatentStepLimit::new(L))).wrap(TrialEpisodeLimit::new(E))` of
src/envs/meta.rs:128-203, 541-617 over src/envs/mdps.rs:12-171 and wrappers/step_limit.rs:13-89, as
include/relearn_hip.h states it (rl_env_create_meta_mdp).

One lane is one env Prng of the oracle's binding — seed_from_u64(seed_env), set_stream(global lane) — consumed in the order
the reference's calls consume it: sample_environment at a trial's start (tests/tabular_mdp_ref.py's gamma and normal, per
(s, a) row-major: S gammas, then the mean's normal, always), per live step one u64 for the successor and, unless the
reward stddev is 0, the reward's normal.  The samplers are tests/tabular_mdp_ref.py's, imported unchanged.

The closed loop (`rollout`) is built as tests/seq_multi_ref.py's meta_rollout is: logits from the oracle's teacher-forced C
forward over the prefix, the action from oracle_log_softmax_f32 / oracle_categorical_sample_u at word period * T + t of
the lane's actor stream, the env from the lanes here.  Nothing here shares code with the library under test.

DRIVEN and CLOSED hold the cases that tests/test_meta_mdp_ref.py (their own conditions, no device) and the GPU tests
(the device against them) share; the references are computed once per process and left unchanged."""
import collections
import ctypes as C
import functools

import numpy as np

import oracle as O
import seq_multi_ref as R
import tabular_mdp_ref as T

L = O.lib()
CONTINUE, TERMINATE, INTERRUPT = 0, 1, 2
F32 = np.float32
MIN_MARGIN = R.MIN_MARGIN  # the project's: 1e-5

Dist = collections.namedtuple("Dist", "S A E L alpha prior_mean prior_stddev reward_stddev")


def dist(S, A, E, L_, alpha=1.0, prior_mean=1.0, prior_stddev=1.0, reward_stddev=1.0):
    return Dist(S, A, E, L_, alpha, prior_mean, prior_stddev, reward_stddev)


def trial_steps(d):
    return d.E * (d.L + 1) - 1


def features(d, state, prev, done):
    """[inner is None] [one-hot(inner state), S] [prev is None] [one-hot(prev action), A] [prev reward] [episode_done]
    (the inner observation is never None: TabularMdp never terminates, the limit's Interrupt keeps the state)"""
    f = np.zeros(d.S + d.A + 4, F32)
    f[1 + state] = 1.0
    if prev is None:
        f[1 + d.S] = 1.0
    else:
        action, reward = prev
        f[2 + d.S + action] = 1.0
        f[2 + d.S + d.A] = F32(reward)
    f[d.S + d.A + 3] = 1.0 if done else 0.0
    return f


def sample_tables(d, rng):
    """DirichletRandomMdps::sample_environment from `rng` where it stands -> (cum [S][A][S] f32, mean [S][A] f64)"""
    tr = np.zeros((d.S, d.A, d.S), F32)
    mean = np.zeros((d.S, d.A), np.float64)
    for s in range(d.S):
        for a in range(d.A):
            g = [T.gamma(d.alpha, rng) for _ in range(d.S)]
            total = 0.0
            for x in g:
                total = total + x
            for j in range(d.S):
                tr[s, a, j] = F32(g[j] / total)
            z, _n = T.normal(rng)
            mean[s, a] = d.prior_mean + d.prior_stddev * z
    return T.cumulative(tr), mean


class MetaMdpLane:
    def __init__(self, d, seed_env, global_lane):
        self.d = d
        self.rng = T.make_rng(seed_env, global_lane)
        self.trials = 0
        self.reset()

    def reset(self):
        """TrialEpisodeLimit / MetaEnv::initial_state: sample_environment, then the inner initial_state (no draw)"""
        self.cum, self.mean = sample_tables(self.d, self.rng)
        self.trials += 1
        self.state, self.inner_left = 0, self.d.L
        self.inner_done = False
        self.prev = None
        self.remaining = self.d.E

    def obs_features(self):
        return features(self.d, self.state, self.prev, self.inner_done)

    def step(self, action):
        """-> (reward f32, successor kind); on Interrupt the lane holds the successor state (observe it, then reset())"""
        if self.inner_done:  # the action is ignored; nothing is drawn
            self.state, self.inner_left = 0, self.d.L
            self.inner_done = False
            self.prev = None
            return F32(0.0), CONTINUE
        s, a = self.state, int(action)
        w = T.next_u64(self.rng)
        nxt = T.successor(self.cum[s, a], T.unit_f32(w & 0xFFFFFFFF))
        r = float(self.mean[s, a])
        if self.d.reward_stddev != 0.0:
            z, _n = T.normal(self.rng)
            r = float(self.mean[s, a]) + self.d.reward_stddev * z
        r = F32(r)
        self.state = nxt
        self.prev = (a, r)
        self.inner_left -= 1
        if self.inner_left == 0:
            self.inner_done = True
            self.remaining -= 1
            if self.remaining == 0:
                return r, INTERRUPT
        return r, CONTINUE


class MetaMdpLanes:
    """n lanes stepped the way the library's env handle steps them"""

    def __init__(self, n, d, lane_offset=0, seed_env=0):
        self.n, self.d, self.D = n, d, d.S + d.A + 4
        self.lanes = [MetaMdpLane(d, seed_env, lane_offset + i) for i in range(n)]

    def reset(self):
        for lane in self.lanes:
            lane.reset()

    def observe(self):
        return np.stack([lane.obs_features() for lane in self.lanes], axis=1)  # [D][n]

    def tables(self):
        """(cum [n][S][A][S] f32, mean [n][S][A] f64) of the current trials"""
        return np.stack([lane.cum for lane in self.lanes]), np.stack([lane.mean for lane in self.lanes])

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
                lane.reset()
        return reward, flag, self.observe(), term


# ---------------------------------------------------------------- driven steps
Driven = collections.namedtuple("Driven", "dist seed note")
N_LANES, OFFSET, TRIALS = 70, 25, 3
DRIVEN = [
    Driven(dist(2, 2, 1, 1), 11, "a reset at every step"),
    Driven(dist(3, 2, 2, 3, reward_stddev=0.5), 12, ""),
    Driven(dist(5, 5, 3, 4), 13, "the default sizes"),
    Driven(dist(8, 4, 2, 2, alpha=0.5), 14, "the Gamma path below 1"),
    Driven(dist(4, 8, 2, 2, alpha=2.5), 15, "Marsaglia-Tsang"),
    Driven(dist(3, 2, 2, 3, reward_stddev=0.0), 16, "no per-step normal draw"),
]
DrivenRef = collections.namedtuple("DrivenRef", "observe0 tables0 actions steps")
"""steps: per step (reward, flag, obs, term_obs, tables after the step)"""


def driven_id(c):
    d = c.dist
    return "S%d-A%d-E%d-L%d-alpha%g-sd%g" % (d.S, d.A, d.E, d.L, d.alpha, d.reward_stddev)


def driven_steps(c):
    return TRIALS * trial_steps(c.dist) + 1  # three whole trials and the first step of the fourth


@functools.lru_cache(maxsize=None)
def driven_reference(c):
    lanes = MetaMdpLanes(N_LANES, c.dist, seed_env=c.seed)
    rs = np.random.default_rng(1000 + c.seed)
    observe0, tables0 = lanes.observe(), lanes.tables()
    actions, steps = [], []
    for _ in range(driven_steps(c)):
        a = rs.integers(0, c.dist.A, N_LANES).astype(np.uint8)
        actions.append(a)
        steps.append(lanes.step(a) + (lanes.tables(),))
    return DrivenRef(observe0, tables0, actions, steps)


# ---------------------------------------------------------------- closed-loop rollouts
Closed = collections.namedtuple("Closed", "net dist n T offset seed")
# (D = S + A + 4, outputs = A); seed: the module's init seed, seed_env = seed + 1, seed_actor = seed + 2.  The seeds are
# chosen on the CPU (tests/test_meta_mdp_ref.py) so that every sampled action is decided by more than MIN_MARGIN.
# Every shape of the one-launch table (handle_spec.hpp) and (3,3) outside it; both cells and both tails; 1, 64, 65 and 130
# lanes; a lane offset; T = 7 against trials of 3 and 5 steps, so that a trial runs across the two collections.
CLOSED = [
    Closed(R.Net("gru", 8, 12, 1, 0, True, 2), dist(2, 2, 2, 2), 130, 7, 0, 501),
    Closed(R.Net("lstm", 9, 9, 2, 6, True, 2), dist(3, 2, 2, 1), 65, 7, 0, 511),
    Closed(R.Net("gru", 11, 10, 1, 7, False, 3), dist(4, 3, 1, 3), 64, 7, 0, 521),
    Closed(R.Net("lstm", 14, 8, 1, 0, True, 5), dist(5, 5, 2, 2), 45, 7, 25, 531),
    Closed(R.Net("gru", 16, 7, 1, 0, True, 4), dist(8, 4, 2, 2, alpha=0.5), 1, 7, 0, 541),
    Closed(R.Net("lstm", 16, 8, 1, 6, True, 8), dist(4, 8, 3, 1, alpha=2.5), 65, 7, 0, 551),
    Closed(R.Net("gru", 10, 9, 1, 6, True, 3), dist(3, 3, 2, 2), 65, 7, 0, 561),
]
PERIODS = 2
Reference = collections.namedtuple("Reference", "periods margin observe tables")


def closed_id(c):
    d = c.dist
    return "%s-S%d-A%d-E%d-L%d-n%d-T%d-off%d" % (R.net_id(c.net), d.S, d.A, d.E, d.L, c.n, c.T, c.offset)


def closed_params(c):
    inits = list(O.RNN_DEFAULT_INITS)
    if c.net.bias:
        inits[2] = R.BIAS_INIT
    return R.init(c.net, c.seed, tuple(inits))


def expected_interrupts(c, periods=PERIODS):
    """per period the steps that end a trial: every lane starts a trial at the run's first step"""
    length = trial_steps(c.dist)
    return [[t for t in range(c.T) if (p * c.T + t + 1) % length == 0] for p in range(periods)]


def rollout(net, d, n, T_, seed_env, seed_actor, params, lane_offset=0, periods=PERIODS):
    k = net.A
    assert net.D == d.S + d.A + 4 and k == d.A
    shape, full = R.shape_of(net), R.to_oracle(net, np.ascontiguousarray(params, dtype=np.float32))
    lanes = MetaMdpLanes(n, d, lane_offset=lane_offset, seed_env=seed_env)
    rngs = []
    for i in range(n):
        r = O.Prng()
        L.oracle_prng_seed_from_u64(C.byref(r), seed_actor)
        L.oracle_prng_set_stream(C.byref(r), lane_offset + i)
        rngs.append(r)
    lp = np.zeros(k, F32)
    margin = np.inf
    out = []
    for period in range(periods):
        obs = np.zeros((net.D, T_ + 1, n), F32)
        term = np.zeros((net.D, T_, n), F32)
        action = np.zeros((T_, n), np.uint8)
        reward = np.zeros((T_, n), F32)
        flag = np.zeros((T_, n), np.uint8)
        obs[:, 0] = lanes.observe()
        for t in range(T_):
            prefix = {"obs": np.ascontiguousarray(obs[:, :t + 2]), "flag": np.ascontiguousarray(flag[:t + 1]),
                      "term_obs": np.ascontiguousarray(term[:, :t + 1])}
            z = O.stack_seq_forward(shape, net.L, full, prefix, want_succ=False)[0][:, t]  # [k][n]
            for i in range(n):
                L.oracle_prng_set_word_pos(C.byref(rngs[i]), period * T_ + t)
                w = L.oracle_prng_next_u32(C.byref(rngs[i]))
                u = F32(w >> 8) * F32(1.0 / (1 << 24))
                zi = np.ascontiguousarray(z[:, i])
                L.oracle_log_softmax_f32(O.f32p(zi), k, O.f32p(lp), 0)
                action[t, i] = L.oracle_categorical_sample_u(O.f32p(lp), k, C.c_float(u), 0)
                cum = np.cumsum(np.exp(R.log_softmax(zi.astype(np.float64))))[:-1]
                margin = min(margin, np.abs(np.float64(u) - cum).min())
            reward[t], flag[t], obs[:, t + 1], term[:, t] = lanes.step(action[t])
        out.append({"obs": obs, "action": action, "reward": reward, "flag": flag, "term_obs": term})
    return Reference(out, float(margin), lanes.observe(), lanes.tables())


@functools.lru_cache(maxsize=None)
def closed_reference(c):
    return rollout(c.net, c.dist, c.n, c.T, c.seed + 1, c.seed + 2, closed_params(c), lane_offset=c.offset)


def optimal_and_uniform_values(cum, mean, d):
    """f64 dynamic programming over one lane's tables -> (optimal, uniform-random) expected reward of a TRIAL: E inner
    episodes of L steps from state 0 (the restart steps earn nothing)"""
    P = np.diff(np.concatenate([np.zeros(cum.shape[:2] + (1,)), cum.astype(np.float64)], axis=2), axis=2)
    v_opt, v_uni = T.finite_horizon_values(P, mean, d.L)
    return d.E * v_opt, d.E * v_uni
