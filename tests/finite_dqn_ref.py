"""Reference for DQN over 3 to 8 actions (rl_dqn_create_finite / ra.FiniteDqn; test infrastructure, not a test): the
reference's DqnActor over a FiniteSpace (src/torch/agents/dqn.rs:360-379) — gen_bool(eps), then action_space.sample(rng) =
gen_range(0..A) on an exploring step, argmax (the first maximal of A action values) otherwise — and its targets
(dqn.rs:300-309: amax(-1) over A), restated on the oracle's pieces and on tests/recurrent_dqn_ref.py, which is general in
everything but the action count.

  gen_range      rand 0.8.5 UniformInt::<u64>::sample_single(0, A) written out on the raw words of the lane's actor stream
                 (tests/test_finite_dqn_cases.py pins it against the oracle's own gen_range and, at A = 2, against the
                 words the two-action restatement consumes)
  lanes          O.MemoryLaneSim for MemoryGame(k, h); the oracle's bandit lanes have two arms, so DeterministicBandit of
                 k arms is restated here (KBanditLanes; pinned against O.BanditLaneSim at two arms)
  modules        feed-forward: the f64 network of tests/test_gpu_general_mlp.py; recurrent: the oracle's teacher-forced f32
                 forward over the observations a lane's module has seen (recurrent_dqn_ref.last_outputs), f64 through
                 oracle/stacked.py
  closed_loop    one collection of the restated actor on the restated lanes, with the gap between the two largest action
                 values at every greedy step"""
import collections
import ctypes as C
import functools

import numpy as np

import finite_dqn_cases as FC
import oracle as O
import recurrent_dqn_ref as R
from oracle import stacked as S

MASK64 = (1 << 64) - 1


def gen_range(rng, A):
    """UniformInt::sample_single(0, A) for u64: widening multiply, zone = (A << A.leading_zeros()) - 1, retry on rejection"""
    zone = ((A << (64 - A.bit_length())) - 1) & MASK64
    while True:
        m = int(O.lib().oracle_prng_next_u64(C.byref(rng))) * A
        if (m & MASK64) <= zone:
            return m >> 64


# ---------------------------------------------------------------- lanes
class KBanditLanes:
    """DeterministicBandit::from_values(values) lanes (src/envs/bandits.rs:52-77,109-116) with the interface of the
    oracle's lane sims: one state, observed as one-hot(5); every step is an episode that Terminates with the chosen arm's
    value as its reward and draws nothing."""

    def __init__(self, n_lanes, values):
        self.n, self.D = n_lanes, 5
        self.values = np.array(values, dtype=np.float64).astype(np.float32)
        self.resets = np.ones(n_lanes, dtype=np.uint64)

    def observe(self):
        obs = np.zeros((self.D, self.n), dtype=np.float32)
        obs[0] = 1.0
        return obs

    def step(self, actions):
        a = np.asarray(actions).astype(np.int64)
        self.resets += np.uint64(1)
        return (self.values[a], np.full(self.n, O.TERMINATE, dtype=np.uint8), self.observe(),
                np.zeros((self.D, self.n), dtype=np.float32))

    def get_state(self):
        return np.zeros(self.n, dtype=np.uint64), np.zeros(self.n, dtype=np.uint64), self.resets.copy()


def make_sim(env_name, n):
    e = FC.ENVS[env_name]
    if e.kind == "bandit":
        sim = KBanditLanes(n, e.values)
    elif e.limit:
        sim = O.MemoryLaneSim(n, e.k, e.h, max_steps=e.limit, limit=O.LIMIT_VISIBLE, **FC.SEEDS)
    else:
        sim = O.MemoryLaneSim(n, e.k, e.h, **FC.SEEDS)
    assert sim.D == e.D
    return sim


def warm_up(env_name, sim, device_env=None):
    """the standalone steps before the first collection (finite_dqn_cases.Env.warm), on the oracle and the device"""
    for _ in range(FC.ENVS[env_name].warm):
        zeros = np.zeros(sim.n, dtype=np.uint8)
        want = sim.step(zeros)
        if device_env is not None:
            for a, b in zip(device_env.step(zeros), want):
                assert np.array_equal(a, b)


def possible_observations(env_name):
    """a superset of the observations the env emits, [rows][D] f32: one-hot states x (under a visible limit) remaining /
    max_steps"""
    e = FC.ENVS[env_name]
    states = 1 if e.kind == "bandit" else e.k + e.h
    rows = []
    for s in range(states):
        for k in (range(1, e.limit + 1) if e.limit else [0]):
            x = np.zeros(e.D, dtype=np.float32)
            x[s] = 1.0
            if e.limit:
                x[e.D - 1] = np.float32(float(k) / float(e.limit))
            rows.append(x)
    return np.array(rows)


# ---------------------------------------------------------------- modules
def module_of(case):
    return R.Module(*FC.REC_MODULES[case.module])


def case_params(case):
    """the module's flat parameters as the device initialises them"""
    e = FC.ENVS[case.env]
    if not FC.is_recurrent(case):
        return O.mlp_layers_init(e.D, FC.FF_MODULES[case.module][0], e.A, case.seed)
    m = module_of(case)
    inits = list(O.RNN_DEFAULT_INITS)
    inits[2] = R.BIAS_INIT
    if m.H2 is None:
        return R.CL.init(m.cell, e.D, m.H, m.L, e.A, m.bias, case.seed, tuple(inits))
    return O.stack_init_with(O.GruShape(e.D, m.H, m.H2, e.A, R.cell_of(m)), m.L, case.seed, tuple(inits))


def embedded(m, D, A, params):
    """recurrent_dqn_ref.embedded at A outputs -> (oracle shape, f64 spec, parameters in the oracle's layout, index)"""
    params = np.ascontiguousarray(params, dtype=np.float32)
    if m.H2 is None:
        return (R.CL.shape_of(m.cell, D, m.H, A), R.CL.spec_of(m.cell, D, m.H, m.L, A),
                R.CL.embed(m.cell, D, m.H, m.L, A, m.bias, params), R.CL.index(m.cell, D, m.H, m.L, A, m.bias))
    spec = S.Spec(S.GRU if m.cell == "gru" else S.LSTM, D, m.H, m.L, m.H2, A)
    assert params.shape == (spec.num_params(),)
    return O.GruShape(D, m.H, m.H2, A, R.cell_of(m)), spec, params, np.arange(len(params))


def first_max(q):
    """argmax over axis 0: the first maximal index"""
    return np.argmax(q, axis=0).astype(np.uint8)


def top_gap(q):
    """the gap between the largest and the second-largest value along axis 0"""
    s = np.sort(np.asarray(q, dtype=np.float64), axis=0)
    return s[-1] - s[-2]


class FiniteActor:
    """DqnActor over n lanes and A actions.  Feed-forward: the greedy action is the first maximal output of the f64 network
    at the lane's observation.  Recurrent: as recurrent_dqn_ref.RecurrentActor — `seen[i]` holds the observations lane i's
    module has stepped over since its state was zero; an exploring step adds nothing."""

    def __init__(self, case, params, lane_offset=0):
        from test_gpu_general_mlp import unflatten
        e = FC.ENVS[case.env]
        self.case, self.D, self.A, self.n = case, e.D, e.A, case.n
        self.recurrent = FC.is_recurrent(case)
        if self.recurrent:
            self.m = module_of(case)
            self.shape, _, self.params, _ = embedded(self.m, e.D, e.A, params)
        else:
            self.hidden, self.activation = FC.FF_MODULES[case.module]
            self.net = unflatten(np.asarray(params), e.D, self.hidden, e.A)
        self.rngs = R.actor_streams(case.n, FC.SEEDS["seed_actor"], lane_offset)
        self.begin_collection()

    def begin_collection(self):
        self.seen = [[] for _ in range(self.n)]

    def values(self, obs, lanes):
        """action values [A][len(lanes)] of the greedy lanes at this step"""
        if self.recurrent:
            return R.last_outputs(self.shape, self.m.L, self.params, [self.seen[i] for i in lanes], self.D)
        from test_gpu_general_mlp import forward64
        z, _ = forward64(self.net, obs[:, lanes].T, self.activation, "Identity")
        return z.T

    def act(self, obs, eps):
        """obs [D][n] -> (actions, explore mask, the least top-two gap of the step's greedy lanes (inf: none))"""
        L, n = O.lib(), self.n
        a, explore = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=bool)
        for i in range(n):
            if L.oracle_prng_gen_bool(C.byref(self.rngs[i]), eps):
                a[i] = gen_range(self.rngs[i], self.A)
                explore[i] = True
            elif self.recurrent:
                self.seen[i].append(obs[:, i].copy())
        g = np.flatnonzero(~explore)
        gap = np.inf
        if len(g):
            q = self.values(obs, g)
            a[g] = first_max(q)
            gap = float(top_gap(q).min())
        return a, explore, gap

    def end_step(self, flags):
        for i in np.flatnonzero(np.asarray(flags) != O.CONTINUE):
            self.seen[i] = []

    def positions(self):
        return np.array([O.lib().oracle_prng_word_pos(C.byref(r)) for r in self.rngs], dtype=np.uint64)


Loop = collections.namedtuple("Loop", "greedy explored margin cuts")


def closed_loop(case, eps, params=None):
    """both collections of the restated actor on the restated lanes -> Loop(greedy action counts [A], explored action
    counts [A], the least top-two gap over every greedy step, lanes cut by the horizon per collection)"""
    e = FC.ENVS[case.env]
    sim = make_sim(case.env, case.n)
    warm_up(case.env, sim)
    actor = FiniteActor(case, case_params(case) if params is None else params)
    greedy, explored = np.zeros(e.A, dtype=np.int64), np.zeros(e.A, dtype=np.int64)
    margin, cuts = np.inf, []
    for T in FC.HORIZONS:
        actor.begin_collection()
        cur = sim.observe()
        for t in range(T):
            a, explore, gap = actor.act(cur, eps)
            margin = min(margin, gap)
            greedy += np.bincount(a[~explore], minlength=e.A)
            explored += np.bincount(a[explore], minlength=e.A)
            _, flag, cur, _ = sim.step(a)
            actor.end_step(flag)
        cuts.append(int((flag == O.CONTINUE).sum()))
    return Loop(greedy, explored, float(margin), cuts)


@functools.lru_cache(maxsize=None)
def case_loops(case):
    """the case's closed loops at eps = 0.5 and 0 (computed once per process; callers leave them unchanged)"""
    return {eps: closed_loop(case, eps) for eps in (0.5, 0.0)}


# ---------------------------------------------------------------- targets, in f64
def reward_to_go(reward, gamma):
    """G_t = r_t + gamma * G_{t+1} over one stored episode"""
    out, g = np.zeros(len(reward)), 0.0
    for j in range(len(reward) - 1, -1, -1):
        g = float(reward[j]) + (float(np.float32(gamma)) * g if j < len(reward) - 1 else 0.0)
        out[j] = g
    return out


def td_targets(v_next, reward, flags, gamma):
    """r_t + gamma * V(s_{t+1}) with V = 0 beyond a Terminate; v_next [len]: amax over the A action values at the
    successor — the next stored step, or the stored successor observation after an Interrupt"""
    v = np.where(np.asarray(flags) == O.TERMINATE, 0.0, v_next)
    return np.asarray(reward, dtype=np.float64) + float(np.float32(gamma)) * v


def recurrent_episode_values(spec, full, obs, flags, succ):
    """seq_packed over one stored episode from the zero state, in f64: obs [len][D], flags [len], succ [len][D] -> (q
    [A][len], amax of the extended sequence's next slot [len])"""
    n_steps, D = obs.shape
    traj = dict(obs=np.concatenate([obs.T[:, :, None], np.zeros((D, 1, 1))], axis=1),
                flag=np.asarray(flags, dtype=np.uint8)[:, None], term_obs=succ.T[:, :, None].astype(np.float64))
    q, qs, _ = S.forward(spec, full, traj)
    v = np.zeros(n_steps)
    for j in range(n_steps):
        if flags[j] == O.INTERRUPT:
            v[j] = qs[:, j, 0].max()
        elif flags[j] == O.CONTINUE:
            v[j] = q[:, j + 1, 0].max()
    return q[:, :, 0], v
