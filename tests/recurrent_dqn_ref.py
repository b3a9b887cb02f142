"""Reference for DQN with a recurrent action-value module (rl_dqn_create_recurrent; test infrastructure, not a test):
the reference's DqnActor over a sequence module (src/torch/agents/dqn.rs:348-380) and its targets (dqn.rs:293-314,
critics/mod.rs:101-148), restated on the oracle's pieces.

The actor, per lane and step, from the lane's sequential actor stream (oracle Prng: seed_from_u64(seed_actor),
set_stream(global lane)): gen_bool(eps) first (no draw at eps == 1.0); an exploring step returns gen_range(0..2) BEFORE
the module's step(), so the module never sees that observation and the lane's recurrent state stays what it was; a greedy
step advances the state and takes the first maximal output.  The state is zero at an episode's first step and at the
first step of every collection.  A recurrent state is a function of the observations the module has seen since it was
zero, so the restatement keeps that list per lane and evaluates the module with the oracle's teacher-forced forward
(O.stack_seq_forward, f32: the lane kernels' arithmetic contract, bit for bit) over it.  `hold` False is the WRONG actor
— one that also advances the state on exploring steps — kept beside the right one so that a test can show that its cases
tell the two apart (tests/test_recurrent_dqn_ref_cpu.py).

Modules with a Linear tail or without recurrent bias vectors are evaluated through their embedding into the oracle's
MLP-tail chain (tests/chain_linear_ref.py, tests/meta_rollout_ref.py: bit-exact under the same contract)."""
import collections
import ctypes as C

import numpy as np

import chain_linear_ref as CL
import oracle as O
from oracle import stacked as S

BIAS_INIT = ("Uniform", "FanAvg", 0.0)  # recurrent bias vectors that are not the default's zeros

# cell, recurrent width, layers, MLP hidden width (None: a Linear tail), recurrent bias vectors
Module = collections.namedtuple("Module", "cell H L H2 bias")
MODULES = {
    "gru-5-mlp-6": Module("gru", 5, 1, 6, True),                  # one partial unit quad
    "lstm-2x33-linear-nobias": Module("lstm", 33, 2, None, False),  # a second trip of the unit loop for wave 0 alone
    "gru-128-mlp-128": Module("gru", 128, 1, 128, True),          # the shape that otherwise runs the tile kernels
}


def cell_of(m):
    return O.CELL_GRU if m.cell == "gru" else O.CELL_LSTM


def module_params(m, D, seed):
    """the module's flat parameters as the device initialises them (init_with at BIAS_INIT where it has bias vectors)"""
    inits = list(O.RNN_DEFAULT_INITS)
    if m.bias:
        inits[2] = BIAS_INIT
    if m.H2 is None:
        return CL.init(m.cell, D, m.H, m.L, 2, m.bias, seed, tuple(inits))
    assert m.bias
    return O.stack_init_with(O.GruShape(D, m.H, m.H2, 2, cell_of(m)), m.L, seed, tuple(inits))


def embedded(m, D, params):
    """-> (oracle shape, f64 spec, parameters in the oracle's MLP-tail layout, index of the module's entries in it)"""
    params = np.ascontiguousarray(params, dtype=np.float32)
    if m.H2 is None:
        return (CL.shape_of(m.cell, D, m.H, 2), CL.spec_of(m.cell, D, m.H, m.L, 2),
                CL.embed(m.cell, D, m.H, m.L, 2, m.bias, params), CL.index(m.cell, D, m.H, m.L, 2, m.bias))
    spec = S.Spec(S.GRU if m.cell == "gru" else S.LSTM, D, m.H, m.L, m.H2, 2)
    assert params.shape == (spec.num_params(),)
    return O.GruShape(D, m.H, m.H2, 2, cell_of(m)), spec, params, np.arange(len(params))


def actor_streams(n, seed_actor, lane_offset=0):
    L, rngs = O.lib(), []
    for i in range(n):
        r = O.Prng()
        L.oracle_prng_seed_from_u64(C.byref(r), seed_actor)
        L.oracle_prng_set_stream(C.byref(r), lane_offset + i)
        L.oracle_prng_set_word_pos(C.byref(r), 0)
        rngs.append(r)
    return rngs


def last_outputs(shape, num_layers, params, histories, D):
    """the module's outputs after each of the observation lists `histories` (each from the zero state) -> [2][len]"""
    n, T = len(histories), max(len(h) for h in histories)
    obs = np.zeros((D, T + 1, n), dtype=np.float32)
    for i, h in enumerate(histories):
        obs[:, :len(h), i] = np.array(h, dtype=np.float32).T
    traj = dict(obs=obs, flag=np.zeros((T, n), dtype=np.uint8), term_obs=np.zeros((D, T, n), dtype=np.float32))
    out, _ = O.stack_seq_forward(shape, num_layers, params, traj, want_succ=False)
    return np.stack([out[:, len(h) - 1, i] for i, h in enumerate(histories)], axis=1)


class RecurrentActor:
    """DqnActor over n lanes.  `seen[i]`: the observations lane i's module has stepped over since its state was zero
    (the right actor's state); `all_steps[i]`: every observation of the lane's episode since the collection began (the
    state of the wrong actor, which steps on exploring steps too)."""

    def __init__(self, module, D, params, n, seed_actor, hold=True):
        self.m, self.D, self.n, self.hold = module, D, n, hold
        self.shape, _, self.params, _ = embedded(module, D, params)
        self.rngs = actor_streams(n, seed_actor)
        self.begin_collection()

    def begin_collection(self):
        self.seen = [[] for _ in range(self.n)]
        self.all_steps = [[] for _ in range(self.n)]

    def act(self, obs, eps):
        """obs [D][n] -> (actions, explore mask, q [2][n] of the acting restatement (NaN on exploring lanes), q of the
        other restatement at the same greedy steps)"""
        L, n = O.lib(), self.n
        a, explore = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=bool)
        for i in range(n):
            if L.oracle_prng_gen_bool(C.byref(self.rngs[i]), eps):
                a[i] = L.oracle_prng_gen_range_u64(C.byref(self.rngs[i]), 0, 2)
                explore[i] = True
            else:
                self.seen[i].append(obs[:, i].copy())
            self.all_steps[i].append(obs[:, i].copy())
        q = np.full((2, n), np.nan, dtype=np.float32)
        q_other = q.copy()
        g = np.flatnonzero(~explore)
        if len(g):
            mine, other = (self.seen, self.all_steps) if self.hold else (self.all_steps, self.seen)
            q[:, g] = last_outputs(self.shape, self.m.L, self.params, [mine[i] for i in g], self.D)
            q_other[:, g] = last_outputs(self.shape, self.m.L, self.params, [other[i] for i in g], self.D)
            a[g] = (q[1, g] > q[0, g]).astype(np.uint8)  # argmax: first maximal index
        return a, explore, q, q_other

    def end_step(self, flags):
        for i in np.flatnonzero(np.asarray(flags) != O.CONTINUE):
            self.seen[i], self.all_steps[i] = [], []

    def positions(self):
        return np.array([O.lib().oracle_prng_word_pos(C.byref(r)) for r in self.rngs], dtype=np.uint64)


def closed_loop(actor, sim, T, eps):
    """one collection of the restated actor on the oracle's lanes.  -> per step (obs, action, explore, q, q_other,
    reward, flag as the store records it)"""
    actor.begin_collection()
    steps, cur = [], sim.observe()
    for t in range(T):
        a, explore, q, q_other = actor.act(cur, eps)
        reward, flag, nxt, _ = sim.step(a)
        actor.end_step(flag)
        rec_flag = flag.copy()
        if t == T - 1:
            rec_flag[flag == O.CONTINUE] = O.INTERRUPT  # the horizon rule
        steps.append(dict(obs=cur, action=a, explore=explore, q=q, q_other=q_other, reward=reward, flag=rec_flag,
                          env_flag=flag))
        cur = nxt
    return steps


# ---------------------------------------------------------------- targets
def episode_outputs(shape, num_layers, params, obs, flags, succ):
    """seq_packed over one stored episode from the zero state, extended by the successor observation of its Interrupt:
    obs [len][D], flags [len], succ [len][D] -> (q [2][len], q at the successor observations [2][len])"""
    n_steps, D = obs.shape
    traj = dict(obs=np.concatenate([obs.T[:, :, None], np.zeros((D, 1, 1), np.float32)], axis=1).astype(np.float32),
                flag=np.asarray(flags, dtype=np.uint8)[:, None].copy(),
                term_obs=np.ascontiguousarray(succ.T[:, :, None], dtype=np.float32))
    out, sout = O.stack_seq_forward(shape, num_layers, params, traj)
    return out[:, :, 0], sout[:, :, 0]


def episode_targets(shape, num_layers, params, obs, reward, flags, succ, gamma, td):
    """the f32 targets of one stored episode.  RewardToGo: G_t = r_t + G_{t+1} * gamma (multiply, then add).  OneStepTd:
    r_t + gamma * V_ext[t + 1], V_ext = amax over the actions of the module's outputs over the extended sequence — the next
    step's, the successor observation's after an Interrupt, 0 after a Terminate (`scalar * tensor`, then add)."""
    reward = np.asarray(reward, dtype=np.float32)
    gamma = np.float32(gamma)
    n_steps = len(reward)
    tgt = np.zeros(n_steps, dtype=np.float32)
    if not td:
        g = np.float32(0.0)
        for j in range(n_steps - 1, -1, -1):
            g = reward[j] if j == n_steps - 1 else np.float32(reward[j] + np.float32(g * gamma))
            tgt[j] = g
        return tgt
    q, qs = episode_outputs(shape, num_layers, params, obs, flags, succ)
    for j in range(n_steps):
        if flags[j] == O.TERMINATE:
            v = np.float32(0.0)
        elif flags[j] == O.INTERRUPT:
            v = max(qs[0, j], qs[1, j])
        else:
            v = max(q[0, j + 1], q[1, j + 1])
        tgt[j] = np.float32(reward[j] + np.float32(gamma * np.float32(v)))
    return tgt


# ---------------------------------------------------------------- the sampler
def sample_minibatch(agent_rng, rings, minibatch_steps):
    """sample_minibatch of dqn.rs:280-291 on restated rings (tests/dqn_ring_ref.py): cycle over the lanes, one
    Uniform::new(0, num_episodes) draw each — index = high half of the widening multiply; a rejection has probability
    below num_episodes / 2^64 and is asserted away — take while the total before the episode is below minibatch_steps;
    the refused episode's draw is consumed.  -> (lanes, starts, lens)"""
    L = O.lib()
    lanes, starts, lens, total, cand = [], [], [], 0, 0
    while True:
        lane = cand % len(rings)
        k = rings[lane].num_episodes()
        assert k > 0
        v = int(L.oracle_prng_next_u64(C.byref(agent_rng)))
        assert (v * k) % (1 << 64) <= (1 << 64) - 1 - ((1 << 64) - k) % k
        start, length = rings[lane].episode((v * k) >> 64)
        if not total < minibatch_steps:
            return np.array(lanes, np.uint32), np.array(starts, np.uint32), np.array(lens, np.uint32)
        lanes.append(lane)
        starts.append(start)
        lens.append(length)
        total += length
        cand += 1


def agent_stream(key):
    r = O.Prng()
    O.lib().oracle_prng_from_seed(C.byref(r), (C.c_uint32 * 8)(*[int(k) for k in key]))
    return r


# ---------------------------------------------------------------- the cases the CPU and the GPU tests share
SEEDS = dict(seed_env=11, seed_actor=12)
N_LANES, HORIZONS = 70, (9, 7)  # a full workgroup plus six live lanes; episodes start and end mid-collection
# name -> (oracle lanes, D, the env's discount factor)
ENVS = {
    "chain-latent-7": (lambda n: O.ChainLaneSim(n, max_steps=7, limit=O.LIMIT_LATENT, **SEEDS), 5, 0.95),
    "chain-visible-7": (lambda n: O.ChainLaneSim(n, max_steps=7, limit=O.LIMIT_VISIBLE, **SEEDS), 6, 0.95),
    "bandit": (lambda n: O.BanditLaneSim(n, (0.0, 1.0), **SEEDS), 5, 1.0),
    "memory-2-3": (lambda n: O.MemoryLaneSim(n, 2, 3, **SEEDS), 5, 1.0),
    "memory-2-6": (lambda n: O.MemoryLaneSim(n, 2, 6, **SEEDS), 8, 1.0),
    "cartpole-visible-7": (lambda n: O.LaneSim(n, max_steps=7, limit=O.LIMIT_VISIBLE, **SEEDS), 5, 0.99),
}
# (env, module, init seed).  Every episode of the bandit is one step: the state is zero at every step, so holding it and
# advancing it are the same function there — no seed can tell the two actors apart on those lanes, and the rule of
# tests/test_recurrent_dqn_ref_cpu.py (b) is asserted on every other case.
# The seeds: the first from 77 on at which the right and the wrong actor differ on at least three greedy steps of the case.
CASE_SEEDS = {
    "gru-5-mlp-6": {"chain-latent-7": 88, "chain-visible-7": 81, "bandit": 77, "memory-2-3": 88, "memory-2-6": 84,
                    "cartpole-visible-7": 90},
    "lstm-2x33-linear-nobias": {"chain-latent-7": 83, "chain-visible-7": 113, "bandit": 77, "memory-2-3": 85,
                                "memory-2-6": 82, "cartpole-visible-7": 83},
}
COLLECT_CASES = [(env, mod, CASE_SEEDS[mod][env]) for mod in sorted(CASE_SEEDS) for env in ENVS]
COLLECT_CASES.append(("chain-latent-7", "gru-128-mlp-128", 86))


def warm_up(env_name, sim, device_env=None):
    """a MemoryGame's episodes all have one length (here 4 or 7 steps), which divides the 16 steps of both collections:
    one standalone step first (oracle and, where given, device), so that both collections start and end mid-episode on
    every lane"""
    if not env_name.startswith("memory"):
        return
    zeros = np.zeros(sim.n, dtype=np.uint8)
    want = sim.step(zeros)
    if device_env is not None:
        for a, b in zip(device_env.step(zeros), want):
            assert np.array_equal(a, b)


def case_id(case):
    return "%s-%s" % (case[0], case[1])
