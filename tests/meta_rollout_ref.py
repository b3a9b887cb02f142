"""Closed-loop reference of a recurrent policy's rollout on the meta-bandit lanes (test infrastructure, not a test).

The library's rollout (relearn_amd/csrc/kernels_seq_stack.hip: k_stack_rollout in one launch, or k_stack_step and the env
kernels launched per step) is restated here from seeds alone, out of three parts that share no code with it:
  the logits at step t   oracle.stack_seq_forward (oracle/stack_impl.inc) over the prefix 0..t of the planes built so far:
                         teacher-forced and causal, the states restart at t = 0 and after a step that is not Continue
  the action             oracle_log_softmax_f32 / oracle_categorical_sample_u at the uniform of word period * T + t of actor
                         stream lane_offset + i
  the env                tests/meta_lanes_ref.py
Every step's forward starts again from t = 0, so the cost is quadratic in T; the horizons here are 13 steps at the most.

GRID holds the cases that tests/test_meta_rollout_ref.py (the reference against itself, no device) and
tests/test_gpu_meta_rollout_shapes.py (the device against the reference) share."""
import collections
import ctypes as C
import functools

import numpy as np

import meta_lanes_ref as M
import oracle as O
from oracle import stacked as S

L = O.lib()
D, ARMS = 6, 2
PLANES = ("obs", "action", "reward", "flag", "term_obs")
BIAS_INIT = ("Uniform", "FanAvg", 0.0)  # recurrent bias vectors that are not the default's zeros

Case = collections.namedtuple("Case", "cell H L H2 bias n T E arms offset seed")
# seed: the module's init seed; seed_env = seed + 1, seed_actor = seed + 2
GRID = [
    Case("gru", 33, 2, 9, True, 70, 13, 3, M.UNIFORM_BERNOULLI, 0, 101),  # second unit pass of one unit, layer loop, K tail
    Case("lstm", 65, 3, 33, True, 70, 13, 3, M.ONE_HOT, 0, 111),          # third pass, cell planes of 3 layers, head's 2nd pass
    Case("gru", 128, 1, 128, True, 130, 13, 10, M.UNIFORM_BERNOULLI, 0, 121),  # no Interrupt in period 0; 3 workgroups
    Case("lstm", 7, 4, 5, True, 1, 13, 1, M.UNIFORM_BERNOULLI, 0, 131),   # one lane, four layers, restart at every step
    Case("gru", 12, 2, 8, False, 64, 13, 3, M.UNIFORM_BERNOULLI, 0, 141),  # no bias vectors; exactly one workgroup
    Case("lstm", 24, 2, 12, False, 128, 7, 2, M.ONE_HOT, 0, 151),         # the same on the LSTM; exactly two workgroups
    Case("gru", 160, 1, 130, True, 65, 13, 3, M.UNIFORM_BERNOULLI, 0, 161),  # widths past 128
    Case("gru", 10, 1, 6, True, 45, 13, 3, M.UNIFORM_BERNOULLI, 25, 171),  # lane_offset: lanes 25..69 of the 70-lane run
    Case("lstm", 18, 2, 10, True, 70, 1, 3, M.UNIFORM_BERNOULLI, 0, 181),  # T = 1
    Case("gru", 20, 2, 16, True, 70, 10, 3, M.ROUND_ROBIN, 0, 191),       # no env draws; two whole trials per collection
    # the one-lane case again at 70 lanes: a rollout shows its states only through the actions they decide, and one
    # lane's 26 draws let a state that never restarted (or a layer fed from the wrong set) pass — 1,820 draws do not
    Case("lstm", 7, 4, 5, True, 70, 13, 1, M.UNIFORM_BERNOULLI, 0, 201),
]
PERIODS = 2
Reference = collections.namedtuple("Reference", "periods margin observe driven")
"""periods: per period the five planes; margin: the smallest |u - p(action 0)| of the run; observe: the lanes'
observation after the last period [6][n]; driven: (reward, flag, obs, term_obs) of one more step at DRIVEN actions"""


def case_id(c):
    return "%s-%d-%d-%d-%s-n%d-T%d-E%d-%s-off%d" % (c.cell, c.H, c.L, c.H2, "bias" if c.bias else "nobias", c.n, c.T, c.E,
                                                   c.arms, c.offset)


def driven_actions(n):
    return (np.arange(n) % ARMS).astype(np.uint8)


def shape_of(cell, H, H2):
    return O.GruShape(D, H, H2, ARMS, O.CELL_GRU if cell == "gru" else O.CELL_LSTM)


def bias_free_index(cell, H, num_layers, H2):
    """indices, in the flat vector of the module WITH recurrent bias vectors, of everything else: the layout of the
    module built without them"""
    spec = S.Spec(S.GRU if cell == "gru" else S.LSTM, D, H, num_layers, H2, ARMS)
    sl, P = spec.slices()
    drop = [np.arange(o, o + int(np.prod(shp))) for name, _, shp, o in sl if name in ("bih", "bhh")]
    return np.setdiff1d(np.arange(P), np.concatenate(drop)), P


def case_params(c):
    """the module's flat parameters as the device initialises them: with bias vectors rl_rnn_mlp_init_with at BIAS_INIT,
    without them the default initialisation (the Zeros bias initializer draws nothing, so it is the default vector of
    the module with biases, less the bias entries)"""
    shape = shape_of(c.cell, c.H, c.H2)
    if c.bias:
        inits = list(O.RNN_DEFAULT_INITS)
        inits[2] = BIAS_INIT
        return O.stack_init_with(shape, c.L, c.seed, tuple(inits))
    keep, _ = bias_free_index(c.cell, c.H, c.L, c.H2)
    return O.stack_init(shape, c.L, c.seed)[keep]


def expand_params(cell, H, num_layers, H2, rnn_bias, params):
    """-> the with-bias layout (zero bias vectors where the module has none)"""
    params = np.ascontiguousarray(params, dtype=np.float32)
    if rnn_bias:
        return params
    keep, P = bias_free_index(cell, H, num_layers, H2)
    assert params.shape == (len(keep),)
    full = np.zeros(P, np.float32)
    full[keep] = params
    return full


def expected_interrupts(T, E, periods=PERIODS):
    """per period the steps that end a trial: every lane starts a trial at the run's first step, a trial is 2 E - 1 steps"""
    length = 2 * E - 1
    return [[t for t in range(T) if (p * T + t + 1) % length == 0] for p in range(periods)]


def rollout(cell, H, num_layers, H2, rnn_bias, n, T, E, distribution, seed_env, seed_actor, params, lane_offset=0,
            periods=PERIODS, in_dim=D):
    assert in_dim == D
    shape = shape_of(cell, H, H2)
    full = expand_params(cell, H, num_layers, H2, rnn_bias, params)
    lanes = M.MetaLanes(n, ARMS, E, distribution, lane_offset=lane_offset, seed_env=seed_env)
    rngs = []
    for i in range(n):
        r = O.Prng()
        L.oracle_prng_seed_from_u64(C.byref(r), seed_actor)
        L.oracle_prng_set_stream(C.byref(r), lane_offset + i)
        rngs.append(r)
    lp = np.zeros(ARMS, np.float32)
    margin = np.inf
    out = []
    for period in range(periods):
        obs = np.zeros((D, T + 1, n), np.float32)
        term = np.zeros((D, T, n), np.float32)
        action = np.zeros((T, n), np.uint8)
        reward = np.zeros((T, n), np.float32)
        flag = np.zeros((T, n), np.uint8)
        obs[:, 0] = lanes.observe()
        for t in range(T):
            # steps 0..t; slot t + 1 and flag[t] are not read by the outputs up to t (want_succ False)
            prefix = {"obs": np.ascontiguousarray(obs[:, :t + 2]), "flag": np.ascontiguousarray(flag[:t + 1]),
                      "term_obs": np.ascontiguousarray(term[:, :t + 1])}
            z = O.stack_seq_forward(shape, num_layers, full, prefix, want_succ=False)[0][:, t]  # [2][n]
            for i in range(n):
                L.oracle_prng_set_word_pos(C.byref(rngs[i]), period * T + t)
                w = L.oracle_prng_next_u32(C.byref(rngs[i]))
                u = np.float32(w >> 8) * np.float32(1.0 / (1 << 24))
                zi = np.ascontiguousarray(z[:, i])
                L.oracle_log_softmax_f32(O.f32p(zi), ARMS, O.f32p(lp), 0)
                action[t, i] = L.oracle_categorical_sample_u(O.f32p(lp), ARMS, C.c_float(u), 0)
                p0 = 1.0 / (1.0 + np.exp(np.float64(zi[1]) - np.float64(zi[0])))
                margin = min(margin, abs(np.float64(u) - p0))
            reward[t], flag[t], obs[:, t + 1], term[:, t] = lanes.step(action[t])
        out.append({"obs": obs, "action": action, "reward": reward, "flag": flag, "term_obs": term})
    observe = lanes.observe()
    driven = lanes.step(driven_actions(n))
    return Reference(out, float(margin), observe, driven)


@functools.lru_cache(maxsize=None)
def reference(case, n=None, offset=None):
    """the case's reference (computed once per process; callers leave it unchanged), optionally at another lane range"""
    n = case.n if n is None else n
    offset = case.offset if offset is None else offset
    return rollout(case.cell, case.H, case.L, case.H2, case.bias, n, case.T, case.E, case.arms, case.seed + 1,
                   case.seed + 2, case_params(case), lane_offset=offset)


def check_data(case, periods):
    """what a case's planes must hold so that it does not pass vacuously"""
    action = np.concatenate([p["action"] for p in periods])
    reward = np.concatenate([p["reward"] for p in periods])
    if case.n > 1:
        assert set(np.unique(action)) == {0, 1}
    assert set(np.unique(reward)) == {0.0, 1.0}
    want = expected_interrupts(case.T, case.E, len(periods))
    for p, planes in enumerate(periods):
        cut = planes["flag"] == M.INTERRUPT
        assert np.array_equal(cut, np.repeat(np.isin(np.arange(case.T), want[p])[:, None], case.n, axis=1)), p
        assert not (planes["flag"] == M.TERMINATE).any()
    if (case.T, case.E) == (13, 3):
        assert want[0] == [4, 9]
    if case.E == 1:
        assert all(w == list(range(case.T)) for w in want)
    if case.E == 10:
        assert want[0] == [] and len(want[1]) == 1
    pos = case.T % (2 * case.E - 1)  # where in its trial a lane stands when period 1 begins
    if pos != 0:
        # the trial that is running ends 2 E - 1 - pos steps into period 1 (where the horizon leaves room): earlier than
        # any trial begun in period 1 could; at an odd position the lane shows the inner episode that has just ended
        first = 2 * case.E - 2 - pos
        assert want[1][:1] == ([first] if first < case.T else [])
        if pos % 2 == 1:
            assert np.all(periods[1]["obs"][0, 0] == 1.0) and np.all(periods[1]["obs"][D - 1, 0] == 1.0)
