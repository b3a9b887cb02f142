"""The case table of DQN over 3 to 8 actions (rl_dqn_create_finite / ra.FiniteDqn; test infrastructure, not a test), shared
by tests/test_finite_dqn_cases.py (the CPU conditions on it) and tests/test_gpu_finite_dqn.py (the device against the
restatement of tests/finite_dqn_ref.py).

The shapes are the smallest at which the action count can go wrong: 200 lanes (no multiple of 64; the recurrent kernels
also at 64), collections of 9 and 7 steps (episodes are cut by the horizon rule and continue into the next collection),
a replay capacity of 24, and between the envs A = 3, 4, 5, 7 and 8 — 3 and 5 pad the recurrent head's four-row passes, 8
fills two.  A MemoryGame episode is h + 1 steps."""
import collections

SEEDS = dict(seed_env=11, seed_actor=12)
N_LANES, HORIZONS, CAPACITY = 200, (9, 7), 24
MARGIN = 1e-4  # tests/test_gpu_dqn_index_envs.py: the least gap between the two largest action values of a greedy step

# kind "memory": MemoryGame(k, h) [+ a visible step limit]; "bandit": DeterministicBandit::from_values(values).
# D: observation features; A: actions; ep_len: steps per episode as the lanes run it; warm: standalone steps before the
# first collection, chosen so that the first collection's 9 steps (and, where the length allows it, both) end mid-episode
Env = collections.namedtuple("Env", "kind k h limit values D A gamma ep_len warm")
ENVS = {
    "memory-3-1": Env("memory", 3, 1, 0, None, 4, 3, 1.0, 2, 0),              # 4 features, the narrowest
    "memory-3-2": Env("memory", 3, 2, 0, None, 5, 3, 1.0, 3, 1),
    "memory-5-2-visible-2": Env("memory", 5, 2, 2, None, 8, 5, 1.0, 2, 0),    # the second record array, every episode interrupted
    "memory-7-1": Env("memory", 7, 1, 0, None, 8, 7, 1.0, 2, 0),
    "bandit-4": Env("bandit", 0, 0, 0, (0.25, -1.0, 1.5, 0.5), 5, 4, 1.0, 1, 0),
    "bandit-8": Env("bandit", 0, 0, 0, (0.5, -0.25, 1.0, 0.0, -1.0, 2.0, 0.75, 1.5), 5, 8, 1.0, 1, 0),
}

FF_MODULES = {"32-relu": ([32], "Relu"), "16-16-tanh": ([16, 16], "Tanh")}
# cell, recurrent width, layers, MLP hidden width (None: a Linear tail), recurrent bias vectors (recurrent_dqn_ref.Module)
REC_MODULES = {"gru-16-mlp-16": ("gru", 16, 1, 16, True), "lstm-2x8-linear": ("lstm", 8, 2, None, True)}

# (env, module, init seed, lanes).  The seeds are chosen on the CPU (tests/test_finite_dqn_cases.py holds the conditions):
# going down the table, the first from 77 on at which the case's margin holds at every greedy step — no step is left out
# of the comparison — and which, while an action index of the env's A has not been a greedy action yet, adds one.
Case = collections.namedtuple("Case", "env module seed n")
FF_CASES = [
    Case("memory-3-1", "32-relu", 77, N_LANES), Case("memory-3-1", "16-16-tanh", 77, N_LANES),
    Case("memory-3-2", "32-relu", 77, N_LANES), Case("memory-3-2", "16-16-tanh", 77, N_LANES),
    Case("memory-5-2-visible-2", "32-relu", 77, N_LANES), Case("memory-5-2-visible-2", "16-16-tanh", 77, N_LANES),
    Case("memory-7-1", "32-relu", 77, N_LANES), Case("memory-7-1", "16-16-tanh", 77, N_LANES),
    Case("bandit-4", "32-relu", 77, N_LANES), Case("bandit-4", "16-16-tanh", 77, N_LANES),
    Case("bandit-8", "32-relu", 77, N_LANES), Case("bandit-8", "16-16-tanh", 77, N_LANES),
]
REC_CASES = [
    Case("memory-3-1", "gru-16-mlp-16", 77, N_LANES), Case("memory-3-1", "lstm-2x8-linear", 77, 64),
    Case("memory-3-2", "gru-16-mlp-16", 77, 64), Case("memory-3-2", "lstm-2x8-linear", 77, N_LANES),
    Case("memory-5-2-visible-2", "gru-16-mlp-16", 77, N_LANES), Case("memory-5-2-visible-2", "lstm-2x8-linear", 82, N_LANES),
    Case("memory-7-1", "gru-16-mlp-16", 77, N_LANES), Case("memory-7-1", "lstm-2x8-linear", 80, N_LANES),
    Case("bandit-4", "gru-16-mlp-16", 78, N_LANES), Case("bandit-4", "lstm-2x8-linear", 79, N_LANES),
    Case("bandit-8", "gru-16-mlp-16", 77, N_LANES), Case("bandit-8", "lstm-2x8-linear", 78, 64),
]
# a bandit has one observation, so a case has one greedy arm: four more bandit-8 cases, so that every arm of the eight is
# the greedy one once (the same search)
COVER_CASES = [Case("bandit-8", "32-relu", seed, N_LANES) for seed in (78, 79, 81, 87)]
COLLECT_CASES = FF_CASES + REC_CASES + COVER_CASES
EPSILONS = (1.0, 0.5, 0.0)

# minibatches, the SGD step, the all-or-nothing update: one feed-forward and one recurrent case per kind of env
MINIBATCH_CASES = [FF_CASES[3], FF_CASES[4], FF_CASES[7], FF_CASES[10], REC_CASES[3], REC_CASES[4], REC_CASES[6],
                   REC_CASES[8]]
STEP_CASES = [FF_CASES[3], REC_CASES[4]]


def is_recurrent(case):
    return case.module in REC_MODULES


def case_id(case):
    return "%s-%s-s%d-n%d" % (case.env, case.module, case.seed, case.n)
