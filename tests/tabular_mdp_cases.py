"""Case tables of the tabular-MDP lane tests (test infrastructure, not a test), with the reason for each case.
tests/test_tabular_mdp_ref.py checks the tables' own conditions on the CPU; tests/test_gpu_tabular_mdp.py runs them."""
import numpy as np

LIMIT_NONE, LIMIT_LATENT, LIMIT_VISIBLE = 0, 1, 2
ERR_INVALID_ARGUMENT, ERR_BUILD_ENV, ERR_UNSUPPORTED = 1, 5, 10
N_LANES = 70  # one wave plus six lanes, as in the wide-meta tests


def random_table(S, A, seed):
    """a dense table: every successor has positive probability, every reward is noisy (stddev 0.5 .. 1.5)"""
    r = np.random.RandomState(seed)
    tr = r.dirichlet(np.ones(S), size=(S, A)).astype(np.float32)
    mean = r.normal(0.0, 1.0, size=(S, A))
    sd = r.uniform(0.5, 1.5, size=(S, A))
    return tr, mean, sd


def mixed_table():
    """4 states, 3 actions: stddev == 0 beside stddev > 0 (a lane's words per step differ from its neighbour's),
    zero-probability successors in the middle and at the end of a row, and one deterministic row (a single 1, which
    still draws its u64)"""
    tr = np.array([
        [[0.5, 0.0, 0.5, 0.0], [0.0, 1.0, 0.0, 0.0], [0.25, 0.25, 0.25, 0.25]],
        [[0.0, 0.0, 0.75, 0.25], [0.125, 0.875, 0.0, 0.0], [0.0, 0.5, 0.0, 0.5]],
        [[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], [0.5, 0.5, 0.0, 0.0]],
        [[0.0, 0.25, 0.75, 0.0], [0.375, 0.0, 0.0, 0.625], [0.0, 0.0, 1.0, 0.0]],
    ], np.float32)
    mean = np.arange(12, dtype=np.float64).reshape(4, 3) / 4.0 - 1.0
    sd = np.array([[0.0, 1.0, 0.5], [2.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.25, 3.0]])
    return tr, mean, sd


# name -> (tables, limit, max_steps, lane_offset); every case runs 40 driven steps on N_LANES lanes
DRIVEN_CASES = {
    # the smallest MDP and the narrowest observation (2 features); no limit: episodes never end
    "s2a2_none": (random_table(2, 2, 1), LIMIT_NONE, 0, 0),
    # an odd state count, three features; several resets within 40 steps
    "s3a2_latent7": (random_table(3, 2, 2), LIMIT_LATENT, 7, 0),
    # the largest tables: all seven compares of the successor count, eight actions
    "s8a8_latent5": (random_table(8, 8, 3), LIMIT_LATENT, 5, 0),
    # the widest observation: seven states and `remaining` make eight features
    "s7a8_visible5": (random_table(7, 8, 4), LIMIT_VISIBLE, 5, 0),
    # five states: must not take the fused five-state Chain kernels
    "s5a3_visible4": (random_table(5, 3, 5), LIMIT_VISIBLE, 4, 0),
    # streams are keyed by global lane
    "s4a3_offset1000": (random_table(4, 3, 6), LIMIT_LATENT, 6, 1000),
    # words per step differ between lanes; zero-probability successors; a deterministic row
    "s4a3_mixed": (mixed_table(), LIMIT_LATENT, 6, 0),
}

# the rollout cases (70 lanes x T = 12): the narrow one and the widest one
ROLLOUT_CASES = {
    "s3a2": (random_table(3, 2, 7), LIMIT_VISIBLE, 5, 0),
    "s7a8": (random_table(7, 8, 8), LIMIT_VISIBLE, 5, 0),
}


def obs_width(case):
    (tr, _mean, _sd), limit, _max_steps, _off = case
    return tr.shape[0] + (1 if limit == LIMIT_VISIBLE else 0)


def _with(tr=None, mean=None, sd=None, limit=LIMIT_LATENT, max_steps=5, S=3, A=2):
    t, m, s = random_table(S, A, 9)
    return dict(transitions=t if tr is None else tr, reward_mean=m if mean is None else mean,
                reward_stddev=s if sd is None else sd, limit=limit, max_steps=max_steps)


def _poke(which, index, value, S=3, A=2):
    t, m, s = random_table(S, A, 9)
    arr = {"tr": t, "mean": m, "sd": s}[which]
    arr[index] = value
    return _with(tr=t, mean=m, sd=s)


def _bad_row(delta):
    t, m, s = random_table(3, 2, 9)
    t[1, 1] = np.array([0.5, 0.25, 0.25 + delta], np.float32)
    return _with(tr=t, mean=m, sd=s)


# name -> (constructor arguments, status code, a fragment of the message that names the reason)
REFUSAL_CASES = {
    "one_state": (_with(*random_table(1, 2, 9), S=1), ERR_BUILD_ENV, "n_states 2..8"),
    "nine_states": (_with(*random_table(9, 2, 9), S=9), ERR_BUILD_ENV, "n_states 2..8"),
    "one_action": (_with(*random_table(3, 1, 9), A=1), ERR_BUILD_ENV, "n_actions 2..8"),
    "nine_actions": (_with(*random_table(3, 9, 9), A=9), ERR_BUILD_ENV, "n_actions 2..8"),
    # the reference's default size: the lanes end at 8
    "reference_default_10x5": (_with(*random_table(10, 5, 9)), ERR_BUILD_ENV, "n_states 2..8"),
    "eight_states_visible": (_with(*random_table(8, 2, 9), limit=LIMIT_VISIBLE), ERR_BUILD_ENV, "VisibleStepLimit"),
    "negative_probability": (_poke("tr", (0, 1, 2), -0.125), ERR_BUILD_ENV, "negative or not finite"),
    "nan_probability": (_poke("tr", (2, 0, 0), np.nan), ERR_BUILD_ENV, "negative or not finite"),
    "inf_probability": (_poke("tr", (2, 0, 0), np.inf), ERR_BUILD_ENV, "negative or not finite"),
    "row_sum_high": (_bad_row(3e-5), ERR_BUILD_ENV, "does not sum to 1"),
    "row_sum_low": (_bad_row(-3e-5), ERR_BUILD_ENV, "does not sum to 1"),
    "nan_mean": (_poke("mean", (1, 0), np.nan), ERR_BUILD_ENV, "mean is not finite"),
    "inf_mean": (_poke("mean", (1, 0), -np.inf), ERR_BUILD_ENV, "mean is not finite"),
    "negative_stddev": (_poke("sd", (2, 1), -1.0), ERR_BUILD_ENV, "stddev is negative or not finite"),
    "nan_stddev": (_poke("sd", (2, 1), np.nan), ERR_BUILD_ENV, "stddev is negative or not finite"),
}


def refusal_reason(args):
    """why rl_env_create_tabular_mdp must refuse `args`, by the rules of include/relearn_hip.h in their order (None: it
    must not) — the cases' own check, independent of the library"""
    tr = np.asarray(args["transitions"], np.float32)
    mean = np.asarray(args["reward_mean"], np.float64)
    sd = np.asarray(args["reward_stddev"], np.float64)
    S, A = tr.shape[0], tr.shape[1]
    if not (2 <= S <= 8 and 2 <= A <= 8):
        return "n_states 2..8 and n_actions 2..8"
    if S + (1 if args["limit"] == LIMIT_VISIBLE else 0) > 8:
        return "VisibleStepLimit"
    for s in range(S):
        for a in range(A):
            row = tr[s, a]
            if not np.all(np.isfinite(row)) or np.any(row < 0):
                return "negative or not finite"
            acc = np.float32(0.0)
            for p in row:
                acc = np.float32(acc + p)
            if not abs(float(acc) - 1.0) <= 1e-5:
                return "does not sum to 1"
            if not np.isfinite(mean[s, a]):
                return "mean is not finite"
            if not np.isfinite(sd[s, a]) or sd[s, a] < 0:
                return "stddev is negative or not finite"
    return None


# ---------------------------------------------------------------- the frequency case
# 4,096 lanes x 64 steps on a (4, 2) table under a uniform-random driver, no limit.  The restatement passes at 256 lanes
# (the first 256 of the same lanes: streams are keyed by global lane) with this seed, tests/test_tabular_mdp_ref.py.
FREQ_TABLE = random_table(4, 2, 10)
FREQ_SEED_ENV, FREQ_STEPS, FREQ_LANES, FREQ_LANES_CPU = 14, 64, 4096, 256
SIGMAS = 4.4  # the reference's bar for sampling tests (src/spaces/index.rs:379-418)


def freq_actions(n):
    return np.random.RandomState(15).randint(0, 2, size=(FREQ_STEPS, FREQ_LANES))[:, :n].astype(np.uint8)


def check_frequencies(table, states, actions, nexts, rewards):
    """every (s, a, s') count and every (s, a) reward mean and variance within 4.4 sigma of the table's; the arguments are
    flat arrays over all steps.  -> the largest deviation seen, in sigmas"""
    tr, mean, sd = table
    S, A = tr.shape[0], tr.shape[1]
    worst = 0.0
    for s in range(S):
        for a in range(A):
            m = (states == s) & (actions == a)
            N = int(m.sum())
            assert N > 100, (s, a, N)
            for j in range(S):
                p = float(tr[s, a, j])
                k = int((nexts[m] == j).sum())
                dev = abs(k - N * p) / np.sqrt(N * p * (1.0 - p))
                assert dev <= SIGMAS, ("count", s, a, j, k, N * p, dev)
                worst = max(worst, dev)
            r = rewards[m].astype(np.float64)
            dev_m = abs(r.mean() - mean[s, a]) / (sd[s, a] / np.sqrt(N))
            dev_v = abs(r.var(ddof=1) - sd[s, a] ** 2) / (sd[s, a] ** 2 * np.sqrt(2.0 / (N - 1)))
            assert dev_m <= SIGMAS and dev_v <= SIGMAS, ("reward", s, a, r.mean(), mean[s, a], r.var(ddof=1), sd[s, a] ** 2)
            worst = max(worst, dev_m, dev_v)
    return worst
