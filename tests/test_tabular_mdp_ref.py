"""CPU checks of the tabular-MDP feature: the host sampler rl_random_mdps_sample (called through ctypes, no engine) equals
the Python restatement (tests/tabular_mdp_ref.py) bit for bit; what its samples mean (Dirichlet rows, normals) at the
reference's 4.4 sigma bar for sampling tests (src/spaces/index.rs:379-418); the lane rule on the restatement; the case
tables' own conditions; the ABI names."""
import ctypes as C
import math

import numpy as np
import pytest

import relearn_amd as ra
import tabular_mdp_cases as cases
import tabular_mdp_ref as R

SIGMAS = 4.4


def lib_sample(S, A, alpha, mean, sd, seed, stream):
    cfg = ra.random_mdps_config_default()
    cfg.num_states, cfg.num_actions = S, A
    cfg.transition_prior_dirichlet_alpha, cfg.reward_prior_mean, cfg.reward_prior_stddev = alpha, mean, sd
    return ra.sample_random_mdp(cfg, seed, stream)


def test_config_default_is_the_references():
    c = ra.random_mdps_config_default()
    assert (c.num_states, c.num_actions, c.transition_prior_dirichlet_alpha, c.reward_prior_mean, c.reward_prior_stddev,
            c.discount_factor) == (10, 5, 1.0, 1.0, 1.0, 1.0)


@pytest.mark.parametrize("alpha", [1.0, 0.5, 2.5])
@pytest.mark.parametrize("size", [(2, 2), (8, 8), (10, 5)])
@pytest.mark.parametrize("seed,stream", [(168, 0), (7, 3)])
def test_sampler_bit_parity(alpha, size, seed, stream):
    S, A = size
    tr, mean = lib_sample(S, A, alpha, 1.0, 1.0, seed, stream)
    tr_ref, mean_ref = R.sample_mdp(S, A, alpha, 1.0, 1.0, seed, stream)
    assert np.array_equal(tr.view(np.uint32), tr_ref.view(np.uint32))
    assert np.array_equal(mean.view(np.uint64), mean_ref.view(np.uint64))
    # what the samples are: distributions over the successors
    assert np.all(tr >= 0.0)
    assert np.all(np.abs(tr.astype(np.float64).sum(axis=2) - 1.0) <= 1e-6)


def test_sampler_prior_mean_and_stddev_enter_in_f64():
    tr, mean = lib_sample(3, 2, 1.0, -2.5, 0.25, 11, 1)
    tr_ref, mean_ref = R.sample_mdp(3, 2, 1.0, -2.5, 0.25, 11, 1)
    assert np.array_equal(tr.view(np.uint32), tr_ref.view(np.uint32))
    assert np.array_equal(mean.view(np.uint64), mean_ref.view(np.uint64))
    _, flat = lib_sample(3, 2, 1.0, -2.5, 0.0, 11, 1)
    assert np.all(flat == -2.5)


@pytest.mark.parametrize("field,value", [("num_states", 0), ("num_states", 65), ("num_actions", 0), ("num_actions", 65),
                                         ("transition_prior_dirichlet_alpha", 0.0),
                                         ("transition_prior_dirichlet_alpha", -1.0),
                                         ("transition_prior_dirichlet_alpha", float("nan")),
                                         ("reward_prior_mean", float("inf")), ("reward_prior_stddev", -0.5),
                                         ("reward_prior_stddev", float("nan")), ("discount_factor", float("nan"))])
def test_sampler_refuses(field, value):
    cfg = ra.random_mdps_config_default()
    setattr(cfg, field, value)
    with pytest.raises(ra.RelearnError) as err:
        ra.sample_random_mdp(cfg, 0, 0)
    assert err.value.code == ra.ERR_INVALID_ARGUMENT
    assert field in str(err.value) or "num_states and num_actions" in str(err.value)


def test_sampler_null_pointers():
    cfg = ra.random_mdps_config_default()
    buf = (C.c_double * 4096)()
    L = ra.lib()
    assert L.rl_random_mdps_sample(None, C.c_uint64(0), C.c_uint64(0), buf, buf) == ra.ERR_INVALID_ARGUMENT
    assert L.rl_random_mdps_sample(C.byref(cfg), C.c_uint64(0), C.c_uint64(0), None, buf) == ra.ERR_INVALID_ARGUMENT
    assert L.rl_random_mdps_sample(C.byref(cfg), C.c_uint64(0), C.c_uint64(0), buf, None) == ra.ERR_INVALID_ARGUMENT
    assert L.rl_random_mdps_config_default(None) == ra.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- what the samples mean
# (seeds fixed; the figures are the restatement's, and the library's sampler gives the same bits)
def both_samplers(S, A, alpha, mean, sd, seed, stream):
    tr, m = R.sample_mdp(S, A, alpha, mean, sd, seed, stream)
    tr_lib, m_lib = lib_sample(S, A, alpha, mean, sd, seed, stream)
    assert np.array_equal(tr.view(np.uint32), tr_lib.view(np.uint32)) and np.array_equal(m.view(np.uint64), m_lib.view(np.uint64))
    return tr, m


@pytest.mark.parametrize("alpha,seed", [(1.0, 21), (0.5, 22), (2.5, 23)])
def test_dirichlet_rows_mean_and_variance(alpha, seed):
    S, rows = 4, 2000
    tr = np.concatenate([both_samplers(S, 50, alpha, 0.0, 1.0, seed, k)[0].reshape(-1, S) for k in range(rows // (S * 50))])
    assert tr.shape == (rows, S)
    x = tr.astype(np.float64)
    m, var = 1.0 / S, (S - 1.0) / (S * S * (S * alpha + 1.0))
    # a component is Beta(alpha, (S - 1) alpha): its fourth central moment gives the variance of the sample variance
    a, b = alpha, (S - 1.0) * alpha
    kurt = 3.0 + 6.0 * ((a - b) ** 2 * (a + b + 1.0) - a * b * (a + b + 2.0)) / (a * b * (a + b + 2.0) * (a + b + 3.0))
    se_mean = math.sqrt(var / rows)
    se_var = var * math.sqrt((kurt - 1.0) / rows)
    for j in range(S):
        assert abs(x[:, j].mean() - m) <= SIGMAS * se_mean, (j, x[:, j].mean(), m, se_mean)
        assert abs(x[:, j].var() - var) <= SIGMAS * se_var, (j, x[:, j].var(), var, se_var)


def test_normals_mean_and_variance():
    # the reward means of 20,000 rows under the prior N(0, 1) are 20,000 standard normals
    z = np.concatenate([both_samplers(1, 50, 1.0, 0.0, 1.0, 31, k)[1].reshape(-1) for k in range(400)])
    n = z.size
    assert n == 20000
    assert abs(z.mean()) <= SIGMAS * math.sqrt(1.0 / n), z.mean()
    assert abs(z.var() - 1.0) <= SIGMAS * math.sqrt(2.0 / n), z.var()


def test_restatement_normals_and_gammas_small():
    # the restatement itself, at a size Python affords: 2,000 normals, and Gamma(alpha) means (= alpha, variance alpha)
    rng = R.make_rng(41, 0)
    z = np.array([R.normal(rng)[0] for _ in range(2000)])
    assert abs(z.mean()) <= SIGMAS * math.sqrt(1.0 / 2000) and abs(z.var() - 1.0) <= SIGMAS * math.sqrt(2.0 / 2000)
    for alpha in (0.5, 1.0, 2.5):
        g = np.array([R.gamma(alpha, rng) for _ in range(2000)])
        assert np.all(g > 0.0)
        assert abs(g.mean() - alpha) <= SIGMAS * math.sqrt(alpha / 2000), (alpha, g.mean())


def test_normal_attempt_rule():
    # u = 2 open01 - 1: the all-ones word gives u = 1 - 2^-52, the zero word u = -(1 - 2^-52); both at once: s > 1, refused
    ok, z = R.normal_attempt(0xFFFFFFFFFFFFFFFF, 0)
    assert not ok and z != z  # the value a 64th attempt would take as it is: the square root of a negative number
    # a draw near the origin: accepted, z = u sqrt(-2 ln(s) / s)
    w = 0x8000000000000000  # open01 = 0.5 + 2^-53: u = 2^-52
    ok, z = R.normal_attempt(w, w)
    u = 2.0 ** -52
    assert ok and z == u * math.sqrt(-2.0 * R.rl_log(2.0 * u * u) / (2.0 * u * u))


# ---------------------------------------------------------------- the lane rule on the restatement
def test_boundary_goes_to_the_next_bucket():
    cum = np.array([0.25, 0.5, 1.0], np.float32)
    assert R.successor(cum, 0.25) == 1 and R.successor(cum, 0.2499999) == 0
    assert R.successor(cum, 0.5) == 2 and R.successor(cum, 0.99999994) == 2  # the count cannot leave 0 .. S - 1


def test_cumulative_closes_the_row_at_its_last_positive_entry():
    tr = np.array([[[0.1, 0.2, 0.7, 0.0]] * 2] * 4, np.float32)  # 0.1 + 0.2 + 0.7 rounds below 1 in f32 or not: either way
    cum = R.cumulative(tr)
    assert np.all(cum[..., 2:] == 1.0)
    assert cum[0, 0, 0] == np.float32(0.1) and cum[0, 0, 1] == np.float32(np.float32(0.1) + np.float32(0.2))


def test_zero_probability_successor_is_never_drawn():
    tr, mean, sd = cases.mixed_table()
    lanes = R.MdpLanes(10, tr, mean, np.zeros_like(sd), R.LIMIT_NONE, 0, 0, seed_env=5)
    acts = np.random.RandomState(0).randint(0, 3, size=(10000, 10))
    for t in range(10000):  # 10 lanes x 10,000 steps = 10^5 steps
        before = [lane.state for lane in lanes.lanes]
        lanes.step(acts[t])
        for i, lane in enumerate(lanes.lanes):
            assert tr[before[i], acts[t, i], lane.state] > 0.0


def test_stddev_zero_draws_two_words_per_step():
    tr, mean, sd = cases.random_table(3, 2, 12)
    lanes = R.MdpLanes(4, tr, mean, np.zeros_like(sd), R.LIMIT_LATENT, 5, 0, seed_env=6)
    acts = np.random.RandomState(1).randint(0, 2, size=(50, 4))
    for t in range(50):
        reward, _, _, _ = lanes.step(acts[t])
        assert np.all(lanes.state()[1] == 2 * (t + 1))
    noisy = R.MdpLanes(4, tr, mean, sd, R.LIMIT_LATENT, 5, 0, seed_env=6)
    for t in range(50):
        noisy.step(acts[t])
    pos = noisy.state()[1]
    assert np.all(pos >= 6 * 50) and np.all((pos - 2 * 50) % 4 == 0)  # 2 + 4 x attempts words per step


def test_frequencies_on_the_restatement_at_the_small_size():
    """the GPU test's seed and driver at 256 of its 4,096 lanes"""
    n = cases.FREQ_LANES_CPU
    tr, mean, sd = cases.FREQ_TABLE
    lanes = R.MdpLanes(n, tr, mean, sd, R.LIMIT_NONE, 0, 0, seed_env=cases.FREQ_SEED_ENV)
    acts = cases.freq_actions(n)
    states, nexts, rewards = [], [], []
    for t in range(cases.FREQ_STEPS):
        states.append(lanes.state()[0].astype(np.int64))
        reward, _, _, _ = lanes.step(acts[t])
        nexts.append(lanes.state()[0].astype(np.int64))
        rewards.append(reward)
    worst = cases.check_frequencies(cases.FREQ_TABLE, np.concatenate(states), acts.ravel(), np.concatenate(nexts),
                                    np.concatenate(rewards))
    print("largest deviation: %.2f sigma" % worst)


def test_deterministic_reward_is_the_mean_as_f32():
    tr, mean, sd = cases.mixed_table()
    lane = R.MdpLanes(1, tr, mean, sd, R.LIMIT_NONE, 0, 0, seed_env=8).lanes[0]
    assert sd[0, 0] == 0.0
    r, kind = lane.step(0)
    assert r == np.float32(mean[0, 0]) and kind == R.CONTINUE and lane.env_pos == 2


def test_dynamic_programming_on_a_known_mdp():
    # two states, two actions, horizon 2: action 1 in state 0 pays 0 and moves to state 1, where action 0 pays 10
    tr = np.zeros((2, 2, 2), np.float32)
    tr[0, 0, 0] = tr[0, 1, 1] = tr[1, 0, 1] = tr[1, 1, 0] = 1.0
    mean = np.array([[1.0, 0.0], [10.0, 0.0]])
    opt, uni = R.finite_horizon_values(tr, mean, 2)
    assert opt == 10.0
    assert uni == 0.5 * (1.0 + 0.5 * 1.0) + 0.5 * (0.0 + 0.5 * 10.0)


# ---------------------------------------------------------------- the case tables' own conditions
@pytest.mark.parametrize("name", sorted(list(cases.DRIVEN_CASES) + list(cases.ROLLOUT_CASES)))
def test_gpu_cases_fit_the_lanes(name):
    case = cases.DRIVEN_CASES.get(name) or cases.ROLLOUT_CASES[name]
    assert cases.obs_width(case) <= 8
    (tr, mean, sd), limit, max_steps, _ = case
    assert cases.refusal_reason(dict(transitions=tr, reward_mean=mean, reward_stddev=sd, limit=limit)) is None


def test_driven_cases_cover_what_the_issue_names():
    shapes = {(c[0][0].shape[0], c[0][0].shape[1], c[1], c[2]) for c in cases.DRIVEN_CASES.values()}
    for want in [(2, 2, cases.LIMIT_NONE, 0), (3, 2, cases.LIMIT_LATENT, 7), (8, 8, cases.LIMIT_LATENT, 5),
                 (7, 8, cases.LIMIT_VISIBLE, 5), (5, 3, cases.LIMIT_VISIBLE, 4)]:
        assert want in shapes
    assert any(c[3] == 1000 for c in cases.DRIVEN_CASES.values())
    tr, _, sd = cases.mixed_table()
    assert np.any(sd == 0.0) and np.any(sd > 0.0) and np.any(tr == 0.0) and np.any(np.all((tr == 0.0) | (tr == 1.0), axis=2))


@pytest.mark.parametrize("name", sorted(cases.REFUSAL_CASES))
def test_refusal_cases_are_refused_for_the_reason_named(name):
    args, code, fragment = cases.REFUSAL_CASES[name]
    reason = cases.refusal_reason(args)
    assert reason is not None and fragment in reason
    assert code == cases.ERR_BUILD_ENV


# ---------------------------------------------------------------- ABI
def test_new_symbols_are_exported():
    L = ra.lib()
    for name in ("rl_env_create_tabular_mdp", "rl_random_mdps_config_default", "rl_random_mdps_sample"):
        assert name in ra.ABI_SYMBOLS
        assert hasattr(L, name)
    assert ra.ENV_TABULAR_MDP == 5
    assert ra.lib().rl_abi_version() == 6  # additive: the version stays
