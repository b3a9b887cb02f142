"""The bandit baselines on the meta-bandit lanes (rl_bandit_agent_*, kernels_bandit_agent.hip: ResettingMetaAgent over
Random / tabular Q-learning / UCB1, src/agents/meta.rs:135-199) against the Python restatement
tests/bandit_agents_ref.py, bit for bit: every case takes TWO collections on one env and one agent and compares, after
each, every plane, the agent's state and actor word position, and afterwards the env's observation and one driven step.
TERM_OBS is compared where a trial was cut by its Interrupt — what rl_rollout defines of that plane."""
import ctypes as C
import math

import numpy as np
import pytest

import bandit_agents_ref as B
import meta_lanes_ref as M
import oracle as O
import relearn_amd as ra

pytestmark = pytest.mark.gpu
L = O.lib()

# (name, kind, exploration_rate, initial_action_count, initial_action_value); None = the reference's default
RANDOM = ("random", B.RANDOM, None, None, None)
GREEDY = ("greedy", B.TABULAR_Q, 0.0, 2, 0.5)      # the experiment's Greedy
EPS_GREEDY = ("eps_greedy", B.TABULAR_Q, 0.2, 2, 0.5)  # the experiment's EpsGreedy
EXPLORER = ("tabular_q_rate_1", B.TABULAR_Q, 1.0, None, None)  # always explores; the default priors (0, 0.0)
UCB1 = ("ucb1", B.UCB1, None, None, None)
AGENTS = [RANDOM, GREEDY, EPS_GREEDY, EXPLORER, UCB1]
IDS = [a[0] for a in AGENTS]


def same_planes(got, want, where):
    for key in ("obs", "action", "reward", "flag"):
        assert np.array_equal(got[key], want[key]), (where, key)
    cut = got["flag"] == M.INTERRUPT
    assert np.array_equal(got["term_obs"][:, cut], want["term_obs"][:, cut]), (where, "term_obs")


def same_state(agent, ref, k, E, where):
    got, want = agent.state(), ref.state()
    assert set(got) - {"ln_table"} == set(want), where
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (where, key)
    if "ln_table" in got:
        assert np.array_equal(got["ln_table"], B.ln_table(k, E)), where
        assert got["ln_table"][0] == 2.0 * math.log(float(2 * k))


def two_collections(engine, agent_spec, dist, k, E, T, n, lane_offset=0, seed=3, reset_between=False):
    """-> (planes of both collections, the agent's final state); every comparison against the restatement is made here"""
    _, kind, rate, count, value = agent_spec
    env = ra.MetaBanditEnv(engine, n, k, E, dist, lane_offset=lane_offset, seed_env=seed, seed_actor=seed + 1)
    agent = ra.BanditAgent(env, kind, rate, count, value)
    traj = ra.Trajectory(engine, n, T, env.D)
    ref_env = M.MetaLanes(n, k, E, dist, lane_offset=lane_offset, seed_env=seed)
    ref = B.BanditAgentLanes(n, k, kind, rate, count, value, lane_offset=lane_offset, seed_actor=seed + 1)
    same_state(agent, ref, k, E, "created")
    planes = []
    for period in range(2):
        if period == 1 and reset_between:
            env.reset(), ref_env.reset()
        agent.rollout(env, traj)
        got = traj.read_all()
        same_planes(got, ref.rollout(ref_env, T), period)
        same_state(agent, ref, k, E, period)
        planes.append(got)
    assert np.array_equal(env.observe(), ref_env.observe())
    a = (np.arange(n) % k).astype(np.uint8)
    reward, flag, obs, term = env.step(a)
    reward_o, flag_o, obs_o, term_o = ref_env.step(a)
    assert np.array_equal(reward, reward_o) and np.array_equal(flag, flag_o) and np.array_equal(obs, obs_o)
    assert np.array_equal(term[:, flag == M.INTERRUPT], term_o[:, flag_o == M.INTERRUPT])
    return planes, agent.state()


# ------------------------------------------------------------------------------------------------ 1. kinds x arms
@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("dist", [M.UNIFORM_BERNOULLI, M.ONE_HOT, M.ROUND_ROBIN])
@pytest.mark.parametrize("spec", AGENTS, ids=IDS)
def test_kinds_distributions_arms(engine, spec, dist, k):
    """45 lanes, 3 episodes per trial, T = 7 against trials of 5 steps: the horizon cuts the second trial after its first
    pull and restart, the second collection finishes it (the agent's state carries over) and starts two more"""
    planes, state = two_collections(engine, spec, dist, k, 3, 7, 45)
    flags = np.concatenate([p["flag"] for p in planes])
    assert np.array_equal(np.nonzero((flags == M.INTERRUPT).all(axis=1))[0], [4, 9])
    actions = np.concatenate([p["action"] for p in planes])
    pulls = np.concatenate([p["obs"][0, :-1] for p in planes]) == 0.0
    assert np.all(actions[~pulls] == 0)  # every restart step records action 0
    if spec[1] == B.UCB1:
        assert np.all(actions[[0, 5, 10]] == k - 1)  # the first pull of every trial: the LAST maximal index
        assert np.all(state["pos"] == 0)
    if spec is GREEDY:
        assert np.all(actions[[0, 5, 10]] == 0)  # ... and the FIRST
        assert np.all(state["pos"] == 2 * np.count_nonzero(pulls, axis=0))  # one f64 per pull, also at rate 0
    if spec is RANDOM or spec is EXPLORER:
        assert actions[pulls].max() == k - 1 and actions[pulls].min() == 0


# ------------------------------------------------------------------------------------------------ 2. trial lengths, horizons
@pytest.mark.parametrize("E", [1, 3, 10])
@pytest.mark.parametrize("spec", [EPS_GREEDY, UCB1], ids=["eps_greedy", "ucb1"])
def test_episodes_per_trial_and_horizons(engine, spec, E):
    """E = 1 restarts the agent at every step.  Horizons: one step; 7 (no multiple of a trial); one trial exactly
    (T = 2 E - 1: the last pull's update is in the state read back, the next collection starts fresh); more than two
    trials.  65 lanes: two workgroups, the second with one lane"""
    for T in sorted({1, 7, 2 * E - 1, 2 * (2 * E - 1) + 3}):
        two_collections(engine, spec, M.UNIFORM_BERNOULLI, 3, E, T, 65, seed=20 + E)


# ------------------------------------------------------------------------------------------------ 3. lanes
@pytest.mark.parametrize("n", [1, 45, 64, 65, 130])
def test_lane_counts(engine, n):
    two_collections(engine, EPS_GREEDY, M.UNIFORM_BERNOULLI, 2, 3, 7, n, seed=31)
    two_collections(engine, UCB1, M.ONE_HOT, 4, 3, 7, n, seed=32)


def test_lane_offset(engine):
    """lanes 25..69 of a 70-lane run are the 45-lane run at lane_offset 25: both random streams are keyed by the global
    lane id"""
    for spec, dist in ((EPS_GREEDY, M.UNIFORM_BERNOULLI), (RANDOM, M.ONE_HOT)):
        whole, st_w = two_collections(engine, spec, dist, 3, 3, 7, 70, seed=41)
        part, st_p = two_collections(engine, spec, dist, 3, 3, 7, 45, lane_offset=25, seed=41)
        for period in range(2):
            for key in ("obs", "action", "reward", "flag"):
                assert np.array_equal(whole[period][key][..., 25:], part[period][key]), (period, key)
        for key in st_p:
            if key != "ln_table":
                assert np.array_equal(st_w[key][..., 25:], st_p[key]), key


# ------------------------------------------------------------------------------------------------ 4. reset between collections
@pytest.mark.parametrize("spec", AGENTS, ids=IDS)
def test_env_reset_in_the_middle_of_a_trial(engine, spec):
    """T = 7 at trials of 5 steps leaves every lane two steps into a trial; rl_env_reset starts a new trial, and with it
    a fresh inner agent — by the env's state, no call on the agent — while the actor word position carries on"""
    planes, state = two_collections(engine, spec, M.UNIFORM_BERNOULLI, 3, 3, 7, 45, seed=51, reset_between=True)
    assert np.array_equal(np.nonzero((planes[1]["flag"] == M.INTERRUPT).all(axis=1))[0], [4])
    if spec[1] == B.UCB1:
        assert np.all(planes[1]["action"][0] == 2)  # a fresh UCB1 agent's first pull
        assert np.all(state["pos"] == 0)
    else:  # the draws of the first collection are not taken again
        assert np.all(state["pos"] > 0) and np.all(state["pos"] % 2 == 0)


# ------------------------------------------------------------------------------------------------ 5. hand-over to a policy
def test_a_policy_rollout_after_a_baseline_collection(engine):
    """the env state and the step counter are handed over whole: a feed-forward policy's rollout on the same env equals
    the restated env driven by the recorded actions, and its draws are words T0 + t of the actor stream"""
    n, k, E, T0, T1, seed = 45, 3, 3, 7, 6, 61
    env = ra.MetaBanditEnv(engine, n, k, E, seed_env=seed, seed_actor=seed + 1)
    agent = ra.BanditAgent(env, "ucb1")
    traj0, traj1 = ra.Trajectory(engine, n, T0, env.D), ra.Trajectory(engine, n, T1, env.D)
    agent.rollout(env, traj0)
    ref_env = M.MetaLanes(n, k, E, seed_env=seed)
    ref_env.replay(traj0.read(ra.TRAJ_ACTION))
    pol = ra.Mlp(engine, env.D, [32], k)
    pol.init(7)
    ra.rollout(env, pol, traj1)
    got = traj1.read_all()
    same_planes(got, dict(ref_env.replay(got["action"]), action=got["action"]), "policy rollout")
    for t in (0, 3):
        x = np.ascontiguousarray(got["obs"][:, t, :].T)
        z = pol.forward(x)
        for i in range(n):
            w = engine.stream_words(seed + 1, i, T0 + t, 1)[0]
            u = np.float32(w >> 8) * np.float32(1.0 / (1 << 24))
            lp = np.zeros(k, dtype=np.float32)
            L.oracle_log_softmax_f32(O.f32p(np.ascontiguousarray(z[i].astype(np.float32))), k, O.f32p(lp), 0)
            assert got["action"][t, i] == L.oracle_categorical_sample_u(O.f32p(lp), k, C.c_float(u), 0), (t, i)


# ------------------------------------------------------------------------------------------------ 6. the guard's words
def test_policy_gradient_on_collected_and_written_planes(engine):
    """a baseline-collected trajectory and one filled from the same planes through rl_traj_write give rl_policy_gradient
    of a feed-forward policy the same bits"""
    n, k, E, T = 70, 2, 3, 13
    env = ra.MetaBanditEnv(engine, n, k, E, seed_env=71, seed_actor=72)
    agent = ra.BanditAgent(env, "tabular_q", 0.2, 2, 0.5)
    adv = np.random.default_rng(5).standard_normal((T, n)).astype(np.float32)
    results = []
    planes = None
    for source in ("collected", "written"):
        pol = ra.Mlp(engine, env.D, [32], k)
        pol.init(9)
        traj = ra.Trajectory(engine, n, T, env.D)
        if source == "collected":
            agent.rollout(env, traj)
            planes = traj.read_all()
        else:
            traj.write_all(planes)
        traj.write(ra.TRAJ_ADVANTAGES, adv)
        results.append(ra.policy_gradient(pol, traj))
    (g0, loss0, ent0), (g1, loss1, ent1) = results
    assert np.array_equal(g0, g1) and loss0 == loss1 and ent0 == ent1
    assert np.abs(g0).max() > 0 and set(np.unique(planes["action"])) == {0, 1}


# ------------------------------------------------------------------------------------------------ 7. StepsSummary
def test_steps_summary_of_a_baseline_collection(engine):
    n, k, E, T = 70, 3, 3, 13
    env = ra.MetaBanditEnv(engine, n, k, E, seed_env=81, seed_actor=82)
    agent = ra.BanditAgent(env, "ucb1")
    traj = ra.Trajectory(engine, n, T, env.D)
    agent.rollout(env, traj)
    summary = ra.StepsSummary(engine, n)
    summary.push(traj)
    stats = summary.read()
    flag, reward = traj.read(ra.TRAJ_FLAG), traj.read(ra.TRAJ_REWARD).astype(np.float64)
    sums, lens = [], []
    for i in range(n):
        acc, length = 0.0, 0
        for t in range(T):
            acc, length = acc + reward[t, i], length + 1
            if flag[t, i] != M.CONTINUE:
                sums.append(acc), lens.append(length)
                acc, length = 0.0, 0
    assert stats.episode_reward.count == len(sums) == 2 * n
    assert abs(stats.episode_reward.mean - np.mean(sums)) < 1e-12
    assert abs(stats.episode_reward.stddev() - np.std(sums)) < 1e-12
    assert stats.episode_length.mean == 2 * E - 1 and set(lens) == {2 * E - 1}
    assert stats.step_reward.count == n * T and abs(stats.step_reward.mean - reward.mean()) < 1e-12


# ------------------------------------------------------------------------------------------------ 8. refusals
def raw_create(env, **fields):
    cfg = ra.bandit_agent_config_default(fields.pop("kind", ra.BANDIT_AGENT_TABULAR_Q))
    for name, v in fields.items():
        setattr(cfg, name, v)
    h = C.c_void_p()
    code = ra.lib().rl_bandit_agent_create(env.h, C.byref(cfg), C.byref(h))
    msg = ra.lib().rl_last_error(env.eng.h).decode() if code != ra.OK else ""
    if code == ra.OK:
        ra.lib().rl_bandit_agent_destroy(h)
    return code, msg


def code_of(f):
    with pytest.raises(ra.RelearnError) as e:
        f()
    return e.value.code, str(e.value)


def test_refusals(engine):
    n, k, E = 8, 3, 4
    env = ra.MetaBanditEnv(engine, n, k, E)
    lib = ra.lib()
    # create
    code, msg = raw_create(ra.ChainEnv(engine, n))
    assert code == ra.ERR_UNSUPPORTED and "rl_bandit_agent_create" in msg
    h = C.c_void_p()
    assert lib.rl_bandit_agent_create(env.h, None, C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    assert lib.rl_bandit_agent_create(env.h, C.byref(ra.bandit_agent_config_default("ucb1")), None) == ra.ERR_INVALID_ARGUMENT
    for fields, name in ((dict(exploration_rate=-0.1), "exploration_rate"),
                         (dict(exploration_rate=float("nan")), "exploration_rate"),
                         (dict(exploration_rate=float("inf")), "exploration_rate"),
                         (dict(exploration_rate=1.5), "exploration_rate"),
                         (dict(kind=ra.BANDIT_AGENT_UCB1, exploration_rate=-1.0), "exploration_rate"),
                         (dict(kind=ra.BANDIT_AGENT_UCB1, exploration_rate=float("inf")), "exploration_rate"),
                         (dict(initial_action_value=-0.5), "initial_action_value"),
                         (dict(initial_action_value=float("nan")), "initial_action_value"),
                         (dict(reserved=1), "reserved"), (dict(kind=ra.BANDIT_AGENT_UCB1, reserved=-1), "reserved")):
        code, msg = raw_create(env, **fields)
        assert code == ra.ERR_INVALID_ARGUMENT and name in msg, (fields, msg)
    cfg = ra.bandit_agent_config_default("ucb1")
    cfg.kind = 3
    assert lib.rl_bandit_agent_create(env.h, C.byref(cfg), C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    assert raw_create(env, kind=ra.BANDIT_AGENT_UCB1, exploration_rate=1.5)[0] == ra.OK  # a scale, not a probability
    assert raw_create(env, exploration_rate=1.0)[0] == ra.OK
    # the table's bound
    long_env = ra.MetaBanditEnv(engine, n, 2, (1 << 20) + 1)
    code, msg = raw_create(long_env, kind=ra.BANDIT_AGENT_UCB1)
    assert code == ra.ERR_UNSUPPORTED and "1048576" in msg
    assert raw_create(long_env, kind=ra.BANDIT_AGENT_TABULAR_Q)[0] == ra.OK  # the bound is the table's
    at_bound = ra.BanditAgent(ra.MetaBanditEnv(engine, n, 2, 1 << 20), "ucb1")
    assert at_bound.read(ra.BANDIT_STATE_LN_TABLE)[-1] == 2.0 * math.log(float(4 + (1 << 20) - 1))
    # rollout
    agent = ra.BanditAgent(env, "ucb1")
    traj = ra.Trajectory(engine, n, 5, env.D)
    for other in (ra.MetaBanditEnv(engine, n, k, E + 1), ra.MetaBanditEnv(engine, n, k - 1, E),
                  ra.MetaBanditEnv(engine, n + 1, k, E)):
        code, msg = code_of(lambda: agent.rollout(other, ra.Trajectory(engine, other.n, 5, other.D)))
        assert code == ra.ERR_INVALID_ARGUMENT and "rl_bandit_agent_rollout" in msg
    for bad in (ra.Trajectory(engine, n + 1, 5, env.D), ra.Trajectory(engine, n, 5, env.D - 1)):
        code, msg = code_of(lambda: agent.rollout(env, bad))
        assert code == ra.ERR_INVALID_ARGUMENT and "trajectory shape does not match the env" in msg
    assert lib.rl_bandit_agent_rollout(agent.h, env.h, None) == ra.ERR_INVALID_ARGUMENT
    assert lib.rl_bandit_agent_rollout(None, env.h, traj.h) == ra.ERR_INVALID_ARGUMENT
    agent.rollout(env, traj)  # ... and the handle still works
    # state_read
    buf = np.zeros(k * n + 1, np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)

    def read(a, field, nbytes):
        return lib.rl_bandit_agent_state_read(a.h, C.c_int32(field), p, C.c_uint64(nbytes))

    assert read(agent, ra.BANDIT_STATE_ACTOR_POS, 8 * n) == ra.OK
    assert read(agent, ra.BANDIT_STATE_ACTOR_POS, 8 * n + 8) == ra.ERR_INVALID_ARGUMENT
    assert read(agent, ra.BANDIT_STATE_COUNTS, 8 * n) == ra.ERR_INVALID_ARGUMENT
    assert read(agent, ra.BANDIT_STATE_LN_TABLE, 8 * E) == ra.OK
    assert read(agent, 5, 8 * n) == ra.ERR_INVALID_ARGUMENT and read(agent, -1, 8 * n) == ra.ERR_INVALID_ARGUMENT
    assert lib.rl_bandit_agent_state_read(agent.h, C.c_int32(0), None, C.c_uint64(8 * n)) == ra.ERR_INVALID_ARGUMENT
    tab, rnd = ra.BanditAgent(env, "tabular_q"), ra.BanditAgent(env, "random")
    assert read(tab, ra.BANDIT_STATE_COUNTS, 8 * k * n) == ra.OK and read(tab, ra.BANDIT_STATE_VALUES, 8 * k * n) == ra.OK
    for a, field, nbytes in ((tab, ra.BANDIT_STATE_VISITS, 8 * n), (tab, ra.BANDIT_STATE_LN_TABLE, 8 * E),
                             (rnd, ra.BANDIT_STATE_COUNTS, 8 * k * n), (rnd, ra.BANDIT_STATE_VALUES, 8 * k * n),
                             (rnd, ra.BANDIT_STATE_VISITS, 8 * n), (rnd, ra.BANDIT_STATE_LN_TABLE, 8 * E)):
        assert read(a, field, nbytes) == ra.ERR_INVALID_ARGUMENT, (field, nbytes)
        assert "no such field" in lib.rl_last_error(engine.h).decode()
    assert read(rnd, ra.BANDIT_STATE_ACTOR_POS, 8 * n) == ra.OK


# ------------------------------------------------------------------------------------------------ 9. the reference's test
def test_the_references_ucb_test_on_the_device(engine):
    """src/agents/meta.rs:238-264 — OneHot(3), 20 episodes per trial, UCB1 0.2 — as 8 lanes x 125 steps: mean reward of
    the completed trials > 0.7 * (20 - 3) = 11.9; by the last-maximal-index rule every one of them earns at least 18"""
    n, T = 8, 125
    env = ra.MetaBanditEnv(engine, n, 3, 20, "one_hot", seed_env=221, seed_actor=0)
    agent = ra.BanditAgent(env, "ucb1")
    traj = ra.Trajectory(engine, n, T, env.D)
    agent.rollout(env, traj)
    reward, flag = traj.read(ra.TRAJ_REWARD).astype(np.float64), traj.read(ra.TRAJ_FLAG)
    totals = []
    for i in range(n):
        acc = 0.0
        for t in range(T):
            acc += reward[t, i]
            if flag[t, i] == M.INTERRUPT:
                totals.append(acc)
                acc = 0.0
    assert len(totals) == n * (T // 39)
    assert np.mean(totals) > 11.9
    assert min(totals) >= 18


# ------------------------------------------------------------------------------------------------ 10. one statistical line
def test_ucb1_beats_random(engine):
    """4,096 lanes, UniformBernoulli(2), 10 episodes per trial, one trial each: a plain-Python simulation of the rules
    gives 6.00 (UCB1) against 5.02 (RANDOM) with a standard error of 0.044 each at 4,000 trials; the bar of 0.5 lies
    eleven standard errors below that gap"""
    n, E = 4096, 10
    means = {}
    for kind in ("ucb1", "random"):
        env = ra.MetaBanditEnv(engine, n, 2, E, seed_env=91, seed_actor=92)
        agent = ra.BanditAgent(env, kind)
        traj = ra.Trajectory(engine, n, 2 * E - 1, env.D)
        agent.rollout(env, traj)
        assert np.all(traj.read(ra.TRAJ_FLAG)[-1] == M.INTERRUPT)
        means[kind] = traj.read(ra.TRAJ_REWARD).astype(np.float64).sum(axis=0).mean()
    print("mean trial reward: UCB1 %.3f, RANDOM %.3f" % (means["ucb1"], means["random"]))
    assert means["ucb1"] - means["random"] > 0.5
