"""The Thompson-sampling baseline on the meta-bandit lanes (RL_BANDIT_AGENT_THOMPSON, kernels_bandit_agent.hip:
ResettingMetaAgent over BetaThompsonSamplingAgentConfig, src/agents/bandits/thompson_sampling.rs:95-136, 186-205; DESIGN.md
§33) against the Python restatement tests/thompson_ref.py, bit for bit: every case takes TWO collections on one env and
one agent and compares, after each, every plane, the low and high counts and the actor word position, and afterwards
the env's observation and one driven step.  Every action compared is the argmax over sums of Beta samples the device
drew with its own rl_log / rl_exp: one differing bit in either shows as another action or another word position.

Tried on scratch builds with one wrong line each: alpha and beta exchanged in Beta::new fails 41 of the 44 cases, the
ChaCha block cache not refilled at a block boundary 43.  The FIRST maximal sum instead of the last fails none: two sums
of continuous samples do not tie, so that rule cannot be seen through drawn samples (tests/test_thompson_ref.py holds
it on given ones, in the restatement)."""
import ctypes as C

import numpy as np
import pytest

import bandit_agents_ref as B
import meta_lanes_ref as M
import relearn_amd as ra
import thompson_ref as TR

pytestmark = pytest.mark.gpu


def same_planes(got, want, where):
    for key in ("obs", "action", "reward", "flag"):
        assert np.array_equal(got[key], want[key]), (where, key)
    cut = got["flag"] == M.INTERRUPT
    assert np.array_equal(got["term_obs"][:, cut], want["term_obs"][:, cut]), (where, "term_obs")


def same_state(agent, ref, where):
    got, want = agent.state(), ref.state()
    assert set(got) == set(want) == {"pos", "low", "high"}, where
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (where, key)


def two_collections(engine, num_samples, dist, k, E, T, n, lane_offset=0, seed=3, reset_between=False):
    """-> (planes of both collections, the agent's final state); every comparison against the restatement is made here"""
    env = ra.MetaBanditEnv(engine, n, k, E, dist, lane_offset=lane_offset, seed_env=seed, seed_actor=seed + 1)
    agent = ra.BanditAgent(env, "thompson", num_samples=num_samples)
    traj = ra.Trajectory(engine, n, T, env.D)
    ref_env = M.MetaLanes(n, k, E, dist, lane_offset=lane_offset, seed_env=seed)
    ref = TR.ThompsonAgentLanes(n, k, num_samples, lane_offset=lane_offset, seed_actor=seed + 1)
    same_state(agent, ref, "created")
    planes = []
    for period in range(2):
        if period == 1 and reset_between:
            env.reset(), ref_env.reset()
        agent.rollout(env, traj)
        got = traj.read_all()
        same_planes(got, ref.rollout(ref_env, T), period)
        same_state(agent, ref, period)
        planes.append(got)
    assert np.array_equal(env.observe(), ref_env.observe())
    a = (np.arange(n) % k).astype(np.uint8)
    reward, flag, obs, term = env.step(a)
    reward_o, flag_o, obs_o, term_o = ref_env.step(a)
    assert np.array_equal(reward, reward_o) and np.array_equal(flag, flag_o) and np.array_equal(obs, obs_o)
    assert np.array_equal(term[:, flag == M.INTERRUPT], term_o[:, flag_o == M.INTERRUPT])
    return planes, agent.state()


# ------------------------------------------------------------------------------------------------ 1. samples x arms
@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("dist", [M.UNIFORM_BERNOULLI, M.ONE_HOT, M.ROUND_ROBIN])
@pytest.mark.parametrize("num_samples", [1, 3, 10])
def test_samples_distributions_arms(engine, num_samples, dist, k):
    """45 lanes, 3 episodes per trial, T = 7 against trials of 5 steps: the horizon cuts the second trial after its first
    pull and restart, the second collection finishes it (the counts carry over) and starts two more"""
    planes, state = two_collections(engine, num_samples, dist, k, 3, 7, 45)
    flags = np.concatenate([p["flag"] for p in planes])
    assert np.array_equal(np.nonzero((flags == M.INTERRUPT).all(axis=1))[0], [4, 9])
    actions = np.concatenate([p["action"] for p in planes])
    pulls = np.concatenate([p["obs"][0, :-1] for p in planes]) == 0.0
    assert np.all(actions[~pulls] == 0)  # every restart step records action 0
    assert actions[pulls].max() == k - 1 and actions[pulls].min() == 0
    # 4 words per attempt, at least one attempt per sample, k * num_samples samples per pull
    assert np.all(state["pos"] % 4 == 0)
    assert np.all(state["pos"] >= 4 * k * num_samples * np.count_nonzero(pulls, axis=0))
    # the trial in progress after 14 steps has had 2 pulls
    assert np.all(state["low"].sum(axis=0) + state["high"].sum(axis=0) == 2 * k + 2)


# ------------------------------------------------------------------------------------------------ 2. trial lengths, horizons
@pytest.mark.parametrize("E", [1, 3, 10])
@pytest.mark.parametrize("num_samples", [1, 10])
def test_episodes_per_trial_and_horizons(engine, num_samples, E):
    """E = 1 restarts the agent at every step.  Horizons: one step; 7 (no multiple of a trial); one trial exactly
    (T = 2 E - 1: the last pull's update is in the counts read back, the next collection starts fresh); more than two
    trials.  65 lanes: two workgroups, the second with one lane"""
    for T in sorted({1, 7, 2 * E - 1, 2 * (2 * E - 1) + 3}):
        two_collections(engine, num_samples, M.UNIFORM_BERNOULLI, 3, E, T, 65, seed=20 + E)


# ------------------------------------------------------------------------------------------------ 3. lanes
@pytest.mark.parametrize("n", [1, 45, 64, 65, 130])
def test_lane_counts(engine, n):
    two_collections(engine, 1, M.UNIFORM_BERNOULLI, 2, 3, 7, n, seed=31)
    two_collections(engine, 3, M.ONE_HOT, 4, 3, 7, n, seed=32)


def test_lane_offset(engine):
    """lanes 25..69 of a 70-lane run are the 45-lane run at lane_offset 25: both random streams are keyed by the global
    lane id"""
    for num_samples, dist in ((1, M.UNIFORM_BERNOULLI), (10, M.ONE_HOT)):
        whole, st_w = two_collections(engine, num_samples, dist, 3, 3, 7, 70, seed=41)
        part, st_p = two_collections(engine, num_samples, dist, 3, 3, 7, 45, lane_offset=25, seed=41)
        for period in range(2):
            for key in ("obs", "action", "reward", "flag"):
                assert np.array_equal(whole[period][key][..., 25:], part[period][key]), (period, key)
        for key in st_p:
            assert np.array_equal(st_w[key][..., 25:], st_p[key]), key


# ------------------------------------------------------------------------------------------------ 4. reset between collections
@pytest.mark.parametrize("num_samples", [1, 10])
def test_env_reset_in_the_middle_of_a_trial(engine, num_samples):
    """T = 7 at trials of 5 steps leaves every lane two steps into a trial; rl_env_reset starts a new trial, and with it
    a fresh inner agent — by the env's state, no call on the agent — while the actor word position carries on"""
    planes, state = two_collections(engine, num_samples, M.UNIFORM_BERNOULLI, 3, 3, 7, 45, seed=51, reset_between=True)
    assert np.array_equal(np.nonzero((planes[1]["flag"] == M.INTERRUPT).all(axis=1))[0], [4])
    assert np.all(state["low"].sum(axis=0) + state["high"].sum(axis=0) == 2 * 3 + 1)  # one pull into the second trial


# ------------------------------------------------------------------------------------------------ 5. hand-over
def test_other_actors_after_a_thompson_collection(engine):
    """the env state and the step counter are handed over whole: a UCB1 collection on the same env, then a feed-forward
    policy's rollout, equal the restated env carried through all three"""
    n, k, E, T0, T1, T2, seed = 45, 3, 3, 7, 6, 5, 61
    env = ra.MetaBanditEnv(engine, n, k, E, seed_env=seed, seed_actor=seed + 1)
    ref_env = M.MetaLanes(n, k, E, seed_env=seed)
    ts = ra.BanditAgent(env, "thompson", num_samples=3)
    ref_ts = TR.ThompsonAgentLanes(n, k, 3, seed_actor=seed + 1)
    traj0 = ra.Trajectory(engine, n, T0, env.D)
    ts.rollout(env, traj0)
    same_planes(traj0.read_all(), ref_ts.rollout(ref_env, T0), "thompson")
    same_state(ts, ref_ts, "thompson")
    ucb = ra.BanditAgent(env, "ucb1")
    ref_ucb = B.BanditAgentLanes(n, k, B.UCB1, seed_actor=seed + 1)
    traj1 = ra.Trajectory(engine, n, T1, env.D)
    ucb.rollout(env, traj1)
    same_planes(traj1.read_all(), ref_ucb.rollout(ref_env, T1), "ucb1 after thompson")
    same_state(ts, ref_ts, "the thompson agent is untouched by another agent's collection")
    pol = ra.Mlp(engine, env.D, [32], k)
    pol.init(7)
    traj2 = ra.Trajectory(engine, n, T2, env.D)
    ra.rollout(env, pol, traj2)
    got = traj2.read_all()
    same_planes(got, dict(ref_env.replay(got["action"]), action=got["action"]), "policy after both")
    ts.rollout(env, traj0)  # ... and the Thompson agent carries on from its own word position
    same_planes(traj0.read_all(), ref_ts.rollout(ref_env, T0), "thompson again")
    same_state(ts, ref_ts, "thompson again")


# ------------------------------------------------------------------------------------------------ 6. refusals
def raw_create(env, **fields):
    cfg = ra.bandit_agent_config_default(fields.pop("kind", ra.BANDIT_AGENT_THOMPSON))
    for name, v in fields.items():
        setattr(cfg, name, v)
    h = C.c_void_p()
    code = ra.lib().rl_bandit_agent_create(env.h, C.byref(cfg), C.byref(h))
    msg = ra.lib().rl_last_error(env.eng.h).decode() if code != ra.OK else ""
    if code == ra.OK:
        ra.lib().rl_bandit_agent_destroy(h)
    return code, msg


def test_refusals(engine):
    n, k, E = 8, 3, 4
    env = ra.MetaBanditEnv(engine, n, k, E)
    lib = ra.lib()
    code, msg = raw_create(ra.ChainEnv(engine, n))
    assert code == ra.ERR_UNSUPPORTED and "rl_bandit_agent_create" in msg
    code, msg = raw_create(env, initial_action_count=0)
    assert code == ra.ERR_INVALID_ARGUMENT and "num_samples" in msg
    code, msg = raw_create(env, initial_action_count=1025)
    assert code == ra.ERR_UNSUPPORTED and "num_samples" in msg and "1024" in msg
    code, msg = raw_create(env, initial_action_count=1 << 40)
    assert code == ra.ERR_UNSUPPORTED and "num_samples" in msg
    assert raw_create(env, initial_action_count=1024)[0] == ra.OK and raw_create(env)[0] == ra.OK
    for reserved in (1, -1):
        code, msg = raw_create(env, reserved=reserved)
        assert code == ra.ERR_INVALID_ARGUMENT and "reserved" in msg
    cfg = ra.bandit_agent_config_default("thompson")
    h = C.c_void_p()
    for bad in (3, 5):  # 3 stays unassigned
        cfg.kind = bad
        assert lib.rl_bandit_agent_create(env.h, C.byref(cfg), C.byref(h)) == ra.ERR_INVALID_ARGUMENT
        assert "unknown kind" in lib.rl_last_error(engine.h).decode()
    # the fields a TABULAR_Q agent's config uses are not looked at
    assert raw_create(env, exploration_rate=float("nan"), initial_action_value=-1.0)[0] == ra.OK
    with pytest.raises(ValueError):
        ra.BanditAgent(env, "ucb1", num_samples=3)
    with pytest.raises(ra.RelearnError) as e:
        ra.BanditAgent(env, "thompson", num_samples=0)
    assert e.value.code == ra.ERR_INVALID_ARGUMENT and "num_samples" in str(e.value)
    # rollout on another env
    agent = ra.BanditAgent(env, "thompson")
    other = ra.MetaBanditEnv(engine, n, k - 1, E)
    with pytest.raises(ra.RelearnError) as e:
        agent.rollout(other, ra.Trajectory(engine, n, 5, other.D))
    assert e.value.code == ra.ERR_INVALID_ARGUMENT and "rl_bandit_agent_rollout" in str(e.value)
    # state_read: fields 1..4 against this kind, 5 and 6 against the others
    buf = np.zeros(k * n + 1, np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)

    def read(a, field, nbytes):
        return lib.rl_bandit_agent_state_read(a.h, C.c_int32(field), p, C.c_uint64(nbytes))

    assert read(agent, ra.BANDIT_STATE_ACTOR_POS, 8 * n) == ra.OK
    assert read(agent, ra.BANDIT_STATE_LOW_COUNTS, 8 * k * n) == ra.OK and np.all(buf[:k * n] == 1)
    assert read(agent, ra.BANDIT_STATE_HIGH_COUNTS, 8 * k * n) == ra.OK and np.all(buf[:k * n] == 1)
    assert read(agent, ra.BANDIT_STATE_LOW_COUNTS, 8 * n) == ra.ERR_INVALID_ARGUMENT
    assert "byte count" in lib.rl_last_error(engine.h).decode()
    for field, nbytes in ((ra.BANDIT_STATE_COUNTS, 8 * k * n), (ra.BANDIT_STATE_VALUES, 8 * k * n),
                          (ra.BANDIT_STATE_VISITS, 8 * n), (ra.BANDIT_STATE_LN_TABLE, 8 * E)):
        assert read(agent, field, nbytes) == ra.ERR_INVALID_ARGUMENT, field
        assert "no such field" in lib.rl_last_error(engine.h).decode()
    assert read(agent, 7, 8 * n) == ra.ERR_INVALID_ARGUMENT and "unknown field" in lib.rl_last_error(engine.h).decode()
    for kind in ("random", "tabular_q", "ucb1"):
        a = ra.BanditAgent(env, kind)
        for field in (ra.BANDIT_STATE_LOW_COUNTS, ra.BANDIT_STATE_HIGH_COUNTS):
            assert read(a, field, 8 * k * n) == ra.ERR_INVALID_ARGUMENT, (kind, field)
            assert "no such field" in lib.rl_last_error(engine.h).decode()
        assert set(a.state()) & {"low", "high"} == set()
    agent.rollout(env, ra.Trajectory(engine, n, 5, env.D))  # ... and the handle still works
    assert np.all(agent.state()["pos"] >= 4 * k * 3)


# ------------------------------------------------------------------------------------------------ 7. one statistical line
def test_thompson_beats_random(engine):
    """4,096 lanes, UniformBernoulli(3), 20 episodes per trial, one trial each.  A CPU simulation of the stated
    algorithm gave 12.52 +- 0.07 (TS) against 9.94 +- 0.06 (RANDOM), OTS 13.36: the bar of 1.5 lies more than ten
    standard errors below the gap.  The TS planes are also compared bit for bit: about 1e6 device rl_log / rl_exp
    evaluations against the host's"""
    n, k, E, seed = 4096, 3, 20, 91
    T = 2 * E - 1
    means = {}
    for kind in ("thompson", "random"):
        env = ra.MetaBanditEnv(engine, n, k, E, seed_env=seed, seed_actor=seed + 1)
        agent = ra.BanditAgent(env, kind)
        traj = ra.Trajectory(engine, n, T, env.D)
        agent.rollout(env, traj)
        got = traj.read_all()
        assert np.all(got["flag"][-1] == M.INTERRUPT)
        means[kind] = got["reward"].astype(np.float64).sum(axis=0).mean()
        if kind == "thompson":
            ref = TR.ThompsonAgentLanes(n, k, 1, seed_actor=seed + 1)
            same_planes(got, ref.rollout(M.MetaLanes(n, k, E, seed_env=seed), T), "4096 lanes")
            same_state(agent, ref, "4096 lanes")
    print("mean trial reward: TS %.3f, RANDOM %.3f" % (means["thompson"], means["random"]))
    assert means["thompson"] - means["random"] >= 1.5
