"""Every kernel that steps a lane, on data that holds a Terminate, an Interrupt, a Continue and both actions, at a lane
count that leaves its last block ragged — the cases the other files of the suite do not reach in one piece (DESIGN.md
§25 lists who steps a lane and which test holds it).  The env side of what the device recorded replays bit for bit through
the oracle's lanes, which are driven with the device's own actions; each test asserts its data conditions from the flag
plane it read back.

50 lanes: one ragged block for the kernels that give a lane a thread (blocks of 64 and 256).  Step limits of 12 to 19
steps over 40 to 60 steps of CartPole under random actions or a freshly initialised module: the oracle's lanes under a
one-layer module of the same seeds end 71 episodes by a fall and 129 at a limit of 12 (seeds and limits were searched with
the oracle alone)."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import relearn_amd as ra

pytestmark = pytest.mark.gpu

N = 50


def conditions(flag, action):
    """the data conditions of a case: every successor code and both actions occur"""
    return {"terminate": bool((flag == O.TERMINATE).any()), "interrupt": bool((flag == O.INTERRUPT).any()),
            "continue": bool((flag == O.CONTINUE).any()), "action 0": bool((action == 0).any()),
            "action 1": bool((action == 1).any())}


def replay_trajectory(sim, got, T):
    """the recorded trajectory against the oracle's lanes stepped with the recorded actions"""
    assert np.array_equal(got["obs"][:, 0, :], sim.observe())
    for t in range(T):
        reward, flag, obs, term = sim.step(got["action"][t])
        assert np.array_equal(got["reward"][t], reward) and np.array_equal(got["flag"][t], flag), t
        assert np.array_equal(got["obs"][:, t + 1, :], obs), t
        m = flag == O.INTERRUPT
        assert np.array_equal(got["term_obs"][:, t, m], term[:, m]), t


# A feed-forward policy with several hidden layers rolls out all T steps in one launch (k_gen_rollout_cartpole).  A
# recurrent policy with two layers runs one launch sequence per step, whose last launch samples, steps and records
# (k_gen_step_cartpole).
@pytest.mark.parametrize("kind", ["fused", "stepwise"])
def test_policy_rollout_off_the_5_128_path_on_a_ragged_lane_count(engine, kind):
    T, max_steps = 48, 12
    pol = ra.Mlp(engine, 5, [32, 32], 2) if kind == "fused" else ra.GruMlp(engine, 5, 2, 16, 12, num_layers=2)
    pol.init(11)
    env = ra.CartPoleEnv(engine, N, max_steps=max_steps, seed_env=3, seed_actor=4)
    sim = O.LaneSim(N, max_steps=max_steps, seed_env=3, seed_actor=4)
    traj = ra.Trajectory(engine, N, T, 5)
    seen = None
    for _ in range(2):  # the second rollout continues the lanes and crosses word 48 of the actor stream
        ra.rollout(env, pol, traj)
        got = traj.read_all()
        replay_trajectory(sim, got, T)
        c = conditions(got["flag"], got["action"])
        seen = c if seen is None else {k: seen[k] or c[k] for k in c}
    assert all(seen.values()), seen


@pytest.mark.parametrize("limit,max_steps", [(ra.LIMIT_LATENT, 19), (ra.LIMIT_NONE, 0)], ids=["latent", "none"])
def test_standalone_cartpole_step_with_four_features(engine, limit, max_steps):
    """k_env_step at D = 4 (no visible step limit), reset and observe included, under random actions"""
    T = 60
    env = ra.CartPoleEnv(engine, N, max_steps=max_steps, limit=limit, seed_env=7, seed_actor=8)
    sim = O.LaneSim(N, max_steps=max_steps, limit=limit, seed_env=7, seed_actor=8)
    assert env.D == 4
    assert np.array_equal(env.observe(), sim.observe())
    rng = np.random.default_rng(5)
    flags, actions = [], []
    for t in range(T):
        a = rng.integers(0, 2, N).astype(np.uint8)
        got, want = env.step(a), sim.step(a)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), t
        assert np.array_equal(got[2], want[2]), t
        m = want[1] == O.INTERRUPT
        assert np.array_equal(got[3][:, m], want[3][:, m]), t
        flags.append(want[1])
        actions.append(a)
    assert np.array_equal(env.observe(), sim.observe())
    c = conditions(np.array(flags), np.array(actions))
    if limit == ra.LIMIT_NONE:
        c.pop("interrupt")  # no limit, no Interrupt: the latent case holds it
    assert all(c.values()), c


# MemoryGame::new(3, 2) and (2, 5) under a visible limit: D = 6 and 8.  Every episode of a MemoryGame has
# history_len + 1 steps, so one limit cannot give both endings: max_steps = history_len + 1 lets the answer step
# through (it passes the limit untouched: Terminate), one step less cuts every episode before it (Interrupt).
@pytest.mark.parametrize("num_actions,history_len,cut", [(3, 2, False), (3, 2, True), (2, 5, False), (2, 5, True)])
def test_standalone_memory_game_of_other_sizes_under_a_visible_limit(engine, num_actions, history_len, cut):
    T = 4 * (history_len + 1) + 1
    max_steps = history_len + (0 if cut else 1)
    kw = dict(num_actions=num_actions, history_len=history_len, max_steps=max_steps, limit=ra.LIMIT_VISIBLE, seed_env=9,
              seed_actor=10)
    env, sim = ra.MemoryEnv(engine, N, **kw), O.MemoryLaneSim(N, **kw)
    assert env.D == sim.D == num_actions + history_len + 1
    assert np.array_equal(env.observe(), sim.observe())
    rng = np.random.default_rng(6)
    flags, rewards = [], []
    for t in range(T):
        a = rng.integers(0, num_actions, N).astype(np.uint8)
        got, want = env.step(a), sim.step(a)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), t
        assert np.array_equal(got[2], want[2]), t
        m = want[1] == O.INTERRUPT
        assert np.array_equal(got[3][:, m], want[3][:, m]), t
        flags.append(want[1])
        rewards.append(want[0])
    for g, w in zip(env.get_state(), sim.get_state()):
        assert np.array_equal(g, w)
    flags, rewards = np.array(flags), np.array(rewards)
    assert (flags == O.CONTINUE).any() and (flags == (O.INTERRUPT if cut else O.TERMINATE)).any()
    assert not (flags == (O.TERMINATE if cut else O.INTERRUPT)).any()
    if not cut:
        assert (rewards == 1.0).any() and (rewards == -1.0).any()  # right and wrong answers


def test_general_dqn_collection_cuts_a_lane_that_terminated_earlier(engine):
    """k_dqn_lane_step on a ragged lane count: the env side of every step through the oracle's lanes, the recorded
    successor codes under the horizon rule (a lane still mid-episode at the last step closes as an Interrupt whose
    successor is the observation the env carries on with), and the actor stream's end position"""
    T, max_steps, eps, seed_actor = 40, 12, 0.3, 34
    env = ra.CartPoleEnv(engine, N, max_steps=max_steps, limit=ra.LIMIT_VISIBLE, seed_env=21, seed_actor=seed_actor)
    sim = O.LaneSim(N, max_steps=max_steps, limit=ra.LIMIT_VISIBLE, seed_env=21, seed_actor=seed_actor)
    q = ra.Mlp(engine, 5, [32, 32], 2)
    q.init(77)
    cfg = ra.dqn_config_default()
    cfg.exploration_kind, cfg.exploration_start = ra.SCHEDULE_CONSTANT, eps
    cfg.minibatch_steps, cfg.opt_steps_per_update, cfg.buffer_capacity, cfg.discount_factor = 700, 3, 64, 0.99
    dqn = ra.Dqn(env, q, ra.Adam(q), cfg)
    cur = sim.observe()
    dqn.collect(T)
    obs, act, flag = dqn.replay_read(ra.REPLAY_OBS), dqn.replay_read(ra.REPLAY_ACTION), dqn.replay_read(ra.REPLAY_FLAG)
    nobs = dqn.replay_read(ra.REPLAY_NEXT_OBS)
    L, draws = O.lib(), 0
    ended = np.zeros(N, dtype=bool)
    for t in range(T):
        assert np.array_equal(obs[:, t, :], cur), t  # slot t = step t (no eviction: T <= capacity)
        reward, fl, nxt, term = sim.step(act[t])
        want = fl.copy()
        m = fl == O.INTERRUPT
        assert np.array_equal(nobs[:, t, m], term[:, m]), t
        if t == T - 1:
            cutm = fl == O.CONTINUE
            want[cutm] = O.INTERRUPT
            assert np.array_equal(nobs[:, t, cutm], nxt[:, cutm])
            assert (cutm & ended).any(), "no lane is cut by the horizon after an earlier Terminate"
        assert np.array_equal(flag[t], want), t
        ended |= fl == O.TERMINATE
        cur = nxt
    # the explore / greedy draws: the stream position every lane ends on is bounded by the draws a step can take, and the
    # recorded random actions are the stream's (tests/test_gpu_dqn.py restates DqnActor::act in full)
    pos = dqn.replay_read(ra.REPLAY_ACTOR_POS)
    assert (pos >= 2 * T).all() and (pos % 2 == 0).all()
    for i in (0, N - 1):
        r = O.Prng()
        L.oracle_prng_seed_from_u64(C.byref(r), seed_actor)
        L.oracle_prng_set_stream(C.byref(r), i)
        L.oracle_prng_set_word_pos(C.byref(r), 0)
        for t in range(T):
            if L.oracle_prng_gen_bool(C.byref(r), eps):
                assert act[t, i] == L.oracle_prng_gen_range_u64(C.byref(r), 0, 2), (t, i)
                draws += 1
        assert L.oracle_prng_word_pos(C.byref(r)) == pos[i]
    assert draws > 0
    c = conditions(flag[:T - 1], act[:T])
    assert all(c.values()), c
