"""Tabular-MDP lanes (rl_env_create_tabular_mdp / ra.TabularMdpEnv) through the C ABI: driven steps, rollouts and a DQN
collection bit for bit against the Python restatement (tests/tabular_mdp_ref.py) stepped with the recorded actions;
rl_env_set_state; transition and reward frequencies at 4.4 sigma; updates on a host-written copy of a collected history;
the reference's DQN criterion and TRPO learning against the MDP's exact values; refusals; actor documents.
The cases and the reason for their shapes: tests/tabular_mdp_cases.py."""
import ctypes as C

import numpy as np
import pytest

import tabular_mdp_cases as cases
import tabular_mdp_ref as R

pytestmark = pytest.mark.gpu

ra = pytest.importorskip("relearn_amd")

N = cases.N_LANES
SEEDS = dict(seed_env=3, seed_actor=4)


def make_env(engine, case, n=N, **seeds):
    (tr, mean, sd), limit, max_steps, off = case
    seeds = seeds or SEEDS
    env = ra.TabularMdpEnv(engine, tr, mean, sd, n_lanes=n, max_steps=max_steps, limit=limit, lane_offset=off, **seeds)
    sim = R.MdpLanes(n, tr, mean, sd, limit, max_steps, off, seed_env=seeds["seed_env"])
    assert (env.D, env.A) == (cases.obs_width(case), tr.shape[1]) and sim.D == env.D
    return env, sim


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_step(env, sim, actions, t):
    reward, flag, obs, term = env.step(actions)
    w_reward, w_flag, w_obs, w_term = sim.step(actions)
    assert np.array_equal(bits(reward), bits(w_reward)), (t, np.flatnonzero(bits(reward) != bits(w_reward))[:8])
    assert np.array_equal(flag, w_flag), t
    assert np.array_equal(bits(obs), bits(w_obs)), t
    cut = w_flag == R.INTERRUPT
    assert np.array_equal(bits(term[:, cut]), bits(w_term[:, cut])), t
    for got, want in zip(env.get_state(), sim.state()):
        assert np.array_equal(got, want), t
    return int(cut.sum())


# ---------------------------------------------------------------- 1. driven steps
@pytest.mark.parametrize("name", sorted(cases.DRIVEN_CASES))
def test_driven_steps_bit_exact(engine, name):
    """40 host-driven steps: rewards, flags, next and interrupt-successor observations and the lane state after every step"""
    case = cases.DRIVEN_CASES[name]
    env, sim = make_env(engine, case)
    assert np.array_equal(env.observe(), sim.observe())
    acts = np.random.RandomState(7).randint(0, env.A, size=(40, N)).astype(np.uint8)
    cuts = sum(check_step(env, sim, acts[t], t) for t in range(40))
    limit, max_steps = case[1], case[2]
    assert cuts == (0 if limit == cases.LIMIT_NONE else N * (40 // max_steps))
    if name == "s4a3_mixed":  # lanes have drawn different numbers of words
        assert len(np.unique(env.get_state()[1])) > 1


def test_a_draw_on_the_boundary_goes_to_the_next_bucket(engine):
    """cum[0] == u of lane 0's first step, exactly: successor 1"""
    probe = R.MdpLanes(1, *cases.random_table(3, 2, 2), seed_env=SEEDS["seed_env"])
    probe.step([0])
    u = probe.lanes[0].last_u
    assert 0.0 < u < 1.0 and float(np.float32(u)) == u and float(np.float32(1.0 - u)) == 1.0 - u
    tr, mean, sd = cases.random_table(3, 2, 2)
    tr[0, :] = np.array([u, 1.0 - u, 0.0], np.float32)
    env, sim = make_env(engine, ((tr, mean, sd), cases.LIMIT_NONE, 0, 0))
    acts = np.zeros(N, np.uint8)
    check_step(env, sim, acts, 0)
    assert env.get_state()[0][0] == 1 and sim.lanes[0].last_u == u


# ---------------------------------------------------------------- 2. rl_env_set_state
def test_set_state(engine):
    case = cases.DRIVEN_CASES["s4a3_mixed"]
    env, sim = make_env(engine, case)
    rs = np.random.RandomState(8)
    state = rs.randint(0, 4, N)
    pos = 2 * rs.randint(0, 5000, N)  # any even word, across block boundaries (words 14 / 16 of a block among them)
    pos[:4] = (14, 16, 30, 2 ** 33 + 14)
    rem = rs.randint(1, 7, N)
    rc = rs.randint(1, 100, N)
    env.set_state(state, pos, rem.astype(np.uint64), rc.astype(np.uint64))
    for lane, s, p, r, c in zip(sim.lanes, state, pos, rem, rc):
        lane.set(s, p, r, c)
    for got, want in zip(env.get_state(), sim.state()):
        assert np.array_equal(got, want)
    assert np.array_equal(env.observe(), sim.observe())
    acts = rs.randint(0, 3, size=(8, N)).astype(np.uint8)
    for t in range(8):
        check_step(env, sim, acts[t], t)
    # a state outside the tables, an odd stream position: refused, nothing written
    before = env.get_state()
    for bad_state, bad_pos in ((4, 0), (-1, 0), (0, 3), (0, -2)):
        with pytest.raises(ra.RelearnError) as err:
            env.set_state(np.full(N, bad_state), np.full(N, bad_pos), np.ones(N, np.uint64), np.ones(N, np.uint64))
        assert err.value.code == ra.ERR_INVALID_ARGUMENT and "rl_env_set_state" in str(err.value)
    for got, want in zip(env.get_state(), before):
        assert np.array_equal(got, want)


# ---------------------------------------------------------------- 3. frequencies
def test_frequencies(engine):
    n = cases.FREQ_LANES
    tr, mean, sd = cases.FREQ_TABLE
    env = ra.TabularMdpEnv(engine, tr, mean, sd, n_lanes=n, seed_env=cases.FREQ_SEED_ENV)
    acts = cases.freq_actions(n)
    states, nexts, rewards = [], [], []
    cur = env.observe().argmax(axis=0)
    for t in range(cases.FREQ_STEPS):
        reward, flag, obs, _ = env.step(acts[t])
        assert not flag.any()
        states.append(cur)
        cur = obs.argmax(axis=0)
        nexts.append(cur)
        rewards.append(reward)
    worst = cases.check_frequencies(cases.FREQ_TABLE, np.concatenate(states), acts.ravel(), np.concatenate(nexts),
                                    np.concatenate(rewards))
    print("largest deviation: %.2f sigma" % worst)


# ---------------------------------------------------------------- 4. rollouts, env side replayed
def modules(engine, D, A, kind, seed=11):
    if kind == "mlp16":
        pol, cri = ra.Mlp(engine, D, [16], A), ra.Mlp(engine, D, [16], 1)
    elif kind == "gru8-linear":
        pol, cri = ra.RnnChain(engine, "gru", D, 8, A), ra.RnnChain(engine, "gru", D, 8, 1)
    else:
        pol, cri = ra.RnnChain(engine, "lstm", D, 8, A, mlp_hidden=8), ra.RnnChain(engine, "lstm", D, 8, 1, mlp_hidden=8)
    pol.init(seed)
    cri.init(seed + 1)
    return pol, cri


MODULE_KINDS = ["mlp16", "gru8-linear", "lstm8-mlp8"]


@pytest.mark.parametrize("kind", MODULE_KINDS)
@pytest.mark.parametrize("name", sorted(cases.ROLLOUT_CASES))
def test_rollout_env_side_replayed(engine, name, kind):
    """rl_rollout at 70 lanes x T = 12, twice in a row (the second starts mid-episode): the recorded actions, fed to the
    restatement, reproduce every reward, flag, observation and successor observation"""
    T = 12
    env, sim = make_env(engine, cases.ROLLOUT_CASES[name])
    pol, _ = modules(engine, env.D, env.A, kind)
    traj = ra.Trajectory(engine, N, T, env.D)
    seen = np.zeros(env.A, np.int64)
    for period in range(2):
        ra.rollout(env, pol, traj)
        got = traj.read_all()
        assert got["action"].max() < env.A
        seen += np.bincount(got["action"].ravel(), minlength=env.A)
        want = sim.replay(got["action"])
        assert np.array_equal(bits(got["obs"]), bits(want["obs"])), period
        assert np.array_equal(bits(got["reward"]), bits(want["reward"])), period
        assert np.array_equal(got["flag"], want["flag"]), period
        cut = want["flag"] == R.INTERRUPT
        assert cut.sum() == N * (T * (period + 1) // 5 - T * period // 5)
        assert np.array_equal(bits(got["term_obs"][:, cut]), bits(want["term_obs"][:, cut])), period
        for a, b in zip(env.get_state(), sim.state()):
            assert np.array_equal(a, b)
    assert seen.min() > 0  # every action was sampled


# ---------------------------------------------------------------- 5. nothing env-specific reaches the updates
@pytest.mark.parametrize("kind", ["mlp16", "gru8-linear"])
def test_updates_on_a_host_written_copy_are_identical(engine, kind):
    T = 12
    env, _ = make_env(engine, cases.ROLLOUT_CASES["s7a8"])
    results = []
    pol, cri = modules(engine, env.D, env.A, kind)
    p0, c0 = pol.get_params(), cri.get_params()
    collected = ra.Trajectory(engine, N, T, env.D)
    ra.rollout(env, pol, collected)
    history = collected.read_all()
    written = ra.Trajectory(engine, N, T, env.D)
    written.write_all(history)
    for traj in (collected, written):
        pol.set_params(p0)
        cri.set_params(c0)
        ra.gae(traj, cri, 0.99, 0.95)
        st = ra.trpo_update(pol, traj)
        assert st.status == ra.OPT_OK
        cst = ra.critic_update(cri, ra.Adam(cri), traj, opt_steps=3)
        results.append((pol.get_params(), cri.get_params(), traj.read(ra.TRAJ_ADVANTAGES)))
    for a, b in zip(*results):
        assert np.array_equal(bits(a), bits(b))
    assert not np.array_equal(results[0][0], p0) and not np.array_equal(results[0][1], c0)


# ---------------------------------------------------------------- 6. DQN
def dqn_config(capacity, eps, minibatch=64, opt_steps=4, td=True, gamma=0.5):
    cfg = ra.dqn_config_default()
    cfg.target = ra.DQN_TARGET_ONE_STEP_TD if td else ra.DQN_TARGET_REWARD_TO_GO
    cfg.exploration_kind, cfg.exploration_start = ra.SCHEDULE_CONSTANT, eps
    cfg.minibatch_steps, cfg.opt_steps_per_update, cfg.buffer_capacity = minibatch, opt_steps, capacity
    cfg.discount_factor = gamma
    for i in range(8):
        cfg.agent_key[i] = i + 1
    return cfg


def last_collection(dqn, T):
    """the last collection out of the ring, time-major (T <= capacity): step t of lane i is at slot (total_i - T + t) mod C"""
    total = dqn.replay_read(ra.REPLAY_TOTAL).astype(np.int64)
    slots = (total[None, :] - T + np.arange(T)[:, None]) % dqn.C
    take = lambda plane: np.take_along_axis(plane, slots, axis=0)
    obs, nobs = dqn.replay_read(ra.REPLAY_OBS), dqn.replay_read(ra.REPLAY_NEXT_OBS)
    return dict(obs=np.stack([take(obs[d]) for d in range(dqn.D)], axis=1),  # [T][D][n]
                next=np.stack([take(nobs[d]) for d in range(dqn.D)], axis=1),
                action=take(dqn.replay_read(ra.REPLAY_ACTION)), reward=take(dqn.replay_read(ra.REPLAY_REWARD)),
                flag=take(dqn.replay_read(ra.REPLAY_FLAG)))


@pytest.mark.parametrize("name,eps", [("s2a2_none", 0.5), ("s3a2_latent7", 0.5), ("s7a8_visible5", 0.5),
                                      ("s4a3_mixed", 1.0), ("s8a8_latent5", 0.0)])
def test_dqn_collection_env_side_replayed(engine, name, eps):
    """k_dqn_lane_step<MdpOps, D, 64, A> behind the per-layer kernels: two collections of 9 and 7 steps, the ring's record
    of each against the restatement stepped with the recorded actions (the horizon rule: the open episode closes as an
    Interrupt with its successor, the env carries on); at rate 0 the actions are the first maximal output"""
    env, sim = make_env(engine, cases.DRIVEN_CASES[name])
    q = ra.Mlp(engine, env.D, [16], env.A, "Tanh")  # (Tanh: at 4 or 5 inputs and two outputs too, the per-layer kernels)
    q.init(21)
    dqn = ra.FiniteDqn(env, q, ra.Adam(q), dqn_config(32, eps))
    for T in (9, 7):
        dqn.collect(T)
        rec = last_collection(dqn, T)
        cur = sim.observe()
        for t in range(T):
            assert np.array_equal(bits(rec["obs"][t]), bits(cur)), t
            if eps == 0.0:
                z = q.forward(np.ascontiguousarray(cur.T))
                top = np.sort(z, axis=1)
                clear = top[:, -1] - top[:, -2] > 1e-5  # (where the f32 forward cannot have ordered the outputs otherwise)
                assert np.array_equal(rec["action"][t][clear], z.argmax(axis=1)[clear])
            reward, flag, nxt, term = sim.step(rec["action"][t])
            want_flag, succ = flag.copy(), term
            if t == T - 1:
                cut = flag == R.CONTINUE
                want_flag[cut] = R.INTERRUPT
                succ = np.where(cut[None], nxt, term)
            assert np.array_equal(rec["flag"][t], want_flag), t
            assert np.array_equal(bits(rec["reward"][t]), bits(reward)), t
            m = want_flag == R.INTERRUPT
            assert np.array_equal(bits(rec["next"][t][:, m]), bits(succ[:, m])), t
            cur = nxt
        for a, b in zip(env.get_state(), sim.state()):
            assert np.array_equal(a, b)
    st = dqn.update()
    assert st.opt_steps == 4 and np.isfinite(st.loss_last)
    dqn.close()


# two states, three actions, no noise.  In state 0 the best action (1) pays nothing and moves to state 1, where action 2
# pays 1 and stays; the others pay more at once and stay behind.  At discount 0.5: Q*(0, .) = (0.7, 1.0, 0.6),
# Q*(1, .) = (1.0, 1.2, 2.0).
DQN_TR = np.zeros((2, 3, 2), np.float32)
DQN_TR[0, 0, 0] = DQN_TR[0, 1, 1] = DQN_TR[0, 2, 0] = 1.0
DQN_TR[1, 0, 0] = DQN_TR[1, 1, 1] = DQN_TR[1, 2, 1] = 1.0
DQN_MEAN = np.array([[0.2, 0.0, 0.1], [0.5, 0.2, 1.0]])
DQN_OPTIMAL = np.array([1, 2])
DQN_PERIODS = 30


def test_dqn_learns_the_delayed_reward(engine):
    """the reference's criterion (train_deterministic_bandit, src/agents/testing.rs:14-64: the right action in at least
    90 % of the greedy evaluation steps) on an MDP whose best first action has the lowest immediate reward, under the
    one-step TD target"""
    q_star = np.zeros((2, 3))
    for _ in range(200):
        q_star = DQN_MEAN + 0.5 * (DQN_TR.astype(np.float64) @ q_star.max(axis=1))
    assert np.array_equal(q_star.argmax(axis=1), DQN_OPTIMAL) and DQN_MEAN[0].argmax() != DQN_OPTIMAL[0]
    n = 64

    def agent(qnet, eps, seed):
        env = ra.TabularMdpEnv(engine, DQN_TR, DQN_MEAN, np.zeros((2, 3)), n_lanes=n, max_steps=8, limit=ra.LIMIT_LATENT,
                               seed_env=seed, seed_actor=seed + 1)
        acfg = ra.adam_config_default()
        acfg.learning_rate = 0.01
        return ra.FiniteDqn(env, qnet, ra.Adam(qnet, acfg), dqn_config(64, eps, minibatch=128, opt_steps=20))

    q = ra.Mlp(engine, 2, [16, 16], 3)
    q.init(7)
    dqn = agent(q, 1.0, 31)  # uniform exploration: every (state, action) is visited
    for _ in range(DQN_PERIODS):
        dqn.collect(8)
        st = dqn.update()
        assert np.isfinite(st.loss_last)
    greedy = agent(q, 0.0, 41)
    greedy.collect(16)  # 64 lanes x 16 steps: two episodes per lane, from state 0
    rec = last_collection(greedy, 16)
    state = rec["obs"].argmax(axis=1)
    right = int((rec["action"] == DQN_OPTIMAL[state]).sum())
    print("optimal action in %d of %d greedy steps; Q(one-hot) = %s" % (right, state.size, q.forward(np.eye(2, dtype=np.float32))))
    assert (state == 0).sum() >= 2 * n and (state == 1).sum() > 0
    assert right >= 0.9 * state.size
    dqn.close()
    greedy.close()


# ---------------------------------------------------------------- 7. learning
LEARN_SEED, LEARN_LIMIT, LEARN_LANES = 5, 16, 1024
LEARN_PERIODS = 24  # twice the slowest of three seeds' crossings, 12, 4 and 7 (profiles/tabular_mdp_learning.json)


def learning_mdp():
    cfg = ra.random_mdps_config_default()
    cfg.num_states, cfg.num_actions = 4, 3
    tr, mean = ra.sample_random_mdp(cfg, LEARN_SEED, 0)
    return tr, mean


def train_trpo(engine, seed, periods):
    """-> (mean episode reward per period, the bar, optimal, uniform)"""
    tr, mean = learning_mdp()
    optimal, uniform = R.finite_horizon_values(tr, mean, LEARN_LIMIT)
    env = ra.TabularMdpEnv(engine, tr, mean, None, n_lanes=LEARN_LANES, max_steps=LEARN_LIMIT, limit=ra.LIMIT_VISIBLE,
                           seed_env=seed, seed_actor=seed + 1)
    pol, cri = ra.Mlp(engine, env.D, [16], env.A), ra.Mlp(engine, env.D, [16], 1)
    pol.init(seed + 2)
    cri.init(seed + 3)
    opt = ra.Adam(cri)
    traj = ra.Trajectory(engine, LEARN_LANES, LEARN_LIMIT, env.D)
    curve = []
    for _ in range(periods):
        ra.rollout(env, pol, traj)  # one whole episode per lane
        curve.append(float(traj.read(ra.TRAJ_REWARD).astype(np.float64).sum() / LEARN_LANES))
        ra.gae(traj, cri, 1.0, 0.95)
        ra.trpo_update(pol, traj)
        ra.critic_update(cri, opt, traj, opt_steps=20)
    return curve, 0.5 * (optimal + uniform), optimal, uniform


def test_trpo_learns_a_sampled_mdp(engine):
    """feed-forward TRPO on a four-state, three-action MDP of DirichletRandomMdps with unit reward noise, 1,024 lanes under a
    visible limit of 16: the mean episode reward passes the midpoint of the uniform-random and the optimal expected episode
    reward, both by f64 dynamic programming"""
    curve, bar, optimal, uniform = train_trpo(engine, 100, LEARN_PERIODS)
    print("uniform %.3f, optimal %.3f, bar %.3f; per period: %s" % (uniform, optimal, bar, " ".join("%.2f" % c for c in curve)))
    assert optimal - uniform > 2.0  # (there is something to learn: the noise of a period's mean is about 4 / 32)
    assert curve[-1] > bar
    assert curve[-1] <= optimal + 1.0  # (nothing earns more than the optimal policy: the dynamic programme is the env's)


def test_uniform_driver_earns_the_uniform_value(engine):
    """the other end of the learning test's bar: 1,024 episodes under uniform-random actions against the f64 dynamic
    programme, within 4.4 standard errors of the episodes' own spread"""
    tr, mean = learning_mdp()
    _, uniform = R.finite_horizon_values(tr, mean, LEARN_LIMIT)
    env = ra.TabularMdpEnv(engine, tr, mean, None, n_lanes=LEARN_LANES, max_steps=LEARN_LIMIT, limit=ra.LIMIT_VISIBLE,
                           seed_env=77)
    acts = np.random.RandomState(78).randint(0, 3, size=(LEARN_LIMIT, LEARN_LANES)).astype(np.uint8)
    total = np.zeros(LEARN_LANES)
    for t in range(LEARN_LIMIT):
        reward, flag, _, _ = env.step(acts[t])
        total += reward
    assert np.all(flag == ra.SUCC_INTERRUPT)
    se = total.std(ddof=1) / np.sqrt(LEARN_LANES)
    print("uniform driver %.3f, dynamic programme %.3f, standard error %.3f" % (total.mean(), uniform, se))
    assert abs(total.mean() - uniform) <= cases.SIGMAS * se


# ---------------------------------------------------------------- 8. refusals
def refusal(f):
    with pytest.raises(ra.RelearnError) as e:
        f()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("name", sorted(cases.REFUSAL_CASES))
def test_env_refusals(engine, name):
    args, code, fragment = cases.REFUSAL_CASES[name]
    got, msg = refusal(lambda: ra.TabularMdpEnv(engine, args["transitions"], args["reward_mean"], args["reward_stddev"],
                                                n_lanes=8, max_steps=args["max_steps"], limit=args["limit"]))
    assert got == code and fragment in msg, msg


def test_null_pointers_and_the_generic_constructor(engine):
    tr, mean, sd = cases.random_table(3, 2, 9)
    cfg = ra.EnvConfig()
    cfg.kind, cfg.n_lanes, cfg.cartpole = ra.ENV_TABULAR_MDP, 8, ra.cartpole_params_default()
    mdp = ra.TabularMdpConfig(3, 2, 1.0)
    h = C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f = ra.lib().rl_env_create_tabular_mdp
    for args in ((None, C.byref(mdp), p(tr), p(mean), p(sd), C.byref(h)), (C.byref(cfg), None, p(tr), p(mean), p(sd), C.byref(h)),
                 (C.byref(cfg), C.byref(mdp), None, p(mean), p(sd), C.byref(h)),
                 (C.byref(cfg), C.byref(mdp), p(tr), None, p(sd), C.byref(h)),
                 (C.byref(cfg), C.byref(mdp), p(tr), p(mean), p(sd), None)):
        assert f(engine.h, *args) == ra.ERR_INVALID_ARGUMENT
    assert f(engine.h, C.byref(cfg), C.byref(mdp), p(tr), p(mean), None, C.byref(h)) == ra.OK  # stddev 1 everywhere
    assert ra.lib().rl_env_destroy(h) == ra.OK
    assert ra.lib().rl_env_create(engine.h, C.byref(cfg), C.byref(h)) == ra.ERR_BUILD_ENV  # the kind has its own constructor
    # NULL stddev is 1.0 everywhere: the same lanes as an explicit table of ones
    a = ra.TabularMdpEnv(engine, tr, mean, None, n_lanes=8, **SEEDS)
    b = ra.TabularMdpEnv(engine, tr, mean, np.ones_like(mean), n_lanes=8, **SEEDS)
    acts = np.arange(8, dtype=np.uint8) % 2
    for _ in range(5):
        for x, y in zip(a.step(acts), b.step(acts)):
            assert np.array_equal(x, y)


def test_agent_refusals(engine):
    env2, _ = make_env(engine, cases.DRIVEN_CASES["s3a2_latent7"])   # 3 features, 2 actions
    env3, _ = make_env(engine, cases.DRIVEN_CASES["s5a3_visible4"])  # 6 features, 3 actions
    cfg = dqn_config(16, 0.5)
    # recurrent DQN, by either constructor
    g2 = ra.RnnChain(engine, "gru", env2.D, 8, 2)
    g3 = ra.RnnChain(engine, "gru", env3.D, 8, 3, mlp_hidden=8)
    for env, g in ((env2, g2), (env3, g3)):
        g.init(1)
        code, msg = refusal(lambda: ra.FiniteDqn(env, g, ra.Adam(g), cfg))
        assert code == ra.ERR_UNSUPPORTED and "rl_dqn_create_finite" in msg and "recurrent" in msg, msg
    code, msg = refusal(lambda: ra.RecurrentDqn(env2, g2, ra.Adam(g2), cfg))
    assert code == ra.ERR_UNSUPPORTED and "rl_dqn_create_recurrent" in msg and "TABULAR_MDP" in msg, msg
    # rl_dqn_create on these lanes
    q2 = ra.Mlp(engine, env2.D, [16], 2)
    q2.init(1)
    code, msg = refusal(lambda: ra.Dqn(env2, q2, ra.Adam(q2), cfg))
    assert code == ra.ERR_UNSUPPORTED and "rl_dqn_create" in msg and "TABULAR_MDP" in msg, msg
    ra.FiniteDqn(env2, q2, ra.Adam(q2), cfg).close()  # two actions build through the finite constructor
    # a module of the fused shape is not collected on these lanes
    env4 = ra.TabularMdpEnv(engine, *cases.random_table(4, 2, 3), n_lanes=8)
    fused = ra.Mlp(engine, 4, 16, 2)
    code, msg = refusal(lambda: ra.FiniteDqn(env4, fused, ra.Adam(fused), cfg))
    assert code == ra.ERR_UNSUPPORTED and "rl_dqn_create_finite" in msg and "per-layer" in msg, msg
    # a module that does not match the env
    q_bad = ra.Mlp(engine, env3.D, [16], 2)
    code, msg = refusal(lambda: ra.FiniteDqn(env3, q_bad, ra.Adam(q_bad), cfg))
    assert code == ra.ERR_INVALID_ARGUMENT and "rl_dqn_create_finite" in msg
    # a two-action recurrent constructor's module in rl_rollout, on an env of another width than its own
    # (on a two-action MDP such a module IS the chain rl_rnn_chain_create builds, and rolls out: the rollout tests)
    old3 = ra.GruMlp(engine, env3.D, 2, 8, 8)
    code, msg = refusal(lambda: ra.rollout(env3, old3, ra.Trajectory(engine, N, 4, env3.D)))
    assert code == ra.ERR_UNSUPPORTED and "two actions" in msg, msg
    # the bandit baselines stay on the meta lanes
    code, msg = refusal(lambda: ra.BanditAgent(env2, "random"))
    assert code == ra.ERR_UNSUPPORTED


# ---------------------------------------------------------------- 9. actor documents
@pytest.mark.parametrize("name", sorted(cases.ROLLOUT_CASES))
def test_actor_documents(engine, name):
    from cbor_ref import decode
    case = cases.ROLLOUT_CASES[name]
    env, _ = make_env(engine, case)
    S = case[0][0].shape[0]
    space = {"inner": {"inner": {"size": S}, "remaining": {"low": 0.0, "high": 1.0}}}
    pol = ra.Mlp(engine, env.D, [16], env.A)
    pol.init(5)
    data = ra.actor_to_cbor(env, pol)
    doc = decode(data)
    assert list(doc) == ["observation_space", "action_space", "policy_module"]
    assert doc["observation_space"] == space and doc["action_space"] == {"size": env.A}
    other = ra.Mlp(engine, env.D, [16], env.A)
    ra.module_from_cbor(other, data)
    assert np.array_equal(other.get_params(), pol.get_params())
    data = ra.actor_to_cbor(env, pol, ra.ACTOR_DQN, exploration_rate=0.25)
    doc = decode(data)
    assert list(doc) == ["observation_space", "action_space", "action_value_fn", "exploration_rate"]
    assert doc["observation_space"] == space and doc["action_space"] == {"size": env.A} and doc["exploration_rate"] == 0.25
    other.init(9)
    ra.module_from_cbor(other, data)
    assert np.array_equal(other.get_params(), pol.get_params())
    chain = ra.RnnChain(engine, "gru", env.D, 8, env.A)
    chain.init(6)
    doc = decode(ra.actor_to_cbor(env, chain))
    assert doc["observation_space"] == space and doc["action_space"] == {"size": env.A}
    # without a visible limit the env's own space is written
    bare = ra.TabularMdpEnv(engine, *case[0], n_lanes=8)
    p2 = ra.Mlp(engine, bare.D, [16], bare.A)
    p2.init(1)
    assert decode(ra.actor_to_cbor(bare, p2))["observation_space"] == {"inner": {"size": S}}
