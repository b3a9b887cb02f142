"""Meta-RL bandit lanes on the device (RL_ENV_META_BANDIT: MetaEnv over bandits under a TrialEpisodeLimit,
src/envs/meta.rs:128-203, 541-617; src/envs/bandits.rs) against the Python restatement tests/meta_lanes_ref.py and the
reference's own step sequence (tests/golden/meta_env_fixtures.json = meta.rs:642-769): the standalone env kernels, the
feed-forward rollout, the recurrent rollout in one launch against the launch sequence per step, the updates on what was
collected, the refusals, and that a recurrent policy learns to use its memory across inner episodes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import meta_lanes_ref as M
import oracle as O
import relearn_amd as ra

pytestmark = pytest.mark.gpu
L = O.lib()
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "meta_env_fixtures.json")))
KIND = {"continue": M.CONTINUE, "terminate": M.TERMINATE, "interrupt": M.INTERRUPT}
PLANES = ("obs", "action", "reward", "flag", "term_obs")


def fixture_features(k, o):
    prev = None if o["prev"] is None else (o["prev"]["action"], o["prev"]["reward"])
    return M.features(k, o["inner_none"], prev, o["done"])


# ------------------------------------------------------------------------------------------------ 1. the reference's steps
def test_fixture_on_the_device(engine):
    n, k = 50, FIXTURE["env"]["n_arms"]
    env = ra.MetaBanditEnv(engine, n, k, FIXTURE["env"]["episodes_per_trial"], FIXTURE["env"]["distribution"])
    assert (env.D, env.A) == (k + 4, k)
    fresh = fixture_features(k, FIXTURE["initial_observation"])
    assert np.array_equal(env.observe(), np.repeat(fresh[:, None], n, axis=1))
    for t, s in enumerate(FIXTURE["steps"]):
        reward, flag, obs, term = env.step(np.full(n, s["action"], np.uint8))
        assert np.all(reward == np.float32(s["reward"])) and np.all(flag == KIND[s["successor"]]), t
        succ = np.repeat(fixture_features(k, s["observation"])[:, None], n, axis=1)
        if KIND[s["successor"]] == M.INTERRUPT:  # the successor goes to term_obs; the lane shows its new trial
            assert np.array_equal(term, succ), t
            assert np.array_equal(obs, np.repeat(fresh[:, None], n, axis=1)), t
        else:
            assert np.array_equal(obs, succ), t


# ------------------------------------------------------------------------------------------------ 2. driven steps
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("dist", [M.UNIFORM_BERNOULLI, M.ONE_HOT])
def test_driven_steps_bit_for_bit(engine, dist, k, E):
    """50 lanes (ragged against workgroups of 64 and 256), 20 steps of random actions, a reset() in the middle of a trial;
    lanes 25..49 equal a 25-lane env at lane_offset 25"""
    n, steps, seed = 50, 20, 11 + k
    env = ra.MetaBanditEnv(engine, n, k, E, dist, seed_env=seed)
    tail = ra.MetaBanditEnv(engine, n - 25, k, E, dist, lane_offset=25, seed_env=seed)
    ref = M.MetaLanes(n, k, E, dist, seed_env=seed)
    rs = np.random.default_rng(100 * k + E)
    assert np.array_equal(env.observe(), ref.observe()) and np.array_equal(tail.observe(), ref.observe()[:, 25:])
    rewards, flags = [], []
    for t in range(steps):
        if t == 8:  # 8 mod (2 E - 1) = 3 at E = 3: inside a trial; the new trial draws where the stream stands
            env.reset(), tail.reset(), ref.reset()
            assert np.array_equal(env.observe(), ref.observe())
        a = rs.integers(0, k, n).astype(np.uint8)
        reward, flag, obs, term = env.step(a)
        reward_o, flag_o, obs_o, term_o = ref.step(a)
        assert np.array_equal(reward, reward_o) and np.array_equal(flag, flag_o), t
        assert np.array_equal(obs, obs_o), t
        cut = flag == M.INTERRUPT
        assert np.array_equal(term[:, cut], term_o[:, cut]), t
        reward_t, flag_t, obs_t, term_t = tail.step(a[25:])
        assert np.array_equal(reward_t, reward[25:]) and np.array_equal(flag_t, flag[25:]), t
        assert np.array_equal(obs_t, obs[:, 25:]) and np.array_equal(term_t[:, cut[25:]], term[:, 25:][:, cut[25:]]), t
        rewards.append(reward), flags.append(flag)
    rewards, flags = np.array(rewards), np.array(flags)
    # what the data must hold: rewards of both values (Bernoulli draws; one-hot arms hit and missed), and the successor
    # kinds this trial length has — every step of a one-episode trial is an Interrupt
    assert set(np.unique(rewards)) == {0.0, 1.0}
    assert set(np.unique(flags)) == ({M.INTERRUPT} if E == 1 else {M.CONTINUE, M.INTERRUPT})


# ------------------------------------------------------------------------------------------------ 3. feed-forward rollout
def test_feed_forward_rollout(engine):
    """[32] Relu policy over 3 arms (7 features), 50 lanes, T = 13 at 3 episodes per trial: trials end at steps 5 and 10
    and the horizon cuts the third"""
    n, T, k, E, seed_env, seed_actor = 50, 13, 3, 3, 5, 6
    env = ra.MetaBanditEnv(engine, n, k, E, seed_env=seed_env, seed_actor=seed_actor)
    pol = ra.Mlp(engine, env.D, [32], k)
    pol.init(7)
    traj = ra.Trajectory(engine, n, T, env.D)
    ra.rollout(env, pol, traj)
    got = traj.read_all()
    want = M.MetaLanes(n, k, E, seed_env=seed_env).replay(got["action"])
    for key in ("obs", "reward", "flag"):
        assert np.array_equal(got[key], want[key]), key
    cut = got["flag"] == M.INTERRUPT
    assert np.array_equal(np.nonzero(cut.all(axis=1))[0], [4, 9]) and not cut[[0, 12]].any()
    assert np.array_equal(got["term_obs"][:, cut], want["term_obs"][:, cut])
    assert set(np.unique(got["reward"])) == {0.0, 1.0} and got["action"].max() == k - 1
    # the actions: inverse-CDF draws at the policy's logits with word t of the lane's actor stream
    for t in (0, 7):
        x = np.ascontiguousarray(got["obs"][:, t, :].T)
        z = pol.forward(x)
        assert np.array_equal(z, O.mlp_layers_forward(env.D, [32], k, pol.get_params(), x, "Relu", "Identity"))
        for i in range(n):
            w = engine.stream_words(seed_actor, i, t, 1)[0]
            u = np.float32(w >> 8) * np.float32(1.0 / (1 << 24))
            lp = np.zeros(k, dtype=np.float32)
            L.oracle_log_softmax_f32(O.f32p(np.ascontiguousarray(z[i].astype(np.float32))), k, O.f32p(lp), 0)
            assert got["action"][t, i] == L.oracle_categorical_sample_u(O.f32p(lp), k, C.c_float(u), 0), (t, i)


# ------------------------------------------------------------------------------------------------ 4. recurrent rollout
def recurrent_policy(engine, cell, D, H, H2, A, seed):
    m = (ra.GruMlp if cell == "gru" else ra.LstmMlp)(engine, D, A, H, H2)
    m.init(seed)
    return m, O.GruShape(D, H, H2, A, O.CELL_GRU if cell == "gru" else O.CELL_LSTM)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_recurrent_rollout_fused_against_stepwise(engine, cell):
    """70 lanes (two workgroups, the second ragged), T = 13, 3 episodes per trial, two rollouts in a row (a trial and the
    actor stream carry over the horizon): the one-launch rollout (kernel variant 0) and the launch sequence per step
    (variant 1) write identical planes, and leave the lanes in states from which a driven step gives identical results"""
    n, T, E, seed_env, seed_actor = 70, 13, 3, 8, 9
    runs = {}
    try:
        for variant in (0, 1):
            engine.set_kernel_variant(variant)
            env = ra.MetaBanditEnv(engine, n, 2, E, seed_env=seed_env, seed_actor=seed_actor)
            pol, shape = recurrent_policy(engine, cell, env.D, 10, 6, 2, 21)
            traj = ra.Trajectory(engine, n, T, env.D)
            planes = []
            for period in range(2):
                ra.rollout(env, pol, traj)
                planes.append(traj.read_all())
            logits = pol.seq_forward(traj, want_succ=False)[0]
            runs[variant] = (planes, env.step(np.arange(n, dtype=np.uint8) % 2), logits, pol.get_params(), shape)
    finally:
        engine.set_kernel_variant(0)
    fused, stepwise = runs[0], runs[1]
    for period in range(2):
        for key in PLANES:  # whole planes: obs[T] and every term_obs entry included
            assert np.array_equal(fused[0][period][key], stepwise[0][period][key]), (period, key)
    (reward_f, flag_f, obs_f, term_f), (reward_s, flag_s, obs_s, term_s) = fused[1], stepwise[1]
    assert np.array_equal(reward_f, reward_s) and np.array_equal(flag_f, flag_s) and np.array_equal(obs_f, obs_s)
    assert np.array_equal(term_f[:, flag_f == M.INTERRUPT], term_s[:, flag_s == M.INTERRUPT])  # (valid where cut)
    # the env side through the restatement, both periods in a row
    ref = M.MetaLanes(n, 2, E, seed_env=seed_env)
    r = O.Prng()
    for period in range(2):
        got = fused[0][period]
        want = ref.replay(got["action"])
        for key in ("obs", "reward", "flag"):
            assert np.array_equal(got[key], want[key]), (period, key)
        cut = got["flag"] == M.INTERRUPT
        assert cut.any() and np.array_equal(got["term_obs"][:, cut], want["term_obs"][:, cut])
    assert (fused[0][1]["flag"][:2] == M.INTERRUPT).any()  # a trial that began before the horizon ends after it
    # the actions of the second period at the logits of the teacher-forced forward (the comparison of
    # tests/test_gpu_stacked.py::test_rollout_on_cartpole_lanes)
    got, params, shape = fused[0][1], fused[3], fused[4]
    z, _ = O.stack_seq_forward(shape, 1, params, got, want_succ=False)
    assert np.array_equal(z, fused[2])
    checked = 0
    for t in range(T):
        p0 = 1.0 / (1.0 + np.exp(z[1, t].astype(np.float64) - z[0, t]))
        for i in range(n):
            L.oracle_prng_seed_from_u64(C.byref(r), seed_actor)
            L.oracle_prng_set_stream(C.byref(r), i)
            L.oracle_prng_set_word_pos(C.byref(r), T + t)
            u = L.oracle_prng_gen_f32(C.byref(r))
            if abs(u - p0[i]) > 1e-6:
                assert got["action"][t, i] == (0 if u < p0[i] else 1), (t, i)
                checked += 1
    assert checked > 0.99 * n * T


# ------------------------------------------------------------------------------------------------ 5. updates
def test_updates_do_not_see_the_env_kind(engine):
    """GAE with a recurrent critic and a TRPO update on the collected trajectory equal the same calls on a trajectory
    filled from its planes through rl_traj_write; the device StepsSummary counts a trial as an episode"""
    n, T, E = 70, 13, 3
    env = ra.MetaBanditEnv(engine, n, 2, E, seed_env=3, seed_actor=4)
    results = []
    planes = None
    for source in ("rollout", "written"):
        pol, _ = recurrent_policy(engine, "gru", env.D, 12, 8, 2, 31)
        cri, _ = recurrent_policy(engine, "lstm", env.D, 8, 8, 1, 32)
        traj = ra.Trajectory(engine, n, T, env.D)
        if source == "rollout":
            ra.rollout(env, pol, traj)
            planes = traj.read_all()
            summary = ra.StepsSummary(engine, n)
            summary.push(traj)
            stats = summary.read()
        else:
            traj.write_all(planes)
        ra.gae(traj, cri, 0.99, 0.3)
        st = ra.trpo_update(pol, traj)
        results.append((traj.read(ra.TRAJ_ADVANTAGES), traj.read(ra.TRAJ_RETURNS), pol.get_params(), st.as_dict()))
    a, b = results
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert a[3]["status"] == ra.OPT_OK and np.abs(a[0]).max() > 0
    # StepsSummary against NumPy: completed trials = Interrupts, their reward sums and lengths
    flag, reward = planes["flag"], planes["reward"].astype(np.float64)
    sums, lens = [], []
    for i in range(n):
        acc, length = 0.0, 0
        for t in range(T):
            acc, length = acc + reward[t, i], length + 1
            if flag[t, i] != M.CONTINUE:
                sums.append(acc), lens.append(length)
                acc, length = 0.0, 0
    assert stats.episode_reward.count == np.count_nonzero(flag == M.INTERRUPT) == len(sums) == 2 * n
    assert abs(stats.episode_reward.mean - np.mean(sums)) < 1e-12
    assert stats.episode_length.mean == 2 * E - 1 and set(lens) == {2 * E - 1}
    assert stats.step_reward.count == n * T and abs(stats.step_reward.mean - reward.mean()) < 1e-12


# ------------------------------------------------------------------------------------------------ 6. refusals
def code_of(f):
    with pytest.raises(ra.RelearnError) as e:
        f()
    return e.value.code, str(e.value)


def test_refusals(engine):
    n = 8
    for bad in (dict(n_arms=1), dict(n_arms=5), dict(episodes_per_trial=0), dict(distribution=7),
                dict(limit=ra.LIMIT_LATENT, max_steps=5), dict(limit=ra.LIMIT_VISIBLE, max_steps=5)):
        assert code_of(lambda: ra.MetaBanditEnv(engine, n, **bad))[0] == ra.ERR_BUILD_ENV, bad
    cfg = ra.EnvConfig()
    cfg.kind, cfg.n_lanes, cfg.cartpole = ra.ENV_META_BANDIT, n, ra.cartpole_params_default()
    h = C.c_void_p()
    assert ra.lib().rl_env_create(engine.h, C.byref(cfg), C.byref(h)) == ra.ERR_BUILD_ENV  # only through its own entry point
    assert ra.lib().rl_env_create_meta_bandit(engine.h, C.byref(cfg), None, C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    for k in (2, 3, 4):
        env = ra.MetaBanditEnv(engine, n, k, 2, "one_hot")
        assert (env.D, env.A) == (k + 4, k)
    env = ra.MetaBanditEnv(engine, n)  # the defaults: two arms, uniform Bernoulli, ten episodes
    assert (env.D, env.A, env.meta.episodes_per_trial) == (6, 2, 10)
    code, msg = code_of(env.get_state)
    assert code == ra.ERR_UNSUPPORTED and "rl_env_get_state" in msg
    code, msg = code_of(lambda: env.set_state(np.zeros((4, n)), np.zeros(n), np.zeros(n), np.zeros(n)))
    assert code == ra.ERR_UNSUPPORTED and "rl_env_set_state" in msg
    qnet = ra.Mlp(engine, 6, [16], 2)
    qnet.init(1)
    dcfg = ra.dqn_config_default()
    dcfg.buffer_capacity, dcfg.minibatch_steps = 64, 32
    code, msg = code_of(lambda: ra.Dqn(env, qnet, ra.Adam(qnet), dcfg))
    assert code == ra.ERR_UNSUPPORTED and "rl_dqn_create" in msg
    code, msg = code_of(lambda: ra.actor_to_cbor(env, qnet))
    assert code == ra.ERR_UNSUPPORTED and "rl_actor_to_cbor" in msg
    # recurrent chains are built for two actions: three arms are refused by rl_rollout's existing rule
    env3 = ra.MetaBanditEnv(engine, n, 3, 2)
    gru = ra.GruMlp(engine, 7, 2, 8, 8)
    gru.init(1)
    assert code_of(lambda: ra.rollout(env3, gru, ra.Trajectory(engine, n, 4, 7)))[0] == ra.ERR_UNSUPPORTED
    # ... and a feed-forward policy must have one output per arm
    assert code_of(lambda: ra.rollout(env3, qnet, ra.Trajectory(engine, n, 4, 7)))[0] == ra.ERR_INVALID_ARGUMENT
    with pytest.raises(ra.RelearnError):
        env.step(np.full(n, 2, np.uint8))  # an action index outside IndexSpace::new(2)


# ------------------------------------------------------------------------------------------------ 7. learning
def test_a_recurrent_policy_learns_to_use_its_memory(engine):
    """OneHotBandits(2), five episodes per trial, GRU chains as policy and critic, rl_actor_critic_update (TRPO + critic
    fitting, GAE lambda 0.3).  A policy without memory across inner episodes pulls the good arm with probability 1/2 in
    expectation over the trial's draw whatever it does: exactly E / 2 = 2.5 per trial, variance at most E^2 / 4, so the
    standard error over 4,096 evaluation trials is at most 0.04.  The bar is a mean trial reward above 3.0 (0.6 E); the
    policy that remembers (try an arm, stay on a hit, switch on a miss) earns 4.5.
    Measured on an MI355X with this configuration (and with a second seed, and with 4,096 lanes of one trial each): the
    evaluation mean first exceeds 3.0 after 6 periods (3.22; 3.12; 3.17) and is 4.37 after 12 (4.43 with 4,096 lanes).
    The test runs 12 = twice the smallest sufficient count; a period takes about 0.03 s."""
    n, E, trials, H, periods, seed = 1024, 5, 2, 32, 12, 40
    T = trials * (2 * E - 1)
    env = ra.MetaBanditEnv(engine, n, 2, E, "one_hot", seed_env=seed, seed_actor=seed + 1)
    pol, cri = ra.GruMlp(engine, env.D, 2, H, H), ra.GruMlp(engine, env.D, 1, H, H)
    pol.init(seed + 2)
    cri.init(seed + 3)
    opt = ra.Adam(cri)
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = 10
    traj = ra.Trajectory(engine, n, T, env.D)
    for _ in range(periods):
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.3)
        ra.actor_critic_update(pol, cri, opt, traj, None, ccfg)
    ev_env = ra.MetaBanditEnv(engine, 4096, 2, E, "one_hot", seed_env=seed + 10, seed_actor=seed + 11)
    ev_traj = ra.Trajectory(engine, 4096, 2 * E - 1, env.D)  # one whole trial per lane
    ra.rollout(ev_env, pol, ev_traj)
    assert np.all(ev_traj.read(ra.TRAJ_FLAG)[-1] == M.INTERRUPT)
    trial_reward = ev_traj.read(ra.TRAJ_REWARD).astype(np.float64).sum(axis=0)
    print("mean trial reward after %d periods: %.3f (se %.3f)" % (periods, trial_reward.mean(), trial_reward.std() / 64.0))
    assert trial_reward.mean() > 3.0
