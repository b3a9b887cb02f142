"""The meta-MDP lanes on the device — rl_env_create_meta_mdp / ra.MetaMdpEnv, MetaEnv<DirichletRandomMdps> under an inner
LatentStepLimit and a TrialEpisodeLimit, every lane drawing its own MDP at each trial's start — against the Python
restatement (tests/meta_mdp_ref.py; its cases are pinned on the CPU by tests/test_meta_mdp_ref.py):

  driven steps   70 lanes and the 45 lanes at offset 25, three trials and a step: rewards, flags, both observations and
                 term_obs after every step, the tables read back after every step (so after every reset), bit for bit
  statistics     4,096 lanes, first step: reward mean and variance, successor counts, at 4.4 sigma
  updates        one TRPO and one PPO update on a collected trajectory equal the same call on a host-written copy
  refusals       every refusal with its code and its entry point's name

The closed loop is tests/test_gpu_meta_mdp_rollout.py.  Every test here fails on a library without the constructor."""
import ctypes as C

import numpy as np
import pytest

import meta_mdp_ref as M
import relearn_amd as ra
import seq_multi_ref as R

pytestmark = pytest.mark.gpu


def make_env(engine, d, n, seed, offset=0, seed_actor=1):
    return ra.MetaMdpEnv(engine, n, d.S, d.A, max_inner_steps=d.L, episodes_per_trial=d.E, alpha=d.alpha,
                         reward_prior_mean=d.prior_mean, reward_prior_stddev=d.prior_stddev,
                         reward_stddev=d.reward_stddev, lane_offset=offset, seed_env=seed, seed_actor=seed_actor)


def code_of(fn):
    with pytest.raises(ra.RelearnError) as e:
        fn()
    return e.value.code, str(e.value)


# ------------------------------------------------------------------------------------------------ 1. driven steps
@pytest.mark.parametrize("c", M.DRIVEN, ids=M.driven_id)
def test_driven_steps_bit_for_bit(engine, c):
    d, n, off = c.dist, M.N_LANES, M.OFFSET
    ref = M.driven_reference(c)
    env, tail = make_env(engine, d, n, c.seed), make_env(engine, d, n - off, c.seed, offset=off)
    assert (env.D, env.A, env.trial_steps) == (d.S + d.A + 4, d.A, M.trial_steps(d))
    assert np.array_equal(env.observe(), ref.observe0) and np.array_equal(tail.observe(), ref.observe0[:, off:])
    cum, mean = env.read_tables()
    assert np.array_equal(cum, ref.tables0[0]) and np.array_equal(mean, ref.tables0[1])
    cum, mean = tail.read_tables()  # tables are indexed by the local lane, streams by the global one
    assert np.array_equal(cum, ref.tables0[0][off:]) and np.array_equal(mean, ref.tables0[1][off:])
    cum, mean = env.read_tables(first_lane=off, n=3)
    assert np.array_equal(cum, ref.tables0[0][off:off + 3]) and np.array_equal(mean, ref.tables0[1][off:off + 3])
    cuts = 0
    for t, (a, (reward_o, flag_o, obs_o, term_o, tables_o)) in enumerate(zip(ref.actions, ref.steps)):
        reward, flag, obs, term = env.step(a)
        assert np.array_equal(reward, reward_o) and np.array_equal(flag, flag_o), t
        assert np.array_equal(obs, obs_o), t
        assert np.array_equal(env.observe(), obs_o), t  # ... and from the stored lane
        cut = flag == M.INTERRUPT
        assert np.array_equal(term[:, cut], term_o[:, cut]), t
        cum, mean = env.read_tables()
        assert np.array_equal(cum, tables_o[0]) and np.array_equal(mean, tables_o[1]), t
        reward_t, flag_t, obs_t, term_t = tail.step(a[off:])
        assert np.array_equal(reward_t, reward_o[off:]) and np.array_equal(flag_t, flag_o[off:]), t
        assert np.array_equal(obs_t, obs_o[:, off:]) and np.array_equal(term_t[:, cut[off:]], term_o[:, off:][:, cut[off:]]), t
        cum, mean = tail.read_tables()
        assert np.array_equal(cum, tables_o[0][off:]) and np.array_equal(mean, tables_o[1][off:]), t
        cuts += int(cut.all())
    assert cuts == M.driven_steps(c) // M.trial_steps(d) >= M.TRIALS  # every lane ends its trials at the same steps
    with pytest.raises(ra.RelearnError):
        env.step(np.full(n, d.A, np.uint8))  # an action index outside IndexSpace::new(A)


def test_reset_in_the_middle_of_a_trial_draws_where_the_stream_stands(engine):
    d = M.dist(3, 2, 2, 3)
    env, ref = make_env(engine, d, 70, 21), M.MetaMdpLanes(70, d, seed_env=21)
    rs = np.random.default_rng(4)
    for t in range(9):
        if t == 4:
            env.reset(), ref.reset()
            assert np.array_equal(env.observe(), ref.observe())
            assert np.array_equal(env.read_tables()[0], ref.tables()[0]) and np.array_equal(env.read_tables()[1], ref.tables()[1])
        a = rs.integers(0, d.A, 70).astype(np.uint8)
        got, want = env.step(a), ref.step(a)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), t


# ------------------------------------------------------------------------------------------------ 2. statistics
SIGMAS = 4.4  # the project's


@pytest.mark.parametrize("S,A,alpha,sd", [(5, 5, 1.0, 1.0), (8, 4, 0.5, 0.5), (4, 8, 2.5, 2.0)])
def test_first_step_statistics(engine, S, A, alpha, sd):
    """4,096 independent lanes, all in state 0 at their first step, lane i taking action i mod A.  The row's mean is
    N(prior_mean, prior_stddev^2) and the reward adds N(0, reward_stddev^2): the reward is normal with the prior's mean and
    variance prior_stddev^2 + reward_stddev^2 (the mean of n of them has standard deviation sigma / sqrt(n), their sample
    variance sigma^2 sqrt(2 / (n - 1))).  A symmetric Dirichlet row gives every successor probability 1 / S: a count is
    Binomial(n, 1 / S)."""
    n, pm, ps = 4096, 1.0, 1.5
    d = M.dist(S, A, 2, 2, alpha=alpha, prior_mean=pm, prior_stddev=ps, reward_stddev=sd)
    env = make_env(engine, d, n, 31 + S)
    reward, flag, obs, _ = env.step((np.arange(n) % A).astype(np.uint8))
    assert np.all(flag == M.CONTINUE) and np.all(np.isfinite(reward))
    var = ps * ps + sd * sd
    r = reward.astype(np.float64)
    print("S=%d A=%d: reward mean %.4f (want %.1f +- %.4f), variance %.4f (want %.4f +- %.4f)" % (
        S, A, r.mean(), pm, SIGMAS * np.sqrt(var / n), r.var(ddof=1), var, SIGMAS * var * np.sqrt(2.0 / (n - 1))))
    assert abs(r.mean() - pm) <= SIGMAS * np.sqrt(var / n)
    assert abs(r.var(ddof=1) - var) <= SIGMAS * var * np.sqrt(2.0 / (n - 1))
    assert np.all(obs[1:1 + S].sum(0) == 1)
    counts = obs[1:1 + S].sum(1)
    bound = SIGMAS * np.sqrt(n * (1.0 / S) * (1.0 - 1.0 / S))
    print("successor counts", counts, "want %.1f +- %.1f" % (n / S, bound))
    assert np.all(np.abs(counts - n / S) <= bound)
    assert np.array_equal(obs[2 + S:2 + S + A].argmax(0), np.arange(n) % A) and np.array_equal(obs[S + A + 2], reward)


# ------------------------------------------------------------------------------------------------ 3. whole updates
@pytest.mark.parametrize("update", ["trpo", "ppo"])
def test_updates_on_a_collected_trajectory_equal_the_written_one(engine, update):
    d = M.dist(5, 5, 2, 2)
    n, T_ = 70, 12
    pnet, cnet = R.Net("gru", 14, 12, 1, 0, True, 5), R.Net("gru", 14, 8, 1, 0, True, 1)
    results, planes = [], None
    for source in ("rollout", "written"):
        env = make_env(engine, d, n, 3, seed_actor=4)
        pol = ra.RnnChainWide(engine, pnet.cell, pnet.D, pnet.H, pnet.A, num_layers=1, bias=True, mlp_hidden=None)
        cri = ra.RnnChainWide(engine, cnet.cell, cnet.D, cnet.H, cnet.A, num_layers=1, bias=True, mlp_hidden=None)
        pol.init(31), cri.init(32)
        traj = ra.Trajectory(engine, n, T_, env.D)
        if source == "rollout":
            ra.rollout(env, pol, traj)
            planes = traj.read_all()
            assert sorted(np.unique(planes["action"])) == list(range(d.A))
            assert (planes["flag"] == M.INTERRUPT).sum() == 2 * n  # trials of 5 steps in 12
        else:
            traj.write_all(planes)
        ra.gae(traj, cri, 0.99, 0.3)
        if update == "trpo":
            st = ra.trpo_update(pol, traj)
            assert st.status == ra.OPT_OK and st.loss_final < st.loss_initial
            extra = (st.as_dict(),)
        else:
            cfg = ra.ppo_config_default()
            cfg.opt_steps_per_update = 3
            _, losses = ra.ppo_update(pol, ra.Adam(pol), traj, cfg, want_losses=True)
            assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]
            extra = (losses.tobytes(),)
        assert not np.array_equal(pol.get_params(), R.init(pnet, 31)) and np.all(np.isfinite(pol.get_params()))
        results.append((traj.read(ra.TRAJ_ADVANTAGES).tobytes(), pol.get_params().tobytes(), extra))
    assert results[0] == results[1]


# ------------------------------------------------------------------------------------------------ 4. refusals
def config(**kw):
    m = ra.meta_mdp_config_default()
    for k, v in kw.items():
        setattr(m, k, v)
    return m


BAD_CONFIGS = [
    dict(n_states=1), dict(n_states=9), dict(n_actions=1), dict(n_actions=9), dict(n_states=8, n_actions=5),
    dict(n_states=10, n_actions=5), dict(max_inner_steps=0), dict(max_inner_steps=1 << 32), dict(episodes_per_trial=0),
    dict(episodes_per_trial=1 << 32), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("inf")), dict(alpha=float("nan")),
    dict(reward_prior_stddev=-0.5), dict(reward_prior_stddev=float("nan")), dict(reward_stddev=-1.0),
    dict(reward_stddev=float("inf")), dict(reward_prior_mean=float("nan")), dict(discount_factor=float("inf")),
]


@pytest.mark.parametrize("bad", BAD_CONFIGS, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_constructor_refusals(engine, bad):
    code, text = code_of(lambda: ra.MetaMdpEnv(engine, 8, meta=config(**bad)))
    assert code == ra.ERR_BUILD_ENV and "rl_env_create_meta_mdp" in text, text


def test_constructor_refuses_a_step_limit_and_bad_lanes_and_the_generic_constructors_refuse_the_kind(engine):
    code, text = code_of(lambda: ra.MetaMdpEnv(engine, 8, limit=ra.LIMIT_LATENT, max_steps=10))
    assert code == ra.ERR_BUILD_ENV and "rl_env_create_meta_mdp" in text and "step limit" in text
    assert code_of(lambda: ra.MetaMdpEnv(engine, 0))[0] == ra.ERR_BUILD_ENV
    cfg = ra.EnvConfig()
    cfg.kind, cfg.n_lanes, cfg.cartpole = ra.ENV_META_MDP, 8, ra.cartpole_params_default()
    h = C.c_void_p()
    assert ra.lib().rl_env_create(engine.h, C.byref(cfg), C.byref(h)) == ra.ERR_BUILD_ENV
    assert "rl_env_create_meta_mdp" in ra.lib().rl_last_error(engine.h).decode()
    meta = config()
    assert ra.lib().rl_env_create_meta_mdp(engine.h, C.byref(cfg), None, C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    assert ra.lib().rl_env_create_meta_mdp(engine.h, None, C.byref(meta), C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    assert ra.lib().rl_env_create_meta_mdp(engine.h, C.byref(cfg), C.byref(meta), None) == ra.ERR_INVALID_ARGUMENT


def test_entry_points_not_built_for_these_lanes_refuse_by_name(engine):
    d = M.dist(2, 2, 2, 2)
    env = make_env(engine, d, 8, 5)
    for fn, name in ((env.get_state, "rl_env_get_state"),
                     (lambda: env.set_state(np.zeros((4, 8)), np.zeros(8, np.int32), np.zeros(8, np.uint64),
                                            np.zeros(8, np.uint64)), "rl_env_set_state")):
        code, text = code_of(fn)
        assert code == ra.ERR_UNSUPPORTED and name in text and "RL_ENV_META_MDP" in text, text
    ff = ra.Mlp(engine, env.D, [16], env.A)  # (eight inputs: the per-layer kernels)
    rec = ra.RnnChainWide(engine, "gru", env.D, 8, env.A, num_layers=1, bias=True, mlp_hidden=6)
    lib, dq, out = ra.lib(), ra.dqn_config_default(), C.c_void_p()
    for mod in (ff, rec):
        opt = ra.Adam(mod)
        for name in ("rl_dqn_create", "rl_dqn_create_recurrent", "rl_dqn_create_finite"):
            rc = getattr(lib, name)(env.h, mod.h, opt.h, C.byref(dq), C.byref(out))
            text = lib.rl_last_error(engine.h).decode()
            if name == "rl_dqn_create_recurrent" and mod is ff:  # on every env: it hears of its module first
                assert rc == ra.ERR_BUILD_AGENT and name in text
                continue
            assert rc == ra.ERR_UNSUPPORTED and name in text and "RL_ENV_META_MDP" in text, (name, rc, text)
        n = C.c_uint64()
        rc = lib.rl_actor_to_cbor(env.h, mod.h, C.c_int32(ra.ACTOR_POLICY), C.c_double(0.0), None, C.c_uint64(0), C.byref(n))
        text = lib.rl_last_error(engine.h).decode()
        assert rc == ra.ERR_UNSUPPORTED and "rl_actor_to_cbor" in text and "RL_ENV_META_MDP" in text, text
    bc, agent = ra.BanditAgentConfig(), C.c_void_p()
    assert lib.rl_bandit_agent_config_default(C.c_int32(ra.BANDIT_AGENT_RANDOM), C.byref(bc)) == ra.OK
    rc = lib.rl_bandit_agent_create(env.h, C.byref(bc), C.byref(agent))
    text = lib.rl_last_error(engine.h).decode()
    assert rc == ra.ERR_UNSUPPORTED and "rl_bandit_agent_create" in text, text
    # ... and the table read-back is these lanes' alone
    other = ra.MetaBanditEnv(engine, 8, 2, 3)
    buf = np.zeros(64, np.float64)
    rc = lib.rl_env_meta_mdp_read_tables(other.h, C.c_uint64(0), C.c_uint64(1), None, buf.ctypes.data_as(C.c_void_p))
    assert rc == ra.ERR_UNSUPPORTED and "rl_env_meta_mdp_read_tables" in lib.rl_last_error(engine.h).decode()
    assert code_of(lambda: env.read_tables(first_lane=7, n=2))[0] == ra.ERR_INVALID_ARGUMENT
    # the lanes still step after all of that
    assert env.step(np.zeros(8, np.uint8))[2].shape == (env.D, 8)


def test_feed_forward_policy_on_two_by_two(engine):
    """a feed-forward module has at most eight inputs: it fits 2 x 2 alone, through the launch sequence per step"""
    d = M.dist(2, 2, 2, 2)
    env = make_env(engine, d, 70, 8)
    pol = ra.Mlp(engine, env.D, [16], env.A)
    pol.init(3)
    traj = ra.Trajectory(engine, 70, 11, env.D)
    ra.rollout(env, pol, traj)
    planes = traj.read_all()
    ref = M.MetaMdpLanes(70, d, seed_env=8)
    obs0 = ref.observe()
    assert np.array_equal(planes["obs"][:, 0], obs0)
    for t in range(11):  # the env's side of the trajectory, replayed at the recorded actions
        reward, flag, obs, term = ref.step(planes["action"][t])
        assert np.array_equal(planes["reward"][t], reward) and np.array_equal(planes["flag"][t], flag), t
        assert np.array_equal(planes["obs"][:, t + 1], obs), t
        cut = flag == M.INTERRUPT
        assert np.array_equal(planes["term_obs"][:, t][:, cut], term[:, cut]), t
    assert (planes["flag"] == M.INTERRUPT).sum() == 2 * 70
