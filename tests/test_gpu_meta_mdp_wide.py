"""The RL2 random-MDP lanes at the reference's size on the device — rl_env_create_meta_mdp_wide / ra.MetaMdpEnvWide (up to
10 states and 20 features: DirichletRandomMdps::default's 10 x 5 has 19), rl_rnn_chain_create_wide20 / ra.RnnChainWide20
(up to 20 inputs) and rl_traj_create_wide / ra.TrajectoryWide (up to 20 planes) — against the Python lanes of
tests/meta_mdp_ref.py at the cases of tests/meta_mdp_wide_cases.py (pinned on the CPU by tests/test_meta_mdp_wide_cases.py):

  driven steps   every case of the table on 70 lanes and on the 45 lanes at offset 25, three trials and a step: rewards,
                 successor codes, both observations and term_obs after every step, the tables read back after every step
                 (so after every reset), bit for bit; a reset in the middle of a trial
  f64            gradient, Fisher-vector product and the clipped PPO gradient of 19-input chains at the bars of
                 tests/test_gpu_seq_multi_action.py: 5e-6, 2e-5, 5e-6 of max |g|
  updates        one TRPO and one PPO update on a collected trajectory equal the same call on a host-written copy
  statistics     4,096 lanes at 10 x 5, first step, at 4.4 sigma
  refusals       every refusal of the three new entry points; the three older ones keep their answers at 10 x 5, 17
                 inputs and 17 planes; inside the older ranges the new ones build the older ones' handles

The closed loop is tests/test_gpu_meta_mdp_wide_rollout.py.  Every test here fails on a library without the entry points."""
import ctypes as C

import numpy as np
import pytest

import meta_mdp_ref as M
import meta_mdp_wide_cases as W
import relearn_amd as ra
import seq_multi_ref as R
from oracle import stacked as S
from test_gpu_stacked import GRAD_RTOL, rel_err

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -24


def make_env(engine, d, n, seed, offset=0, seed_actor=1, cls=None):
    cls = cls or ra.MetaMdpEnvWide
    return cls(engine, n, d.S, d.A, max_inner_steps=d.L, episodes_per_trial=d.E, alpha=d.alpha,
               reward_prior_mean=d.prior_mean, reward_prior_stddev=d.prior_stddev, reward_stddev=d.reward_stddev,
               lane_offset=offset, seed_env=seed, seed_actor=seed_actor)


def module(engine, net, seed=None):
    m = ra.RnnChainWide20(engine, net.cell, net.D, net.H, net.A, num_layers=net.L, bias=net.bias, mlp_hidden=net.H2 or None)
    assert m.P == R.num_params(net)
    if seed is not None:
        m.init(seed)
    return m


def code_of(fn):
    with pytest.raises(ra.RelearnError) as e:
        fn()
    return e.value.code, str(e.value)


# ------------------------------------------------------------------------------------------------ 1. driven steps
@pytest.mark.parametrize("c", W.DRIVEN, ids=W.driven_id)
def test_driven_steps_bit_for_bit(engine, c):
    d, n, off = c.dist, W.N_LANES, W.OFFSET
    ref = W.driven_reference(c)
    env, tail = make_env(engine, d, n, c.seed), make_env(engine, d, n - off, c.seed, offset=off)
    assert (env.D, env.A, env.trial_steps) == (d.S + d.A + 4, d.A, M.trial_steps(d))
    assert np.array_equal(env.observe(), ref.observe0) and np.array_equal(tail.observe(), ref.observe0[:, off:])
    cum, mean = env.read_tables()  # at the logical width S, whatever the padded row is
    assert cum.shape == (n, d.S, d.A, d.S)
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
    assert cuts == W.driven_steps(c) // M.trial_steps(d) >= W.TRIALS
    with pytest.raises(ra.RelearnError):
        env.step(np.full(n, d.A, np.uint8))  # an action index outside IndexSpace::new(A)


def test_reset_in_the_middle_of_a_trial_draws_where_the_stream_stands(engine):
    d = M.dist(10, 5, 2, 3)
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


# ------------------------------------------------------------------------------------------------ 2. f64 comparisons
NETS = [R.Net("gru", 19, 8, 1, 0, True, 5), R.Net("lstm", 19, 8, 1, 6, True, 5), R.Net("gru", 19, 33, 2, 6, False, 5)]
CRITIC = R.Net("gru", 19, 8, 1, 0, True, 1)  # the critic of 10 x 5 lanes: 19 inputs, one output
T = 5


def written(engine, net, n, seed, T_=T):
    h = R.history(net, n, T_, seed)
    traj = ra.TrajectoryWide(engine, n, T_, net.D)
    traj.write_all(h)
    traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
    traj.write(ra.TRAJ_RETURNS, h["rtg"])
    return traj, h


@pytest.mark.parametrize("net", NETS + [CRITIC], ids=R.net_id)
def test_initialisation_and_forward_are_bit_exact(engine, net):
    import oracle as O
    m = module(engine, net, 31)
    assert np.array_equal(m.get_params(), R.init(net, 31))
    traj, h = written(engine, net, 70, 5)
    out_d, succ_d = m.seq_forward(traj)
    out_o, succ_o = O.stack_seq_forward(R.shape_of(net), net.L, R.to_oracle(net, m.get_params()), h)
    assert out_d.shape == (net.A, T, 70)
    assert np.array_equal(out_d, out_o) and np.array_equal(succ_d, succ_o)
    # every one of the 19 input columns reaches the output: zeroing plane d changes it
    for dd in (16, 17, 18):
        h2 = dict(h)
        h2["obs"] = h["obs"].copy()
        h2["obs"][dd] = 0.0
        traj.write_all(h2)
        assert not np.array_equal(m.seq_forward(traj)[0], out_d), dd


@pytest.mark.parametrize("net", NETS, ids=R.net_id)
def test_gradient_and_fvp_against_f64(engine, net):
    """rl_policy_gradient and rl_policy_fvp on a host-written trajectory at the bars tests/test_gpu_seq_multi_action.py
    uses: GRAD_RTOL = 5e-6 for the gradient, 2e-5 for the Fisher-vector product.  Measured on an MI355X: see DESIGN §47."""
    assert GRAD_RTOL == 5e-6
    n = 70
    m = module(engine, net, 41)
    traj, h = written(engine, net, n, 6)
    assert sorted(np.unique(h["action"])) == list(range(net.A))
    spec, p = R.spec_of(net), m.get_params()
    full = R.to_oracle(net, p)
    logits, _, _ = S.forward(spec, full, h, want_succ=False)
    dz, loss64, ent64 = R.surrogate_dlogits(logits, h["action"], h["adv"])
    g64 = R.restrict(net, S.backward(spec, full, h, dz))
    g_d, loss_d, ent_d = ra.policy_gradient(m, traj)
    e_g = rel_err(g_d, g64)
    v = np.random.default_rng(3).normal(size=m.P).astype(np.float32)
    h64 = R.restrict(net, S.policy_fvp(spec, full, R.to_oracle(net, v, tangent=True), h, 1e-5))
    h_d = ra.policy_fvp(m, traj, v, 1e-5)
    e_h = rel_err(h_d, h64)
    print("%s: gradient rel err %.3g (bar %.3g), fvp rel err %.3g (bar 2e-05)" % (R.net_id(net), e_g, GRAD_RTOL, e_h))
    assert g_d.shape == g64.shape and e_g < GRAD_RTOL, e_g
    assert e_h < 2e-5, e_h
    assert abs(loss_d - loss64) <= 2e-5 * abs(loss64) + 1e-7 and abs(ent_d - ent64) <= 2e-5 * abs(ent64) + 1e-7
    for name, l, shp, o, _ in R.blocks(net):  # every block receives gradient: all 19 columns of W_ih among them
        s = slice(o, o + int(np.prod(shp)))
        assert np.abs(g_d[s]).max() > 0, (name, l)
    wih = g_d[:R.blocks(net)[0][2][0] * net.D].reshape(-1, net.D)
    assert np.all(np.abs(wih).max(0) > 0)


def sgd_steps(pol, traj, p0, lr, steps, clip):
    cfg = ra.optimizer_config_default(ra.OPTIMIZER_SGD)
    cfg.learning_rate = lr
    step = ra.ppo_config_default()
    step.opt_steps_per_update, step.clip_distance = steps, clip
    pol.set_params(p0)
    opt = ra.Optimizer(pol, cfg)
    try:
        _, losses = ra.ppo_update(pol, opt, traj, step, want_losses=True)
        return pol.get_params(), losses.astype(np.float64)
    finally:
        opt.close()


PPO_NET, PPO_LR, PPO_N, PPO_INIT_SEED, PPO_HISTORY_SEED = R.Net("gru", 19, 12, 1, 6, True, 5), 16.0, 70, 51, 8


def test_clipped_ppo_gradient_off_ratio_one(engine):
    """tests/test_gpu_seq_multi_action.py's method and bar at 19 inputs: under plain SGD from p0, one rl_ppo_update step
    gives p1 and two give p2; (p1 - p2) / lr is the clipped gradient AT p1, against the f64 restatement at clip distances
    0.2 and 0; the bar is GRAD_RTOL of max |g| plus the readback term of element j"""
    net, lr = PPO_NET, PPO_LR
    m = module(engine, net, PPO_INIT_SEED)
    traj, h = written(engine, net, PPO_N, PPO_HISTORY_SEED)
    spec, p0 = R.spec_of(net), m.get_params()
    z0, _, _ = S.forward(spec, R.to_oracle(net, p0), h, want_succ=False)
    for clip in (0.2, 0.0):
        p1, _ = sgd_steps(m, traj, p0, lr, 1, clip)
        p2, losses = sgd_steps(m, traj, p0, lr, 2, clip)
        assert not np.array_equal(p1, p0) and np.all(np.isfinite(p2))
        full1 = R.to_oracle(net, p1)
        z1, _, _ = S.forward(spec, full1, h, want_succ=False)
        dz, loss64, ratio = R.ppo_dlogits(z1, z0, h["action"], h["adv"], clip)
        g64 = R.restrict(net, S.backward(spec, full1, h, dz))
        lo, hi = 1.0 - clip, 1.0 + clip
        margin = min(np.abs(ratio - lo).min(), np.abs(ratio - hi).min())
        clipped = ((h["adv"] > 0) & (ratio > hi)) | ((h["adv"] < 0) & (ratio < lo))
        print("%s clip %.1f: %d of %d samples clipped, nearest ratio to a bound %.3g" % (
            R.net_id(net), clip, clipped.sum(), ratio.size, margin))
        assert margin > 1e-4 and clipped.sum() >= 0.05 * ratio.size and (~clipped).sum() >= 0.05 * ratio.size
        g_dev = (p1.astype(np.float64) - p2.astype(np.float64)) / lr
        readback = ULP * (np.abs(p2.astype(np.float64)) + lr * np.abs(g64)) / lr
        diff, gmax = np.abs(g_dev - g64), np.abs(g64).max()
        print("%s clip %.1f: device error %.3g of max|g|, %.3g beyond the readback term (bar %.3g)" % (
            R.net_id(net), clip, diff.max() / gmax, np.maximum(diff - readback, 0.0).max() / gmax, GRAD_RTOL))
        assert np.all(diff <= GRAD_RTOL * gmax + readback)
        assert abs(losses[1] - loss64) <= 2e-5 * max(1.0, abs(loss64))


# ------------------------------------------------------------------------------------------------ 3. whole updates
@pytest.mark.parametrize("update", ["trpo", "ppo"])
def test_updates_on_a_collected_trajectory_equal_the_written_one(engine, update):
    d = M.dist(10, 5, 2, 2)
    n, T_ = 70, 12
    pnet, cnet = R.Net("gru", 19, 12, 1, 0, True, 5), CRITIC
    results, planes = [], None
    for source in ("rollout", "written"):
        env = make_env(engine, d, n, 3, seed_actor=4)
        pol, cri = module(engine, pnet, 31), module(engine, cnet, 32)
        traj = ra.TrajectoryWide(engine, n, T_, env.D)
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


# ------------------------------------------------------------------------------------------------ 4. statistics
SIGMAS = 4.4  # the project's


def test_first_step_statistics_at_ten_by_five(engine):
    """4,096 independent lanes, all in state 0 at their first step, lane i taking action i mod A: the reward is normal with
    the prior's mean and variance prior_stddev^2 + reward_stddev^2; a symmetric Dirichlet row gives every one of the TEN
    successors probability 1 / 10, so a count is Binomial(n, 1 / 10) — states 8 and 9 among them."""
    S_, A, n, pm, ps, sd = 10, 5, 4096, 1.0, 1.5, 1.0
    d = M.dist(S_, A, 2, 2, prior_mean=pm, prior_stddev=ps, reward_stddev=sd)
    env = make_env(engine, d, n, 41)
    reward, flag, obs, _ = env.step((np.arange(n) % A).astype(np.uint8))
    assert np.all(flag == M.CONTINUE) and np.all(np.isfinite(reward))
    var = ps * ps + sd * sd
    r = reward.astype(np.float64)
    print("reward mean %.4f (want %.1f +- %.4f), variance %.4f (want %.4f +- %.4f)" % (
        r.mean(), pm, SIGMAS * np.sqrt(var / n), r.var(ddof=1), var, SIGMAS * var * np.sqrt(2.0 / (n - 1))))
    assert abs(r.mean() - pm) <= SIGMAS * np.sqrt(var / n)
    assert abs(r.var(ddof=1) - var) <= SIGMAS * var * np.sqrt(2.0 / (n - 1))
    assert np.all(obs[1:1 + S_].sum(0) == 1)
    counts = obs[1:1 + S_].sum(1)
    bound = SIGMAS * np.sqrt(n * (1.0 / S_) * (1.0 - 1.0 / S_))
    print("successor counts", counts, "want %.1f +- %.1f" % (n / S_, bound))
    assert np.all(np.abs(counts - n / S_) <= bound)
    assert np.array_equal(obs[2 + S_:2 + S_ + A].argmax(0), np.arange(n) % A) and np.array_equal(obs[S_ + A + 2], reward)


# ------------------------------------------------------------------------------------------------ 5. refusals, identities
def config(**kw):
    m = ra.meta_mdp_config_default()
    for k, v in kw.items():
        setattr(m, k, v)
    return m


BAD_CONFIGS = [
    dict(n_states=1), dict(n_states=11), dict(n_actions=1), dict(n_actions=9), dict(n_states=10, n_actions=7),
    dict(n_states=9, n_actions=8), dict(n_states=10, max_inner_steps=0), dict(max_inner_steps=1 << 32),
    dict(n_states=10, episodes_per_trial=0), dict(episodes_per_trial=1 << 32), dict(n_states=10, alpha=0.0),
    dict(alpha=float("nan")), dict(n_states=10, reward_prior_stddev=-0.5), dict(reward_stddev=float("inf")),
    dict(n_states=10, reward_prior_mean=float("nan")), dict(n_states=10, discount_factor=float("inf")),
]


@pytest.mark.parametrize("bad", BAD_CONFIGS, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_wide_constructor_refusals(engine, bad):
    code, text = code_of(lambda: ra.MetaMdpEnvWide(engine, 8, meta=config(**bad)))
    assert code == ra.ERR_BUILD_ENV and "rl_env_create_meta_mdp_wide" in text, text


def test_wide_constructor_checks_sizes_first_and_refuses_a_step_limit_and_null(engine):
    code, text = code_of(lambda: ra.MetaMdpEnvWide(engine, 8, meta=config(n_states=11, alpha=-1.0, max_inner_steps=0)))
    assert code == ra.ERR_BUILD_ENV and "n_states 2..10" in text and "at most 20" in text, text
    code, text = code_of(lambda: ra.MetaMdpEnvWide(engine, 8, 10, 5, limit=ra.LIMIT_LATENT, max_steps=10))
    assert code == ra.ERR_BUILD_ENV and "rl_env_create_meta_mdp_wide" in text and "step limit" in text
    assert code_of(lambda: ra.MetaMdpEnvWide(engine, 0, 10, 5))[0] == ra.ERR_BUILD_ENV
    cfg = ra.EnvConfig()
    cfg.kind, cfg.n_lanes, cfg.cartpole = ra.ENV_META_MDP, 8, ra.cartpole_params_default()
    h, meta = C.c_void_p(), config(n_states=10)
    lib = ra.lib()
    assert lib.rl_env_create_meta_mdp_wide(engine.h, C.byref(cfg), None, C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    assert lib.rl_env_create_meta_mdp_wide(engine.h, None, C.byref(meta), C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    assert lib.rl_env_create_meta_mdp_wide(engine.h, C.byref(cfg), C.byref(meta), None) == ra.ERR_INVALID_ARGUMENT


def test_the_older_entry_points_keep_their_answers(engine):
    code, text = code_of(lambda: ra.MetaMdpEnv(engine, 8, meta=config(n_states=10, n_actions=5)))
    assert code == ra.ERR_BUILD_ENV and "rl_env_create_meta_mdp:" in text and "at most 16" in text, text
    code, text = code_of(lambda: ra.RnnChainWide(engine, "gru", 17, 8, 5))
    assert code == ra.ERR_BUILD_AGENT and "rl_rnn_chain_create_wide:" in text and "in_dim 1..16" in text, text
    code, text = code_of(lambda: ra.Trajectory(engine, 8, 4, 17))
    assert code == ra.ERR_INVALID_ARGUMENT and "1..16" in text, text


def test_chain_and_trajectory_refusals(engine):
    for kw in (dict(in_dim=0), dict(in_dim=21), dict(out_dim=0), dict(out_dim=13), dict(hidden=0), dict(hidden=257)):
        a = dict(in_dim=19, hidden=8, out_dim=5)
        a.update(kw)
        code, text = code_of(lambda: ra.RnnChainWide20(engine, "gru", a["in_dim"], a["hidden"], a["out_dim"]))
        assert code == ra.ERR_BUILD_AGENT, (kw, text)
        if a["in_dim"] > 16:
            assert "rl_rnn_chain_create_wide20" in text and "in_dim 1..20" in text, text
    code, text = code_of(lambda: ra.RnnChainWide20(engine, "gru", 19, 8, 5, num_layers=5))
    assert code == ra.ERR_UNSUPPORTED
    for bad_d in (0, 21):
        code, text = code_of(lambda: ra.TrajectoryWide(engine, 8, 4, bad_d))
        assert code == ra.ERR_INVALID_ARGUMENT, text
    assert "rl_traj_create_wide" in code_of(lambda: ra.TrajectoryWide(engine, 8, 4, 21))[1]
    assert code_of(lambda: ra.TrajectoryWide(engine, 0, 4, 19))[0] == ra.ERR_INVALID_ARGUMENT
    # whatever reads a trajectory checks its own width against the planes'
    traj = ra.TrajectoryWide(engine, 8, 4, 20)
    pol = module(engine, R.Net("gru", 19, 8, 1, 0, True, 5), 1)
    env = make_env(engine, M.dist(10, 5, 2, 2), 8, 1)
    assert code_of(lambda: ra.rollout(env, pol, traj))[0] == ra.ERR_INVALID_ARGUMENT
    assert code_of(lambda: pol.seq_forward(traj))[0] == ra.ERR_INVALID_ARGUMENT


def test_entry_points_not_built_for_these_lanes_refuse_by_name(engine):
    env = make_env(engine, M.dist(10, 5, 2, 2), 8, 5)
    for fn, name in ((env.get_state, "rl_env_get_state"),
                     (lambda: env.set_state(np.zeros((4, 8)), np.zeros(8, np.int32), np.zeros(8, np.uint64),
                                            np.zeros(8, np.uint64)), "rl_env_set_state")):
        code, text = code_of(fn)
        assert code == ra.ERR_UNSUPPORTED and name in text and "RL_ENV_META_MDP" in text, text
    assert code_of(lambda: ra.Mlp(engine, env.D, [16], env.A))[0] == ra.ERR_BUILD_AGENT  # no feed-forward module of 19 inputs
    rec = module(engine, R.Net("gru", 19, 8, 1, 6, True, 5), 1)
    # (rl_dqn_create hears of more than two outputs, and of a module that does not match, before it hears of the env, on
    # every env: it gets the two-action lanes of 9 x 2 and their module)
    env2 = make_env(engine, M.dist(9, 2, 2, 2), 8, 5)
    rec2 = module(engine, R.Net("gru", 15, 8, 1, 6, True, 2), 1)
    lib, dq, out = ra.lib(), ra.dqn_config_default(), C.c_void_p()
    for name in ("rl_dqn_create", "rl_dqn_create_recurrent", "rl_dqn_create_finite"):
        e_, mod = (env2, rec2) if name == "rl_dqn_create" else (env, rec)
        opt = ra.Adam(mod)
        rc = getattr(lib, name)(e_.h, mod.h, opt.h, C.byref(dq), C.byref(out))
        text = lib.rl_last_error(engine.h).decode()
        assert rc == ra.ERR_UNSUPPORTED and name in text and "RL_ENV_META_MDP" in text, (name, rc, text)
    n = C.c_uint64()
    rc = lib.rl_actor_to_cbor(env.h, rec.h, C.c_int32(ra.ACTOR_POLICY), C.c_double(0.0), None, C.c_uint64(0), C.byref(n))
    text = lib.rl_last_error(engine.h).decode()
    assert rc == ra.ERR_UNSUPPORTED and "rl_actor_to_cbor" in text and "RL_ENV_META_MDP" in text, text
    assert env.step(np.zeros(8, np.uint8))[2].shape == (19, 8)  # the lanes still step after all of that


def test_new_entry_points_inside_the_older_ranges_build_the_older_handles(engine):
    d = M.dist(5, 5, 2, 2)
    old, new = make_env(engine, d, 70, 9, cls=ra.MetaMdpEnv), make_env(engine, d, 70, 9)
    assert (old.D, old.A) == (new.D, new.A) == (14, 5)
    assert old.observe().tobytes() == new.observe().tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(old.read_tables(), new.read_tables()))
    a = (np.arange(70) % 5).astype(np.uint8)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(old.step(a), new.step(a)))
    net = R.Net("lstm", 14, 9, 1, 6, True, 5)
    mo = ra.RnnChainWide(engine, net.cell, net.D, net.H, net.A, num_layers=1, bias=True, mlp_hidden=6)
    mn = module(engine, net)
    mo.init(7), mn.init(7)
    assert mo.P == mn.P and mo.get_params().tobytes() == mn.get_params().tobytes()
    code, text = code_of(lambda: ra.RnnChainWide20(engine, "gru", 14, 8, 13))  # the older refusal, word for word
    assert "rl_rnn_chain_create_wide:" in text
    to, tn = ra.Trajectory(engine, 70, 6, 14), ra.TrajectoryWide(engine, 70, 6, 14)
    ra.rollout(old, mo, to), ra.rollout(new, mn, tn)
    po, pn = to.read_all(), tn.read_all()
    assert all(po[k].tobytes() == pn[k].tobytes() for k in R.PLANES)
    assert "1..16" in code_of(lambda: ra.TrajectoryWide(engine, 8, 4, 0))[1]
