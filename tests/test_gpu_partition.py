"""The PartitionGame lanes on the device — rl_env_create_partition / ra.PartitionEnv (23 features, 24 under a visible
limit), rl_rnn_chain_create_wide24 / ra.RnnChainWide24 (up to 24 inputs) and rl_traj_create_wide24 / ra.TrajectoryWide24 (up
to 24 planes) — against the Python lanes of tests/partition_ref.py at the cases of tests/partition_cases.py (pinned on the
CPU by tests/test_partition_ref.py):

  driven steps   every case of the table — 64 and 200 lanes, VISIBLE 3, LATENT 3 and no limit, a lane offset — two horizons
                 of 7 steps with uploaded actions: rewards, successor codes, both observations and term_obs after every
                 step, bit for bit; elements that straddle a ChaCha block in every case; a reset in the middle of an episode
  f64            forward, gradient and Fisher-vector product (one output: the critic's gradient and loss) at 23 and 24
                 inputs against torch's f64 vectors
                 (tests/golden/torch_golden_seq_w24.json) and the stacked oracle, at the bars of
                 tests/test_gpu_meta_mdp_wide.py: forward bit-exact against the C oracle, 5e-6 and 2e-5 of max |g|
  updates        TRPO, PPO, REINFORCE and the critic step on a collected trajectory equal the same call on a host-written
                 copy of it
  statistics     rl_summary_push against NumPy on the records
  refusals       every refusal by code and name; inside the older ranges the new constructors build the older handles

The closed loop is tests/test_gpu_partition_rollout.py.  Every test here fails on a library without the entry points."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle as O
import partition_cases as W
import partition_ref as P
import relearn_amd as ra
import seq_multi_ref as R
from oracle import stacked as S
from steps_summary_ref import close, period_summaries
from test_gpu_stacked import GRAD_RTOL, rel_err
from test_seq_multi_ref import net_of

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torch_golden_seq_w24.json")) as f:
    GOLD = json.load(f)
GOLD_CASES = [k for k in GOLD if k != "generator"]


def make_env(engine, limit, n, seed, offset=0, seed_actor=1):
    return ra.PartitionEnv(engine, n, max_steps=limit.max_steps, limit=limit.kind, lane_offset=offset, seed_env=seed,
                           seed_actor=seed_actor)


def module(engine, net, seed=None):
    m = ra.RnnChainWide24(engine, net.cell, net.D, net.H, net.A, num_layers=net.L, bias=net.bias, mlp_hidden=net.H2 or None)
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
    ref = W.driven_reference(c)
    assert ref.straddles > 0  # elements whose ten words span two ChaCha blocks
    env = make_env(engine, c.limit, c.n, c.seed, offset=c.offset)
    assert (env.D, env.A) == (P.obs_dim(c.limit), 2)
    assert np.array_equal(env.observe(), ref.observe0)
    cuts = 0
    for t, (a, (reward_o, flag_o, obs_o, term_o)) in enumerate(zip(ref.actions, ref.steps)):
        reward, flag, obs, term = env.step(a)
        assert np.array_equal(reward, reward_o) and np.array_equal(flag, flag_o), t
        assert np.array_equal(obs, obs_o), t
        assert np.array_equal(env.observe(), obs_o), t  # ... and from the stored lane
        cut = flag == P.INTERRUPT
        assert np.array_equal(term[:, cut], term_o[:, cut]), t
        cuts += int(cut.all())
    assert cuts == (0 if c.limit.kind == P.LIMIT_NONE else W.DRIVEN_STEPS // c.limit.max_steps)
    with pytest.raises(ra.RelearnError):
        env.step(np.full(c.n, 2, np.uint8))  # an action index outside the two classifications


def test_reset_in_the_middle_of_an_episode_draws_where_the_stream_stands(engine):
    env, ref = make_env(engine, W.LATENT3, 200, 21), P.PartitionLanes(200, W.LATENT3, seed_env=21)
    rs = np.random.default_rng(4)
    for t in range(9):
        if t == 4:
            env.reset(), ref.reset()
            assert np.array_equal(env.observe(), ref.observe())
        a = rs.integers(0, 2, 200).astype(np.uint8)
        got, want = env.step(a), ref.step(a)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), t


# ------------------------------------------------------------------------------------------------ 2. f64 comparisons
def golden_traj(engine, c, net):
    D, n, T = net.D, c["n"], c["T"]
    h = {"obs": np.array(c["obs"], np.float32).reshape(D, T + 1, n),
         "term_obs": np.array(c["term_obs"], np.float32).reshape(D, T, n),
         "flag": np.array(c["flag"], np.uint8).reshape(T, n), "reward": np.zeros((T, n), np.float32),
         "action": np.array(c.get("action", [0] * (T * n)), np.uint8).reshape(T, n)}
    traj = ra.TrajectoryWide24(engine, n, T, D)
    traj.write_all(h)
    if "adv" in c:
        h["adv"] = np.array(c["adv"], np.float32).reshape(T, n)
        traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
    return traj, h


@pytest.mark.parametrize("name", GOLD_CASES)
def test_module_against_the_torch_vectors(engine, name):
    """the f32 parameters and planes nearest torch's f64 ones, two outputs and one: the forward is bit-exact against the
    C oracle on them and within 1e-5 of torch's outputs (tests/test_seq_w24_ref.py's bar for the f32 forward); gradient
    and Fisher-vector product against the f64 oracle on the same f32 data at GRAD_RTOL = 5e-6 and 2e-5.  Torch's own
    vectors were computed on the f64 data, half an f32 ulp away in every entry: the device is held to them at the same
    bars plus the distance between the two f64 results, which is the references' own and is printed.  One output: the
    same for rl_critic_gradient and its loss"""
    assert GRAD_RTOL == 5e-6
    c = GOLD[name]
    net = net_of(c)
    A, n, T = net.A, c["n"], c["T"]
    m = module(engine, net)
    p32 = np.array(c["params"], np.float32)
    m.set_params(p32)
    traj, h = golden_traj(engine, c, net)
    full = R.to_oracle(net, p32)
    out_d = m.seq_forward(traj, want_succ=False)[0]
    out_o = O.stack_seq_forward(R.shape_of(net), net.L, full, h, want_succ=False)[0]
    want_out = np.array(c["out"]).reshape(A, T, n)
    assert out_d.shape == (A, T, n) and np.array_equal(out_d, out_o)
    e_out = np.abs(out_d - want_out).max() / max(1.0, np.abs(want_out).max())
    print("%s: forward %.3g of torch's outputs (bar 1e-05)" % (name, e_out))
    assert e_out < 1e-5
    if A == 1:  # the critic: rl_critic_gradient of mean((V - target)^2), the targets in the return plane
        target = np.array(c["target"], np.float32).reshape(T, n)
        traj.write(ra.TRAJ_RETURNS, target)
        values, _, _ = S.forward(R.spec_of(net), full, h, want_succ=False)
        d = values[0] - target.astype(np.float64)
        g64 = R.restrict(net, S.backward(R.spec_of(net), full, h, (2.0 * d / (T * n))[None]))
        loss64 = (d * d).mean()
        g_d, loss_d = ra.critic_gradient(m, traj)
        e_g, t_g, r_g = rel_err(g_d, g64), rel_err(g_d, np.array(c["grad"])), rel_err(g64, np.array(c["grad"]))
        r_l = abs(loss64 - c["loss"]) / c["loss"]
        print("%s: critic gradient rel err %.3g (bar %.3g); against torch %.3g (the f64 oracle on the rounded data: %.3g); "
              "loss %.9g, f64 %.9g, torch %.9g" % (name, e_g, GRAD_RTOL, t_g, r_g, loss_d, loss64, c["loss"]))
        assert g_d.shape == g64.shape and e_g < GRAD_RTOL and t_g < GRAD_RTOL + r_g
        # (the loss at tests/test_gpu_stacked.py's bar, 1e-5 of it; torch's plus the references' own distance)
        assert abs(loss_d - loss64) <= 1e-5 * loss64 and abs(loss_d - c["loss"]) <= (1e-5 + r_l) * c["loss"]
        wih = g_d[:R.blocks(net)[0][2][0] * net.D].reshape(-1, net.D)
        assert np.all(np.abs(wih).max(0) > 0)
        return
    spec = R.spec_of(net)
    logits, _, _ = S.forward(spec, full, h, want_succ=False)
    dz, _, _ = R.surrogate_dlogits(logits, h["action"], h["adv"])
    g64 = R.restrict(net, S.backward(spec, full, h, dz))
    g_d, _, _ = ra.policy_gradient(m, traj)
    v = np.array(c["v"], np.float32)
    h64 = R.restrict(net, S.policy_fvp(spec, full, R.to_oracle(net, v, tangent=True), h, 0.0))
    h_d = ra.policy_fvp(m, traj, v, 0.0)
    e_g, e_h = rel_err(g_d, g64), rel_err(h_d, h64)
    t_g, t_h = rel_err(g_d, np.array(c["grad"])), rel_err(h_d, np.array(c["fvp"]))
    r_g, r_h = rel_err(g64, np.array(c["grad"])), rel_err(h64, np.array(c["fvp"]))  # f32-rounded data against f64 data
    print("%s: gradient rel err %.3g (bar %.3g), fvp rel err %.3g (bar 2e-05); against torch %.3g, %.3g (the f64 oracle "
          "on the rounded data: %.3g, %.3g)" % (name, e_g, GRAD_RTOL, e_h, t_g, t_h, r_g, r_h))
    assert e_g < GRAD_RTOL and e_h < 2e-5
    assert t_g < GRAD_RTOL + r_g and t_h < 2e-5 + r_h
    wih = g_d[:R.blocks(net)[0][2][0] * net.D].reshape(-1, net.D)
    assert np.all(np.abs(wih).max(0) > 0)  # every one of the 23 or 24 input columns carries gradient


NETS = [R.Net("gru", 24, 8, 1, 6, True, 2), R.Net("lstm", 24, 8, 1, 0, True, 2), R.Net("gru", 23, 33, 2, 0, False, 2),
        R.Net("lstm", 23, 8, 1, 6, True, 2)]
CRITIC = R.Net("gru", 24, 8, 1, 6, True, 1)  # the experiment's critic: 24 inputs, one output
T = 5


def written(engine, net, n, seed, T_=T):
    h = R.history(net, n, T_, seed)
    traj = ra.TrajectoryWide24(engine, n, T_, net.D)
    traj.write_all(h)
    traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
    traj.write(ra.TRAJ_RETURNS, h["rtg"])
    return traj, h


@pytest.mark.parametrize("net", NETS + [CRITIC], ids=R.net_id)
def test_initialisation_and_forward_are_bit_exact(engine, net):
    m = module(engine, net, 31)
    assert np.array_equal(m.get_params(), R.init(net, 31))
    traj, h = written(engine, net, 200, 5)
    out_d, succ_d = m.seq_forward(traj)
    out_o, succ_o = O.stack_seq_forward(R.shape_of(net), net.L, R.to_oracle(net, m.get_params()), h)
    assert out_d.shape == (net.A, T, 200)
    assert np.array_equal(out_d, out_o) and np.array_equal(succ_d, succ_o)
    # every input column above the older bound reaches the output: zeroing plane d changes it
    for dd in range(20, net.D):
        h2 = dict(h)
        h2["obs"] = h["obs"].copy()
        h2["obs"][dd] = 0.0
        traj.write_all(h2)
        assert not np.array_equal(m.seq_forward(traj)[0], out_d), dd


@pytest.mark.parametrize("net", NETS + [CRITIC], ids=R.net_id)
def test_gradient_and_fvp_against_f64(engine, net):
    """rl_policy_gradient and rl_policy_fvp on a host-written trajectory of 200 lanes at the bars
    tests/test_gpu_meta_mdp_wide.py uses: GRAD_RTOL = 5e-6 for the gradient, 2e-5 for the Fisher-vector product; for the
    critic rl_critic_gradient of mean((V - returns)^2) at GRAD_RTOL and the loss at 1e-5 of it, as
    tests/test_gpu_stacked.py holds it"""
    n = 200
    m = module(engine, net, 41)
    traj, h = written(engine, net, n, 6)
    spec, p = R.spec_of(net), m.get_params()
    full = R.to_oracle(net, p)
    if net.A == 1:
        values, _, _ = S.forward(spec, full, h, want_succ=False)
        d = values[0] - h["rtg"].astype(np.float64)
        g64 = R.restrict(net, S.backward(spec, full, h, (2.0 * d / d.size)[None]))
        g_d, loss_d = ra.critic_gradient(m, traj)
        e_g = rel_err(g_d, g64)
        print("%s: critic gradient rel err %.3g (bar %.3g)" % (R.net_id(net), e_g, GRAD_RTOL))
        assert g_d.shape == g64.shape and e_g < GRAD_RTOL, e_g
        assert abs(loss_d - (d * d).mean()) <= 1e-5 * (d * d).mean()
        wih = g_d[:R.blocks(net)[0][2][0] * net.D].reshape(-1, net.D)
        assert np.all(np.abs(wih).max(0) > 0)
        return
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
    wih = g_d[:R.blocks(net)[0][2][0] * net.D].reshape(-1, net.D)
    assert np.all(np.abs(wih).max(0) > 0)


# ------------------------------------------------------------------------------------------------ 3. whole updates
@pytest.mark.parametrize("update", ["trpo", "ppo", "reinforce", "critic"])
@pytest.mark.parametrize("limit", [W.VISIBLE3, W.LATENT3], ids=W.limit_id)
def test_updates_on_a_collected_trajectory_equal_the_written_one(engine, update, limit):
    n, T_ = 200, W.HORIZON
    D = P.obs_dim(limit)
    pnet, cnet = R.Net("gru", D, 12, 1, 6, True, 2), R.Net("gru", D, 8, 1, 6, True, 1)
    results, planes = [], None
    for source in ("rollout", "written"):
        env = make_env(engine, limit, n, 3, seed_actor=4)
        pol, cri = module(engine, pnet, 31), module(engine, cnet, 32)
        traj = ra.TrajectoryWide24(engine, n, T_, env.D)
        if source == "rollout":
            ra.rollout(env, pol, traj)
            planes = traj.read_all()
            assert sorted(np.unique(planes["action"])) == [0, 1]
            assert (planes["flag"] == P.INTERRUPT).sum() == 2 * n  # episodes of 3 steps in 7
        else:
            traj.write_all(planes)
        ra.gae(traj, cri, 0.999, 0.95)
        if update == "trpo":
            st = ra.trpo_update(pol, traj)
            assert st.status == ra.OPT_OK and st.loss_final < st.loss_initial
            extra = (st.as_dict(),)
        elif update == "critic":
            ccfg = ra.values_opt_config_default()
            ccfg.opt_steps_per_update = 3
            cst = ra.values_opt_update(cri, ra.Adam(cri), traj, ccfg)
            assert cst.loss_last < cst.loss_first
            extra = (cst.loss_first, cst.loss_last, cri.get_params().tobytes())
        elif update == "ppo":
            cfg = ra.ppo_config_default()
            cfg.opt_steps_per_update = 3
            _, losses = ra.ppo_update(pol, ra.Adam(pol), traj, cfg, want_losses=True)
            assert np.all(np.isfinite(losses))
            extra = (losses.tobytes(),)
        else:
            ra.reinforce_update(pol, ra.Adam(pol), traj)
            extra = ()
        if update != "critic":
            assert not np.array_equal(pol.get_params(), R.init(pnet, 31)) and np.all(np.isfinite(pol.get_params()))
        results.append((traj.read(ra.TRAJ_ADVANTAGES).tobytes(), pol.get_params().tobytes(), extra))
    assert results[0] == results[1]


# ------------------------------------------------------------------------------------------------ 4. statistics
def test_summary_push_against_numpy(engine):
    n, T_ = 200, W.HORIZON
    env = make_env(engine, W.VISIBLE3, n, 8, seed_actor=9)
    pol = module(engine, R.Net("gru", 24, 8, 1, 6, True, 2), 33)
    traj, s = ra.TrajectoryWide24(engine, n, T_, 24), ra.StepsSummary(engine, n)
    rewards, flags, got = [], [], []
    for _ in range(3):
        ra.rollout(env, pol, traj)
        rewards.append(traj.read(ra.TRAJ_REWARD)), flags.append(traj.read(ra.TRAJ_FLAG))
        s.push(traj)
        got.append(s.read())
        s.clear()
    want = period_summaries(rewards, flags)
    for g, w in zip(got, want):
        for f in ("step_reward", "episode_reward", "episode_length"):
            close(getattr(g, f), w[f], f)
    assert got[0].episode_length.count == 2 * n and got[0].episode_length.mean == 3.0
    assert set(np.unique(np.stack(rewards))) == {-1.0, 1.0}


# ------------------------------------------------------------------------------------------------ 5. refusals, identities
def test_constructor_refusals(engine):
    code, text = code_of(lambda: ra.PartitionEnv(engine, 8, max_steps=0, limit=ra.LIMIT_VISIBLE))
    assert code == ra.ERR_BUILD_ENV and "step limit" in text, text
    code, text = code_of(lambda: ra.PartitionEnv(engine, 8, max_steps=3, limit=7))
    assert code == ra.ERR_BUILD_ENV and "rl_env_create_partition" in text and "limit_kind" in text, text
    assert code_of(lambda: ra.PartitionEnv(engine, 0))[0] == ra.ERR_BUILD_ENV
    cfg = ra.EnvConfig()
    cfg.kind, cfg.n_lanes, cfg.cartpole = ra.ENV_PARTITION, 8, ra.cartpole_params_default()
    h, lib = C.c_void_p(), ra.lib()
    assert lib.rl_env_create_partition(engine.h, None, C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    assert lib.rl_env_create_partition(engine.h, C.byref(cfg), None) == ra.ERR_INVALID_ARGUMENT
    # the kind is the constructor's own: rl_env_create does not build it
    rc = lib.rl_env_create(engine.h, C.byref(cfg), C.byref(h))
    assert rc == ra.ERR_BUILD_ENV and "rl_env_create_partition" in lib.rl_last_error(engine.h).decode()
    env = ra.PartitionEnv(engine, 8, limit=ra.LIMIT_NONE, max_steps=0)
    assert (env.D, env.A) == (23, 2)
    env = ra.PartitionEnv(engine, 8)  # the experiment's: VisibleStepLimit::new(1000)
    assert (env.D, env.A) == (24, 2) and env.observe()[23].tolist() == [1.0] * 8


def test_the_older_entry_points_keep_their_answers(engine):
    code, text = code_of(lambda: ra.RnnChainWide20(engine, "gru", 21, 8, 2))
    assert code == ra.ERR_BUILD_AGENT and "rl_rnn_chain_create_wide20:" in text and "in_dim 1..20" in text, text
    code, text = code_of(lambda: ra.TrajectoryWide(engine, 8, 4, 21))
    assert code == ra.ERR_INVALID_ARGUMENT and "rl_traj_create_wide:" in text and "1..20" in text, text
    code, text = code_of(lambda: ra.Trajectory(engine, 8, 4, 17))
    assert code == ra.ERR_INVALID_ARGUMENT and "1..16" in text, text


def test_chain_and_trajectory_refusals(engine):
    for kw in (dict(in_dim=0), dict(in_dim=25), dict(out_dim=0), dict(out_dim=13), dict(hidden=0), dict(hidden=257)):
        a = dict(in_dim=24, hidden=8, out_dim=2)
        a.update(kw)
        code, text = code_of(lambda: ra.RnnChainWide24(engine, "gru", a["in_dim"], a["hidden"], a["out_dim"]))
        assert code == ra.ERR_BUILD_AGENT, (kw, text)
        if a["in_dim"] > 20:
            assert text.split(": ", 1)[-1].startswith("rl_rnn_chain_create_wide24: in_dim 1..24, ") or \
                "rl_rnn_chain_create_wide24: in_dim 1..24, " in text, text
    assert code_of(lambda: ra.RnnChainWide24(engine, "gru", 24, 8, 2, num_layers=5))[0] == ra.ERR_UNSUPPORTED
    for bad_d in (0, 25):
        assert code_of(lambda: ra.TrajectoryWide24(engine, 8, 4, bad_d))[0] == ra.ERR_INVALID_ARGUMENT
    assert "rl_traj_create_wide24" in code_of(lambda: ra.TrajectoryWide24(engine, 8, 4, 25))[1]
    assert code_of(lambda: ra.TrajectoryWide24(engine, 0, 4, 24))[0] == ra.ERR_INVALID_ARGUMENT
    # whatever reads a trajectory checks its own width against the planes'
    traj = ra.TrajectoryWide24(engine, 8, 4, 24)
    pol = module(engine, R.Net("gru", 23, 8, 1, 0, True, 2), 1)
    env = ra.PartitionEnv(engine, 8, limit=ra.LIMIT_NONE, max_steps=0)
    assert code_of(lambda: ra.rollout(env, pol, traj))[0] == ra.ERR_INVALID_ARGUMENT
    assert code_of(lambda: pol.seq_forward(traj))[0] == ra.ERR_INVALID_ARGUMENT


def test_entry_points_not_built_for_these_lanes_refuse_by_name(engine):
    env = ra.PartitionEnv(engine, 8, max_steps=3)
    for fn, name in ((env.get_state, "rl_env_get_state"),
                     (lambda: env.set_state(np.zeros((4, 8)), np.zeros(8, np.int32), np.zeros(8, np.uint64),
                                            np.zeros(8, np.uint64)), "rl_env_set_state")):
        code, text = code_of(fn)
        assert code == ra.ERR_UNSUPPORTED and name in text and "RL_ENV_PARTITION" in text, text
    assert code_of(lambda: ra.Mlp(engine, env.D, [16], env.A))[0] == ra.ERR_BUILD_AGENT  # no feed-forward module of 24 inputs
    # a feed-forward module, whatever its shape, is refused by name before a shape is compared
    ff, traj = ra.Mlp(engine, 5, 16, 2), ra.TrajectoryWide24(engine, 8, 4, env.D)
    code, text = code_of(lambda: ra.rollout(env, ff, traj))
    assert code == ra.ERR_UNSUPPORTED and "rl_rollout" in text and "RL_ENV_PARTITION" in text, text
    rec = module(engine, R.Net("gru", 24, 8, 1, 6, True, 2), 1)
    lib, dq, out = ra.lib(), ra.dqn_config_default(), C.c_void_p()
    for name in ("rl_dqn_create", "rl_dqn_create_recurrent", "rl_dqn_create_finite"):
        opt = ra.Adam(rec)
        rc = getattr(lib, name)(env.h, rec.h, opt.h, C.byref(dq), C.byref(out))
        text = lib.rl_last_error(engine.h).decode()
        assert rc == ra.ERR_UNSUPPORTED and name in text and "RL_ENV_PARTITION" in text, (name, rc, text)
    n = C.c_uint64()
    rc = lib.rl_actor_to_cbor(env.h, rec.h, C.c_int32(ra.ACTOR_POLICY), C.c_double(0.0), None, C.c_uint64(0), C.byref(n))
    text = lib.rl_last_error(engine.h).decode()
    assert rc == ra.ERR_UNSUPPORTED and "rl_actor_to_cbor" in text and "RL_ENV_PARTITION" in text, text
    code, text = code_of(lambda: ra.BanditAgent(env, "ucb1"))
    assert code == ra.ERR_UNSUPPORTED and "rl_bandit_agent" in text, text
    assert env.step(np.zeros(8, np.uint8))[2].shape == (24, 8)  # the lanes still step after all of that


def test_new_entry_points_inside_the_older_ranges_build_the_older_handles(engine):
    for D, A, older in ((19, 5, ra.RnnChainWide20), (14, 5, ra.RnnChainWide), (6, 2, ra.RnnChain)):
        net = R.Net("lstm", D, 9, 1, 6, True, A)
        mo = older(engine, net.cell, net.D, net.H, net.A, num_layers=1, bias=True, mlp_hidden=6)
        mn = module(engine, net)
        mo.init(7), mn.init(7)
        assert mo.P == mn.P and mo.get_params().tobytes() == mn.get_params().tobytes()
        h = R.history(net, 70, T, 5)
        older_traj = ra.TrajectoryWide if D > 16 else ra.Trajectory
        to, tn = older_traj(engine, 70, T, D), ra.TrajectoryWide24(engine, 70, T, D)
        to.write_all(h), tn.write_all(h)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(mo.seq_forward(to), mn.seq_forward(tn)))
    # the older refusals, word for word
    assert "rl_rnn_chain_create_wide20:" in code_of(lambda: ra.RnnChainWide24(engine, "gru", 19, 8, 13))[1]
    assert "rl_rnn_chain_create_wide:" in code_of(lambda: ra.RnnChainWide24(engine, "gru", 14, 8, 13))[1]
    assert "1..16" in code_of(lambda: ra.TrajectoryWide24(engine, 8, 4, 0))[1]
