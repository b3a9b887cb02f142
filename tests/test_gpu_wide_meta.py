"""The RL2 bandit experiment's pieces at 5 to 12 arms on the device — rl_env_create_meta_bandit_wide / ra.MetaBanditEnvWide
(k + 4 = 9..16 observation features) and rl_rnn_chain_create_wide / ra.RnnChainWide (up to 16 inputs and 12 outputs on the
lane-per-thread kernels, the head's outputs in up to three passes of four rows) — against the references that are
general in k, D and A (tests/meta_lanes_ref.py, tests/seq_multi_ref.py, tests/bandit_agents_ref.py,
tests/thompson_ref.py; pinned on the CPU by tests/test_seq_wide_ref.py): driven env steps bit for bit; initialisation and
forward bit for bit; gradient / Fisher-vector product / loss / KL / the clipped PPO gradient against f64 at the bars of
tests/test_gpu_seq_multi_action.py; closed-loop rollouts in one launch, per step and mixed; every update entry point;
the six baselines; identity with the older constructors inside their range; refusals; a trajectory shared with a
two-output module; and the RL2 model learning to use its memory on five arms.

Shapes (tests/wide_meta_cases.py says why): k in {5, 8, 9, 10, 12}; H in {7, 33}, mlp_hidden in {0, 6}; both cells; one
two-layer chain; one without recurrent bias vectors; n in {1, 70}; T = 5 (updates) and 13 (rollouts, 3 episodes per
trial).  Every test here fails on a library without the two entry points."""
import ctypes as C

import numpy as np
import pytest

import bandit_agents_ref as B
import meta_lanes_ref as M
import oracle as O
import relearn_amd as ra
import seq_multi_ref as R
import thompson_ref as TR
import wide_meta_cases as W
from oracle import stacked as S
from test_gpu_stacked import GRAD_RTOL, rel_err

pytestmark = pytest.mark.gpu
T = 5
ULP = 2.0 ** -24


def module(engine, net, seed=None):
    m = ra.RnnChainWide(engine, net.cell, net.D, net.H, net.A, num_layers=net.L, bias=net.bias, mlp_hidden=net.H2 or None)
    assert m.P == R.num_params(net)
    if seed is not None:
        m.init(seed)
    return m


def written(engine, net, n, seed, T_=T):
    h = R.history(net, n, T_, seed)
    traj = ra.Trajectory(engine, n, T_, net.D)
    traj.write_all(h)
    traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
    traj.write(ra.TRAJ_RETURNS, h["rtg"])
    return traj, h


def code_of(fn):
    with pytest.raises(ra.RelearnError) as e:
        fn()
    return e.value.code, str(e.value)


# ------------------------------------------------------------------------------------------------ 1. driven steps
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("k", [5, 9, 12])
@pytest.mark.parametrize("dist", [M.UNIFORM_BERNOULLI, M.ONE_HOT, M.ROUND_ROBIN])
def test_driven_steps_bit_for_bit(engine, dist, k, E):
    """50 lanes (ragged against workgroups of 64 and 256), 20 steps of random actions over all k arms, a reset() in the
    middle of a trial; lanes 25..49 equal a 25-lane env at lane_offset 25.  At k >= 8 a trial's means fill a ChaCha block
    or more, so the means of one trial lie in two or three blocks"""
    n, steps, seed = 50, 20, 11 + k
    env = ra.MetaBanditEnvWide(engine, n, k, E, dist, seed_env=seed)
    tail = ra.MetaBanditEnvWide(engine, n - 25, k, E, dist, lane_offset=25, seed_env=seed)
    assert (env.D, env.A) == (k + 4, k)
    ref = M.MetaLanes(n, k, E, dist, seed_env=seed)
    rs = np.random.default_rng(100 * k + E)
    assert np.array_equal(env.observe(), ref.observe()) and np.array_equal(tail.observe(), ref.observe()[:, 25:])
    rewards, flags, actions = [], [], []
    for t in range(steps):
        if t == 8:  # 8 mod (2 E - 1) = 3 at E = 3: inside a trial; the new trial draws where the stream stands
            env.reset(), tail.reset(), ref.reset()
            assert np.array_equal(env.observe(), ref.observe())
        a = rs.integers(0, k, n).astype(np.uint8)
        reward, flag, obs, term = env.step(a)
        reward_o, flag_o, obs_o, term_o = ref.step(a)
        assert np.array_equal(reward, reward_o) and np.array_equal(flag, flag_o), t
        assert np.array_equal(obs, obs_o), t
        # ... and from the stored lane (the step's own observation comes from registers; this one from the lane's byte,
        # whose action field must hold 0..k-1)
        assert np.array_equal(env.observe(), obs_o), t
        cut = flag == M.INTERRUPT
        assert np.array_equal(term[:, cut], term_o[:, cut]), t
        reward_t, flag_t, obs_t, term_t = tail.step(a[25:])
        assert np.array_equal(reward_t, reward[25:]) and np.array_equal(flag_t, flag[25:]), t
        assert np.array_equal(obs_t, obs[:, 25:]) and np.array_equal(term_t[:, cut[25:]], term[:, 25:][:, cut[25:]]), t
        rewards.append(reward), flags.append(flag), actions.append(a)
    rewards, flags = np.array(rewards), np.array(flags)
    assert set(np.unique(rewards)) == {0.0, 1.0} and sorted(np.unique(actions)) == list(range(k))
    assert set(np.unique(flags)) == ({M.INTERRUPT} if E == 1 else {M.CONTINUE, M.INTERRUPT})
    with pytest.raises(ra.RelearnError):
        env.step(np.full(n, k, np.uint8))  # an action index outside IndexSpace::new(k)


# ------------------------------------------------------------------------------------------------ 2. init, forward
@pytest.mark.parametrize("net", W.NETS + W.CRITICS, ids=R.net_id)
def test_initialisation_draws_every_tensor_at_its_real_width(engine, net):
    m = module(engine, net, 31)
    assert np.array_equal(m.get_params(), R.init(net, 31))
    none_if = lambda x: x if net.bias else None
    m.init_with(33, O.RNN_DEFAULT_INITS[0], O.RNN_DEFAULT_INITS[1], none_if(R.BIAS_INIT), *O.RNN_DEFAULT_INITS[3:])
    inits = list(O.RNN_DEFAULT_INITS)
    if net.bias:
        inits[2] = R.BIAS_INIT
    assert np.array_equal(m.get_params(), R.init(net, 33, tuple(inits)))
    q = np.random.default_rng(2).normal(size=m.P).astype(np.float32)
    m.set_params(q)
    assert np.array_equal(m.get_params(), q)


@pytest.mark.parametrize("net", W.NETS + W.CRITICS, ids=R.net_id)
@pytest.mark.parametrize("n", [1, 70])
def test_forward_is_bit_exact(engine, net, n):
    """module outputs and successor outputs (Interrupt and horizon cuts) against the C restatement: identical bits"""
    m = module(engine, net, 31)
    traj, h = written(engine, net, n, 5)
    out_d, succ_d = m.seq_forward(traj)
    out_o, succ_o = O.stack_seq_forward(R.shape_of(net), net.L, R.to_oracle(net, m.get_params()), h)
    assert out_d.shape == (net.A, T, n)
    assert np.array_equal(out_d, out_o) and np.array_equal(succ_d, succ_o)
    assert np.abs(out_o).min() > 0 and np.count_nonzero(succ_o[net.A - 1]) > 0
    for q in range(1, net.A):  # no output row repeats another (a pass that read the rows of the pass before it would)
        assert not np.array_equal(out_d[q], out_d[q - 1])


# ------------------------------------------------------------------------------------------------ 3. f64 comparisons
@pytest.mark.parametrize("net", W.NETS, ids=R.net_id)
@pytest.mark.parametrize("n", [1, 70])
def test_gradient_fvp_loss_and_kl_against_f64(engine, net, n):
    """rl_policy_gradient, rl_policy_fvp and rl_policy_loss_kl on a host-written trajectory whose action plane uses every
    index, at the bars tests/test_gpu_seq_multi_action.py uses for the same quantities: GRAD_RTOL for the gradient, 2e-5
    for the Fisher-vector product, 2e-5 / 2e-4 (+ the f32 floor of a log-probability difference) for loss and KL"""
    m = module(engine, net, 41)
    traj, h = written(engine, net, n, 6)
    if n >= net.A:
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
    print("%s n=%d: gradient rel err %.3g (bar %.3g), fvp rel err %.3g (bar 2e-05)" % (R.net_id(net), n, e_g, GRAD_RTOL, e_h))
    assert g_d.shape == g64.shape and e_g < GRAD_RTOL, e_g
    assert e_h < 2e-5, e_h
    assert abs(loss_d - loss64) <= 2e-5 * abs(loss64) + 1e-7 and abs(ent_d - ent64) <= 2e-5 * abs(ent64) + 1e-7
    for name, l, shp, o, _ in R.blocks(net):  # every block receives gradient, the head's rows of every output included
        s = slice(o, o + int(np.prod(shp)))
        assert np.abs(g_d[s]).max() > 0, (name, l)
        assert rel_err(g_d[s], g64[s]) < 100 * GRAD_RTOL, (name, l, rel_err(g_d[s], g64[s]))
    A = net.A
    head_bias = g_d[-A:]
    assert np.all(head_bias != 0) and np.abs(head_bias - g64[-A:]).max() <= 100 * GRAD_RTOL * np.abs(g64[-A:]).max()
    moved = (p + 0.01 * v).astype(np.float32)
    m.set_params(moved)
    loss1, kl1 = ra.policy_loss_kl(m, traj, p)
    z1, _, _ = S.forward(spec, R.to_oracle(net, moved), h, want_succ=False)
    l64, k64 = R.loss_and_kl(z1, logits, h["action"], h["adv"])
    print("%s n=%d: loss %.8g (f64 %.8g), KL %.6g (f64 %.6g)" % (R.net_id(net), n, loss1, l64, kl1, k64))
    assert abs(loss1 - l64) <= 2e-5 * abs(l64) + 1e-7
    kl_floor = 4 * ULP * np.abs(R.log_softmax(logits)).max(0).mean()
    assert abs(kl1 - k64) <= 2e-4 * abs(k64) + kl_floor
    m.set_params(p)
    assert ra.policy_loss_kl(m, traj, p)[1] == 0.0


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


@pytest.mark.parametrize("net,lr", W.PPO_CASES, ids=[R.net_id(c[0]) for c in W.PPO_CASES])
def test_clipped_ppo_gradient_off_ratio_one(engine, net, lr):
    """tests/test_gpu_seq_multi_action.py's method and bar at nine and twelve outputs: under plain SGD from p0, one
    rl_ppo_update step gives p1 and two give p2; (p1 - p2) / lr is the clipped gradient AT p1, against the f64
    restatement at clip distances 0.2 and 0; the bar is GRAD_RTOL of max |g| plus the readback term of element j"""
    m = module(engine, net, W.PPO_INIT_SEED)
    traj, h = written(engine, net, W.PPO_N, W.PPO_HISTORY_SEED, W.PPO_T)
    spec, p0 = R.spec_of(net), m.get_params()
    z0, _, _ = S.forward(spec, R.to_oracle(net, p0), h, want_succ=False)
    for clip in (0.2, 0.0):
        p1, _ = sgd_steps(m, traj, p0, lr, 1, clip)
        again, _ = sgd_steps(m, traj, p0, lr, 1, clip)
        p2, losses = sgd_steps(m, traj, p0, lr, 2, clip)
        assert np.array_equal(p1, again) and not np.array_equal(p1, p0) and np.all(np.isfinite(p2))
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


# ------------------------------------------------------------------------------------------------ 4. rollouts
def meta_run(engine, case, variants):
    net = case.net
    try:
        env = ra.MetaBanditEnvWide(engine, case.n, net.A, case.E, case.arms, lane_offset=case.offset,
                                   seed_env=case.seed + 1, seed_actor=case.seed + 2)
        assert (env.D, env.A) == (net.D, net.A)
        pol = module(engine, net)
        if net.bias:
            pol.init_with(case.seed, bias=R.BIAS_INIT)
        else:
            pol.init(case.seed)
        assert np.array_equal(pol.get_params(), R.meta_case_params(case))
        traj = ra.Trajectory(engine, case.n, case.T, net.D)
        planes = []
        for variant in variants:
            engine.set_kernel_variant(variant)
            ra.rollout(env, pol, traj)
            planes.append(traj.read_all())
        engine.set_kernel_variant(0)
        logits = pol.seq_forward(traj, want_succ=False)[0]
        observe = env.observe()
    finally:
        engine.set_kernel_variant(0)
    return planes, logits, observe


@pytest.mark.parametrize("case", W.META_CASES, ids=R.meta_case_id)
def test_rollout_on_wide_meta_bandit_lanes(engine, case):
    """5, 9, 10 and 12 arms: all steps in one launch (kernel variant 0), the launch sequence per step (variant 1), and one
    then the other, against the closed-loop reference — whole planes, obs[T] and term_obs included, two collections in a
    row, no sample excused (tests/test_seq_wide_ref.py holds every margin above 1e-5)"""
    ref = R.meta_reference(case)
    net = case.net
    z = O.stack_seq_forward(R.shape_of(net), net.L, R.to_oracle(net, R.meta_case_params(case)), ref.periods[-1],
                            want_succ=False)[0]
    runs = {}
    for what, variants in (("one launch", (0, 0)), ("per step", (1, 1)), ("one launch, then per step", (0, 1))):
        planes, logits, observe = runs[what] = meta_run(engine, case, variants)
        for p in range(R.PERIODS):
            for key in ("action", "reward", "flag", "obs"):
                assert np.array_equal(planes[p][key], ref.periods[p][key]), (what, p, key)
            cut = ref.periods[p]["flag"] == M.INTERRUPT
            assert cut.any() and np.array_equal(planes[p]["term_obs"][:, cut], ref.periods[p]["term_obs"][:, cut]), (what, p)
        assert np.array_equal(logits, z), what
        assert np.array_equal(observe, ref.observe), what
    for p in range(R.PERIODS):  # the two against each other: every term_obs entry included
        for key in R.PLANES:
            assert np.array_equal(runs["one launch"][0][p][key], runs["per step"][0][p][key]), (p, key)
    if case.n >= 70:
        assert sorted(np.unique(np.concatenate([q["action"] for q in runs["one launch"][0]]))) == list(range(net.A))


# ------------------------------------------------------------------------------------------------ 5. whole updates
@pytest.mark.parametrize("update", ["trpo", "ppo", "reinforce", "actor_critic", "actor_critic_begin_finish"])
def test_updates_on_a_collected_trajectory_equal_the_written_one(engine, update):
    """every update entry point on a trajectory collected on ten-arm lanes — policy 14 -> 10, critic 14 -> 1, both
    Chain<Gru, Linear>, the experiment's model — equals the same call on the same planes written by the host"""
    n, T_, E, k = 70, 10, 3, 10
    pnet, cnet = R.Net("gru", 14, 12, 1, 0, True, 10), R.Net("gru", 14, 8, 1, 0, True, 1)
    results, planes = [], None
    for source in ("rollout", "written"):
        env = ra.MetaBanditEnvWide(engine, n, k, E, "one_hot", seed_env=3, seed_actor=4)
        pol, cri = module(engine, pnet, 31), module(engine, cnet, 32)
        traj = ra.Trajectory(engine, n, T_, env.D)
        if source == "rollout":
            ra.rollout(env, pol, traj)
            planes = traj.read_all()
            assert sorted(np.unique(planes["action"])) == list(range(k))
        else:
            traj.write_all(planes)
        ra.gae(traj, cri, 0.99, 0.3)
        ccfg = ra.values_opt_config_default()
        ccfg.opt_steps_per_update = 3
        extra = ()
        if update == "trpo":
            st = ra.trpo_update(pol, traj)
            assert st.status == ra.OPT_OK and st.loss_final < st.loss_initial and st.constraint_val_final <= 0.01
            extra = (st.as_dict(),)
        elif update == "ppo":
            cfg = ra.ppo_config_default()
            cfg.opt_steps_per_update = 3
            _, losses = ra.ppo_update(pol, ra.Adam(pol), traj, cfg, want_losses=True)
            assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]
            extra = (losses.tobytes(),)
        elif update == "reinforce":
            st = ra.reinforce_update(pol, ra.Adam(pol), traj)
            assert np.isfinite(st.loss_first) and np.isfinite(st.entropy) and st.entropy > 0
            extra = (st.loss_first, st.entropy)
        elif update == "actor_critic":
            pst, cst, losses = ra.actor_critic_update(pol, cri, ra.Adam(cri), traj, None, ccfg, want_losses=True)
            assert pst.status == ra.OPT_OK and losses[-1] < losses[0]
            extra = (pst.as_dict(), losses.tobytes())
        else:
            pst = ra.actor_critic_update_begin(pol, cri, ra.Adam(cri), traj, None, ccfg)
            cst, losses = ra.actor_critic_update_finish(traj, want_losses=True)
            assert pst.status == ra.OPT_OK and losses[-1] < losses[0]
            extra = (pst.as_dict(), losses.tobytes())
        assert not np.array_equal(pol.get_params(), R.init(pnet, 31)) and np.all(np.isfinite(pol.get_params()))
        results.append((traj.read(ra.TRAJ_ADVANTAGES), pol.get_params(), cri.get_params(), extra))
    a, b = results
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert np.abs(a[0]).max() > 0


# ------------------------------------------------------------------------------------------------ 6. baselines
def same_planes(got, want, where):
    for key in ("obs", "action", "reward", "flag"):
        assert np.array_equal(got[key], want[key]), (where, key)
    cut = got["flag"] == M.INTERRUPT
    assert np.array_equal(got["term_obs"][:, cut], want["term_obs"][:, cut]), (where, "term_obs")


# the experiment's six: (name, kind, exploration_rate, initial_action_count, initial_action_value, num_samples)
BASELINES = [("random", B.RANDOM, None, None, None, None), ("greedy", B.TABULAR_Q, 0.0, 2, 0.5, None),
             ("eps_greedy", B.TABULAR_Q, 0.2, 2, 0.5, None), ("ucb1", B.UCB1, None, None, None, None),
             ("ts", "thompson", None, None, None, 1), ("ots", "thompson", None, None, None, 10)]


@pytest.mark.parametrize("k", [5, 12])
@pytest.mark.parametrize("spec", BASELINES, ids=[b[0] for b in BASELINES])
def test_baselines_bit_for_bit(engine, spec, k):
    """all six kinds, as tests/test_gpu_bandit_agents.py and tests/test_gpu_thompson_agents.py hold them at 2..4 arms:
    45 lanes, 3 episodes per trial, T = 7 against trials of 5 steps, two collections on one env and one agent; after
    each, every plane, the agent's state and actor word position; afterwards the env's observation and a driven step"""
    _, kind, rate, count, value, num_samples = spec
    n, E, T_, seed, dist = 45, 3, 7, 3 + k, M.UNIFORM_BERNOULLI
    env = ra.MetaBanditEnvWide(engine, n, k, E, dist, seed_env=seed, seed_actor=seed + 1)
    traj = ra.Trajectory(engine, n, T_, env.D)
    ref_env = M.MetaLanes(n, k, E, dist, seed_env=seed)
    if num_samples is None:
        agent = ra.BanditAgent(env, kind, rate, count, value)
        ref = B.BanditAgentLanes(n, k, kind, rate, count, value, seed_actor=seed + 1)
    else:
        agent = ra.BanditAgent(env, kind, num_samples=num_samples)
        ref = TR.ThompsonAgentLanes(n, k, num_samples, seed_actor=seed + 1)

    def same_state(where):
        got, want = agent.state(), ref.state()
        assert set(got) - {"ln_table"} == set(want), where
        for key in want:
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (where, key)
        if "ln_table" in got:
            assert np.array_equal(got["ln_table"], B.ln_table(k, E)), where

    same_state("created")
    planes = []
    for period in range(2):
        agent.rollout(env, traj)
        got = traj.read_all()
        same_planes(got, ref.rollout(ref_env, T_), period)
        same_state(period)
        planes.append(got)
    assert np.array_equal(env.observe(), ref_env.observe())
    a = (np.arange(n) % k).astype(np.uint8)
    reward, flag, obs, term = env.step(a)
    reward_o, flag_o, obs_o, term_o = ref_env.step(a)
    assert np.array_equal(reward, reward_o) and np.array_equal(flag, flag_o) and np.array_equal(obs, obs_o)
    assert np.array_equal(term[:, flag == M.INTERRUPT], term_o[:, flag_o == M.INTERRUPT])
    flags = np.concatenate([p["flag"] for p in planes])
    assert np.array_equal(np.nonzero((flags == M.INTERRUPT).all(axis=1))[0], [4, 9])
    actions = np.concatenate([p["action"] for p in planes])
    pulls = np.concatenate([p["obs"][0, :-1] for p in planes]) == 0.0
    assert np.all(actions[~pulls] == 0)
    if kind == B.UCB1:
        assert np.all(actions[[0, 5, 10]] == k - 1)  # the first pull of every trial: the LAST maximal index
    elif spec[0] == "greedy":
        assert np.all(actions[[0, 5, 10]] == 0)      # ... and the FIRST
    else:
        assert actions[pulls].max() == k - 1 and actions[pulls].min() == 0


# ------------------------------------------------------------------------------------------------ 7. identity, refusals
@pytest.mark.parametrize("k", [2, 4])
def test_wide_env_constructor_inside_the_old_range_is_the_old_one(engine, k):
    n, E = 50, 3
    old = ra.MetaBanditEnv(engine, n, k, E, seed_env=5, seed_actor=6)
    new = ra.MetaBanditEnvWide(engine, n, k, E, seed_env=5, seed_actor=6)
    assert (old.D, old.A) == (new.D, new.A) == (k + 4, k)
    rs = np.random.default_rng(k)
    assert np.array_equal(old.observe(), new.observe())
    for t in range(12):
        a = rs.integers(0, k, n).astype(np.uint8)
        for x, y in zip(old.step(a), new.step(a)):
            assert np.array_equal(x, y), t
    pol = ra.RnnChainWide(engine, "gru", k + 4, 9, k)
    pol.init(3)
    t_old, t_new = ra.Trajectory(engine, n, 7, k + 4), ra.Trajectory(engine, n, 7, k + 4)
    ra.rollout(old, pol, t_old)
    ra.rollout(new, pol, t_new)
    a, b = t_old.read_all(), t_new.read_all()
    for key in R.PLANES:
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("net", [R.Net("gru", 5, 128, 1, 128, True, 2), R.Net("lstm", 8, 9, 2, 0, False, 8),
                                 R.Net("gru", 7, 7, 1, 6, True, 3)], ids=R.net_id)
def test_wide_chain_constructor_inside_the_old_range_is_the_old_one(engine, net):
    """in_dim <= 8 and out_dim <= 8: the same parameters, forward and gradient bytes (the fused tile kernels' 5 -> 128 ->
    128 -> 2 shape included)"""
    n = 64
    args = (engine, net.cell, net.D, net.H, net.A)
    kw = dict(num_layers=net.L, bias=net.bias, mlp_hidden=net.H2 or None)
    old, new = ra.RnnChain(*args, **kw), ra.RnnChainWide(*args, **kw)
    old.init(7)
    new.init(7)
    assert old.P == new.P and np.array_equal(old.get_params(), new.get_params())
    h = R.history(net, n, T, 9)
    traj = ra.Trajectory(engine, n, T, net.D)
    traj.write_all(h)
    traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
    for x, y in zip(old.seq_forward(traj), new.seq_forward(traj)):
        assert np.array_equal(x, y)
    g_old, g_new = ra.policy_gradient(old, traj), ra.policy_gradient(new, traj)
    assert np.array_equal(g_old[0], g_new[0]) and g_old[1:] == g_new[1:] and np.abs(g_old[0]).max() > 0


def test_refusals(engine):
    n = 8
    # arms
    for bad in (dict(n_arms=0), dict(n_arms=1), dict(n_arms=13), dict(n_arms=10, episodes_per_trial=0),
                dict(n_arms=10, distribution=7), dict(n_arms=10, limit=ra.LIMIT_LATENT, max_steps=5)):
        assert code_of(lambda: ra.MetaBanditEnvWide(engine, n, **bad))[0] == ra.ERR_BUILD_ENV, bad
    assert code_of(lambda: ra.MetaBanditEnv(engine, n, n_arms=5))[0] == ra.ERR_BUILD_ENV  # the older one keeps its answer
    cfg = ra.EnvConfig()
    cfg.kind, cfg.n_lanes, cfg.cartpole = ra.ENV_META_BANDIT, n, ra.cartpole_params_default()
    h = C.c_void_p()
    assert ra.lib().rl_env_create_meta_bandit_wide(engine.h, C.byref(cfg), None, C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    for k in range(2, 13):
        env = ra.MetaBanditEnvWide(engine, n, k, 2, "one_hot")
        assert (env.D, env.A) == (k + 4, k)
        env.close()

    # outputs and inputs
    def create(**kw):
        c = ra.rnn_chain_config_default("gru")
        c.hidden, c.mlp_hidden = 8, 0
        for key, v in kw.items():
            setattr(c, key, v)
        return ra.lib().rl_rnn_chain_create_wide(engine.h, C.byref(c), C.byref(h))

    for kw in (dict(out_dim=0), dict(out_dim=13), dict(in_dim=14, out_dim=0), dict(in_dim=14, out_dim=13), dict(in_dim=0),
               dict(in_dim=17), dict(in_dim=0, out_dim=12), dict(in_dim=17, out_dim=12), dict(in_dim=14, hidden=0),
               dict(in_dim=14, hidden=257), dict(in_dim=14, mlp_hidden=257), dict(in_dim=14, rnn_bias=2),
               dict(in_dim=14, cell=2), dict(in_dim=14, num_layers=0)):
        assert create(**kw) == ra.ERR_BUILD_AGENT, kw
        assert not h.value
    assert create(in_dim=14, num_layers=5) == ra.ERR_UNSUPPORTED
    assert ra.lib().rl_rnn_chain_create_wide(engine.h, None, C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    c = ra.rnn_chain_config_default("gru")
    c.in_dim = 14
    assert ra.lib().rl_rnn_chain_create_wide(engine.h, C.byref(c), None) == ra.ERR_INVALID_ARGUMENT
    for kw in (dict(in_dim=16, out_dim=12, hidden=256, num_layers=4, mlp_hidden=256, cell=1), dict(in_dim=9, out_dim=1, hidden=1),
               dict(in_dim=1, out_dim=9, hidden=1)):
        assert create(**kw) == ra.OK  # the corners of the range build
        assert ra.lib().rl_mlp_destroy(h) == ra.OK
    # the older constructor keeps its answers
    old = ra.rnn_chain_config_default("gru")
    old.out_dim = 9
    assert ra.lib().rl_rnn_chain_create(engine.h, C.byref(old), C.byref(h)) == ra.ERR_BUILD_AGENT
    old.out_dim, old.in_dim = 2, 9
    assert ra.lib().rl_rnn_chain_create(engine.h, C.byref(old), C.byref(h)) == ra.ERR_BUILD_AGENT

    # what stays refused on a ten-arm env, by name
    env = ra.MetaBanditEnvWide(engine, n, 10, 2)
    code, msg = code_of(lambda: ra.Mlp(engine, env.D, [16], 10))  # feed-forward modules have at most eight inputs
    assert code == ra.ERR_BUILD_AGENT and "in_dim 1..8" in msg
    pol = ra.RnnChainWide(engine, "gru", env.D, 8, 10)
    pol.init(1)
    dcfg = ra.dqn_config_default()
    dcfg.buffer_capacity, dcfg.minibatch_steps = 64, 32
    code, msg = code_of(lambda: ra.FiniteDqn(env, pol, ra.Adam(pol), dcfg))
    assert code == ra.ERR_UNSUPPORTED and "rl_dqn_create_finite" in msg
    code, msg = code_of(lambda: ra.RecurrentDqn(env, pol, ra.Adam(pol), dcfg))
    assert code == ra.ERR_UNSUPPORTED and "rl_dqn_create_recurrent" in msg
    assert code_of(lambda: ra.Dqn(env, pol, ra.Adam(pol), dcfg))[0] == ra.ERR_UNSUPPORTED
    code, msg = code_of(lambda: ra.actor_to_cbor(env, pol))
    assert code == ra.ERR_UNSUPPORTED and "rl_actor_to_cbor" in msg
    code, msg = code_of(env.get_state)
    assert code == ra.ERR_UNSUPPORTED and "rl_env_get_state" in msg
    code, msg = code_of(lambda: env.set_state(np.zeros((4, n)), np.zeros(n), np.zeros(n), np.zeros(n)))
    assert code == ra.ERR_UNSUPPORTED and "rl_env_set_state" in msg
    # shapes against envs: one output per arm, the env's features
    nine = ra.RnnChainWide(engine, "gru", env.D, 8, 9)
    nine.init(1)
    assert code_of(lambda: ra.rollout(env, nine, ra.Trajectory(engine, n, 4, env.D)))[0] == ra.ERR_INVALID_ARGUMENT
    assert code_of(lambda: ra.rollout(env, pol, ra.Trajectory(engine, n, 4, 13)))[0] == ra.ERR_INVALID_ARGUMENT
    # a trajectory collected on ten arms does not update a policy of twelve outputs
    t10 = ra.Trajectory(engine, n, 4, env.D)
    ra.rollout(env, pol, t10)
    twelve = ra.RnnChainWide(engine, "gru", env.D, 8, 12)
    twelve.init(1)
    assert code_of(lambda: ra.policy_gradient(twelve, t10))[0] == ra.ERR_INVALID_ARGUMENT
    assert code_of(lambda: ra.Trajectory(engine, n, 4, 17))[0] == ra.ERR_INVALID_ARGUMENT


def test_a_trajectory_serves_twelve_and_two_outputs_in_turn(engine):
    """lp0, dz and the output planes grow to twelve planes where the twelve-output module first meets the trajectory; the
    two-output module's results before and after equal those on a fresh trajectory, bit for bit"""
    n = 70
    net2, net12 = R.Net("gru", 16, 9, 2, 6, True, 2), R.Net("lstm", 16, 7, 1, 0, True, 12)
    h2 = R.history(net2, n, T, 11)
    h12 = dict(h2, action=R.history(net12, n, T, 11)["action"])

    def fill(traj, h):
        traj.write_all(h)
        traj.write(ra.TRAJ_ADVANTAGES, h["adv"])

    def two_output_results(traj, m2):
        fill(traj, h2)
        v = np.random.default_rng(4).normal(size=m2.P).astype(np.float32)
        p = m2.get_params()
        out = (m2.seq_forward(traj), ra.policy_gradient(m2, traj), ra.policy_fvp(m2, traj, v, 1e-5),
               ra.policy_loss_kl(m2, traj, (p + 0.01 * v).astype(np.float32)))
        st = ra.trpo_update(m2, traj)
        res = out + (m2.get_params(), st.as_dict())
        m2.set_params(p)
        return res

    def same(a, b):
        if isinstance(a, (tuple, list)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if isinstance(a, np.ndarray):
            return np.array_equal(a, b)
        return a == b

    m2, m12 = module(engine, net2, 21), module(engine, net12, 22)
    fresh = two_output_results(ra.Trajectory(engine, n, T, 16), m2)
    shared = ra.Trajectory(engine, n, T, 16)
    fill(shared, h12)
    spec12, full12 = R.spec_of(net12), R.to_oracle(net12, m12.get_params())
    z12, _, _ = S.forward(spec12, full12, h12, want_succ=False)
    g64 = R.restrict(net12, S.backward(spec12, full12, h12, R.surrogate_dlogits(z12, h12["action"], h12["adv"])[0]))
    g12 = ra.policy_gradient(m12, shared)[0]
    assert rel_err(g12, g64) < GRAD_RTOL
    out12, _ = m12.seq_forward(shared)
    assert np.array_equal(out12, O.stack_seq_forward(R.shape_of(net12), 1, full12, h12)[0])
    ra.trpo_update(m12, shared)  # (a whole update: CG vectors, line search, the P-sized workspace)
    assert np.all(np.isfinite(m12.get_params()))
    after = two_output_results(shared, m2)
    assert same(fresh, after)
    fill(shared, h12)
    m12.set_params(R.restrict(net12, full12))
    assert np.array_equal(ra.policy_gradient(m12, shared)[0], g12)


# ------------------------------------------------------------------------------------------------ 8. learning
LEARNING = dict(arms=5, lanes=1024, episodes_per_trial=10, trials_per_period=2, hidden=32, seed=40)
PERIODS = 30  # twice the smallest count that clears the bar with three seeds (profiles/wide_meta_learning.json)


def learn(engine, n, E, trials, H, periods, seed, arms, curve=None):
    T_ = trials * (2 * E - 1)
    env = ra.MetaBanditEnvWide(engine, n, arms, E, "one_hot", seed_env=seed, seed_actor=seed + 1)
    pol = ra.RnnChainWide(engine, "gru", env.D, H, arms)
    cri = ra.RnnChainWide(engine, "gru", env.D, H, 1)
    pol.init(seed + 2)
    cri.init(seed + 3)
    opt = ra.Adam(cri)
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = 10
    traj = ra.Trajectory(engine, n, T_, env.D)

    def evaluate():
        ev_env = ra.MetaBanditEnvWide(engine, 4096, arms, E, "one_hot", seed_env=seed + 10, seed_actor=seed + 11)
        ev_traj = ra.Trajectory(engine, 4096, 2 * E - 1, env.D)  # one whole trial per lane
        ra.rollout(ev_env, pol, ev_traj)
        assert np.all(ev_traj.read(ra.TRAJ_FLAG)[-1] == M.INTERRUPT)
        r = ev_traj.read(ra.TRAJ_REWARD).astype(np.float64).sum(axis=0)
        ev_traj.close()
        ev_env.close()
        return r.mean(), r.std() / 64.0

    for period in range(periods):
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.3)
        ra.actor_critic_update(pol, cri, opt, traj, None, ccfg)
        if curve is not None:
            curve.append(evaluate()[0])
    return evaluate()


def test_the_rl2_model_learns_to_use_its_memory_on_five_arms(engine):
    """OneHotBandits::new(5), ten episodes per trial, 1,024 lanes, GRU(32) -> ReLU -> Linear as policy and critic (nine
    inputs: the wide constructors), rl_actor_critic_update with GAE lambda 0.3 and 10 critic steps.  A policy without
    memory across inner episodes earns 10 / 5 = 2.0 per trial in expectation; trying the arms in turn and staying on the
    hit earns 10 - (0 + 1 + 2 + 3 + 4) / 5 = 8.0.  The bar is the midpoint: an evaluation mean above 5.0 on 4,096 fresh
    trials (a trial's reward lies in [0, 10]: standard error at most 5 / 64 = 0.078).
    Measured on an MI355X with this configuration, evaluated after every period (profiles/wide_meta_learning.json): seed
    40 exceeds 5.0 from period 15 on (5.04; 6.93 after 30, 7.97 after 60), seed 50 from period 12 (5.33), seed 60 from
    period 13 (5.09); none falls back below.  The test runs 30 = twice the smallest count sufficient for all three; 60
    periods with an evaluation after each take 3.1 s, the 30 periods and one evaluation of the test about 1 s."""
    c = LEARNING
    mean, se = learn(engine, c["lanes"], c["episodes_per_trial"], c["trials_per_period"], c["hidden"], PERIODS, c["seed"],
                     c["arms"])
    print("mean trial reward after %d periods: %.3f (se %.3f)" % (PERIODS, mean, se))
    assert se < 0.08
    assert mean > 5.0
