"""Recurrent chains over 3 to 8 actions — rl_rnn_chain_create / ra.RnnChain, ChainConfig<GruConfig | LstmConfig,
MlpConfig | LinearConfig> on IndexSpace::new(3..8) — on the lane-per-thread kernels (relearn_amd/csrc/
kernels_seq_stack.hip: the head's outputs in passes of four rows) and the k-plane per-sample kernels
(kernels_seq_bwd.hip, kernels_seq_fvp.hip), against the oracle (tests/seq_multi_ref.py; pinned on the CPU at A = 3 and 8
by tests/test_seq_multi_ref.py): the forward bit for bit, gradients / Fisher-vector products / loss / KL against f64 at the
bars of tests/test_gpu_stacked.py, the clipped PPO gradient off ratio 1, rollouts on the meta-bandit lanes of three and
four arms against a closed-loop reference and on MemoryGame / k-armed bandit lanes against the oracle's lanes, every
update entry point, actor documents, refusals, one trajectory shared with a two-output module, and the RL2 model learning
to use its memory on three arms.

Shapes: A in {3, 4, 5, 8} (3 and 5 are off the four-row pass, 8 is two full passes); H in {7, 33} and H2 in {6, 33} (unit-loop
tails, and a second trip of one unit); one and two layers; one module without recurrent bias vectors; n in {1, 70} (one
lane; a second workgroup with a ragged end); T = 5 with Terminate and Interrupt inside and at the horizon."""
import ctypes as C

import numpy as np
import pytest

import cbor_ref
import meta_lanes_ref as M
import oracle as O
import relearn_amd as ra
import seq_multi_ref as R
from oracle import stacked as S
from test_gpu_stacked import GRAD_RTOL, rel_err

pytestmark = pytest.mark.gpu

NETS = [
    R.Net("gru", 7, 7, 1, 6, True, 3),      # the three-arm meta lanes' width; every loop below its block size
    R.Net("lstm", 8, 33, 2, 33, True, 5),   # second unit trip of one unit in both widths, two layers, five outputs
    R.Net("gru", 5, 33, 1, 0, True, 8),     # Linear tail, two full passes of output rows
    R.Net("lstm", 6, 7, 2, 0, False, 4),    # Linear tail without recurrent bias vectors, exactly one pass
    R.Net("lstm", 5, 7, 1, 6, True, 8),     # MLP tail, two passes
    R.Net("gru", 8, 33, 2, 6, False, 4),    # MLP tail without recurrent bias vectors
    R.Net("gru", 5, 128, 1, 128, True, 3),  # the tile kernels' shape: more than two outputs keeps it off them
]
T = 5


def module(engine, net, seed=None):
    m = ra.RnnChain(engine, net.cell, net.D, net.H, net.A, num_layers=net.L, bias=net.bias, mlp_hidden=net.H2 or None)
    assert m.P == R.num_params(net)
    if seed is not None:
        m.init(seed)
    return m


def written(engine, net, n, seed):
    h = R.history(net, n, T, seed)
    traj = ra.Trajectory(engine, n, T, net.D)
    traj.write_all(h)
    traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
    traj.write(ra.TRAJ_RETURNS, h["rtg"])
    return traj, h


def code_of(fn):
    with pytest.raises(ra.RelearnError) as e:
        fn()
    return e.value.code


# ------------------------------------------------------------------------------------------------ 1. init, forward
@pytest.mark.parametrize("net", NETS, ids=R.net_id)
def test_initialisation_draws_the_head_at_its_real_width(engine, net):
    m = module(engine, net, 31)
    p = m.get_params()
    assert np.array_equal(p, R.init(net, 31))
    none_if = lambda x: x if net.bias else None
    m.init_with(33, O.RNN_DEFAULT_INITS[0], O.RNN_DEFAULT_INITS[1], none_if(R.BIAS_INIT), *O.RNN_DEFAULT_INITS[3:])
    inits = list(O.RNN_DEFAULT_INITS)
    if net.bias:
        inits[2] = R.BIAS_INIT
    assert np.array_equal(m.get_params(), R.init(net, 33, tuple(inits)))
    q = np.random.default_rng(2).normal(size=m.P).astype(np.float32)
    m.set_params(q)
    assert np.array_equal(m.get_params(), q)


@pytest.mark.parametrize("net", NETS, ids=R.net_id)
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
    for q in range(1, net.A):  # no output row repeats another
        assert not np.array_equal(out_d[q], out_d[q - 1])


# ------------------------------------------------------------------------------------------------ 2. f64 comparisons
@pytest.mark.parametrize("net", NETS, ids=R.net_id)
@pytest.mark.parametrize("n", [1, 70])
def test_gradient_fvp_loss_and_kl_against_f64(engine, net, n):
    """rl_policy_gradient, rl_policy_fvp and rl_policy_loss_kl on a host-written trajectory whose action plane uses every
    index: GRAD_RTOL for the gradient, 2e-5 for the Fisher-vector product (tests/test_gpu_stacked.py's bars), 2e-5 / 2e-4
    for loss and KL (tests/test_gpu_multi_action.py's)"""
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
    # loss and KL of moved parameters against the old ones (the line search's evaluation)
    moved = (p + 0.01 * v).astype(np.float32)
    m.set_params(moved)
    loss1, kl1 = ra.policy_loss_kl(m, traj, p)
    z1, _, _ = S.forward(spec, R.to_oracle(net, moved), h, want_succ=False)
    l64, k64 = R.loss_and_kl(z1, logits, h["action"], h["adv"])
    print("%s n=%d: loss %.8g (f64 %.8g), KL %.6g (f64 %.6g)" % (R.net_id(net), n, loss1, l64, kl1, k64))
    assert abs(loss1 - l64) <= 2e-5 * abs(l64) + 1e-7
    # KL = mean_b sum_a p0_a (lp0_a - lp_a): in f32 each log-probability is (z - max) - log(sum), two roundings of its
    # own magnitude, so a difference lp0_a - lp_a carries up to 4 ulp (2^-24) of |lp| that no term cancels; the weights
    # p0_a sum to 1.  That absolute floor stands beside the relative bar (it matters where the KL itself is ~1e-4 over a
    # handful of samples; tests/test_gpu_multi_action.py averages 1,760 samples and uses 1e-8)
    kl_floor = 4 * ULP * np.abs(R.log_softmax(logits)).max(0).mean()
    assert abs(kl1 - k64) <= 2e-4 * abs(k64) + kl_floor
    m.set_params(p)
    assert ra.policy_loss_kl(m, traj, p)[1] == 0.0


ULP = 2.0 ** -24


def sgd_steps(pol, traj, p0, lr, steps, clip):
    """`steps` PPO steps under plain SGD from p0 with a fresh optimiser (tests/test_gpu_ppo_clip.py's method)"""
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


# (net, SGD rate): the rate is chosen on the CPU (the f64 oracle's step from the same start) so that the first step
# clips at least a fifth of the samples at clip distance 0.2 and leaves no ratio within 3e-4 of a bound
PPO_CASES = [(R.Net("gru", 7, 12, 1, 6, True, 3), 2.0), (R.Net("lstm", 7, 12, 1, 0, True, 3), 4.0)]


@pytest.mark.parametrize("net,lr", PPO_CASES, ids=[R.net_id(c[0]) for c in PPO_CASES])
def test_clipped_ppo_gradient_off_ratio_one(engine, net, lr):
    """Under plain SGD from p0, one rl_ppo_update step gives p1 and two give p2; both runs share log pi_0 of p0, so
    (p1 - p2) / lr is the clipped gradient AT p1, where the first (large) step has moved the ratios off 1 both ways.
    Against the f64 restatement (tests/seq_multi_ref.py: ppo_dlogits through oracle.stacked's backward) at clip distances
    0.2 and 0; the bar is GRAD_RTOL of max |g| plus the readback term 2^-24 (|p2_j| + lr |g_j|) / lr of element j."""
    n = 70
    m = module(engine, net, 51)
    traj, h = written(engine, net, n, 8)
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


# ------------------------------------------------------------------------------------------------ 3. rollouts
def meta_run(engine, case, variants):
    net = case.net
    try:
        env = ra.MetaBanditEnv(engine, case.n, net.A, case.E, case.arms, lane_offset=case.offset,
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


@pytest.mark.parametrize("case", R.META_CASES, ids=R.meta_case_id)
def test_rollout_on_meta_bandit_lanes(engine, case):
    """three arms (D = 7) and four arms (D = 8): all steps in one launch (kernel variant 0), the launch sequence per step
    (variant 1), and one then the other, against the closed-loop reference — whole planes, obs[T] and term_obs included,
    two collections in a row, no sample excused (tests/test_seq_multi_ref.py holds every margin above 1e-5)"""
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
    assert sorted(np.unique(np.concatenate([q["action"] for q in runs["one launch"][0]]))) == list(range(net.A))


def sampled_actions_follow_the_logits(got, z, seed_actor, word0):
    """the recorded actions are the inverse-CDF draws at the teacher-forced logits (samples within 1e-6 of a cumulative
    boundary set aside: the closed-loop cases above excuse none)"""
    A, T_, n = z.shape
    r = O.Prng()
    checked = 0
    for t in range(T_):
        zz = z[:, t].astype(np.float64)
        cum = np.cumsum(np.exp(R.log_softmax(zz)), axis=0)[:-1]  # [A - 1][n]
        for i in range(n):
            O.lib().oracle_prng_seed_from_u64(C.byref(r), seed_actor)
            O.lib().oracle_prng_set_stream(C.byref(r), i)
            O.lib().oracle_prng_set_word_pos(C.byref(r), word0 + t)
            u = O.lib().oracle_prng_gen_f32(C.byref(r))
            if np.abs(u - cum[:, i]).min() > 1e-6:
                assert got["action"][t, i] == int((u >= cum[:, i]).sum()), (t, i)
                checked += 1
    assert checked > 0.99 * n * T_


@pytest.mark.parametrize("net", [R.Net("gru", 5, 12, 1, 6, True, 3), R.Net("lstm", 5, 9, 2, 0, True, 3)], ids=R.net_id)
def test_stepwise_rollout_on_memory_game_lanes(engine, net):
    """MemoryGame::new(3, 2) (five features, three actions): the env side replayed bit for bit through the oracle's lanes,
    the logits against the teacher-forced C forward, the actions against the sampler, two collections in a row"""
    n, T_ = 70, 9
    env = ra.MemoryEnv(engine, n, 3, 2, seed_env=7, seed_actor=8)
    assert (env.D, env.A) == (5, 3)
    sim = O.MemoryLaneSim(n, 3, 2, seed_env=7, seed_actor=8)
    pol = module(engine, net, 13)
    traj = ra.Trajectory(engine, n, T_, 5)
    seen = set()
    for period in range(2):
        ra.rollout(env, pol, traj)
        got = traj.read_all()
        if period == 0:
            assert np.array_equal(got["obs"][:, 0, :], sim.observe())
        for t in range(T_):
            reward, flag, obs, term = sim.step(got["action"][t])
            assert np.array_equal(got["reward"][t], reward) and np.array_equal(got["flag"][t], flag), t
            assert np.array_equal(got["obs"][:, t + 1, :], obs), t
        z, _ = O.stack_seq_forward(R.shape_of(net), net.L, R.to_oracle(net, pol.get_params()), got, want_succ=False)
        assert np.array_equal(z, pol.seq_forward(traj, want_succ=False)[0])
        sampled_actions_follow_the_logits(got, z, 8, period * T_)
        seen |= set(np.unique(got["action"]))
        assert (got["flag"] == O.TERMINATE).any()
    assert seen == {0, 1, 2}


def test_stepwise_rollout_on_a_four_armed_bandit(engine):
    values = (0.25, -1.0, 1.5, 0.5)
    n, T_, net = 70, 6, R.Net("gru", 5, 7, 1, 0, True, 4)
    env = ra.BanditEnv(engine, n, values=values, seed_env=5, seed_actor=6)
    assert (env.D, env.A) == (5, 4)
    pol = module(engine, net, 3)
    traj = ra.Trajectory(engine, n, T_, 5)
    ra.rollout(env, pol, traj)
    got = traj.read_all()
    one_hot = np.zeros((5, n), dtype=np.float32)
    one_hot[0] = 1.0
    v32 = np.asarray(values, dtype=np.float32)
    assert sorted(np.unique(got["action"])) == [0, 1, 2, 3]
    assert np.array_equal(got["reward"], v32[got["action"]]) and (got["flag"] == O.TERMINATE).all()
    assert np.array_equal(got["obs"], np.broadcast_to(one_hot[:, None, :], (5, T_ + 1, n)))
    z, _ = O.stack_seq_forward(R.shape_of(net), net.L, R.to_oracle(net, pol.get_params()), got, want_succ=False)
    assert np.array_equal(z, pol.seq_forward(traj, want_succ=False)[0])
    sampled_actions_follow_the_logits(got, z, 6, 0)


# ------------------------------------------------------------------------------------------------ 4. whole updates
@pytest.mark.parametrize("update", ["trpo", "ppo", "reinforce", "actor_critic", "actor_critic_begin_finish"])
def test_updates_on_a_collected_trajectory_equal_the_written_one(engine, update):
    """every update entry point on a trajectory collected on three-arm meta lanes equals the same call on the same planes
    written by the host (the check tests/test_gpu_meta_bandit.py makes for two arms)"""
    n, T_, E = 70, 10, 3
    pnet, cnet = R.Net("gru", 7, 12, 1, 0, True, 3), R.Net("lstm", 7, 8, 1, 6, True, 1)
    results, planes = [], None
    for source in ("rollout", "written"):
        env = ra.MetaBanditEnv(engine, n, 3, E, "one_hot", seed_env=3, seed_actor=4)
        pol, cri = module(engine, pnet, 31), module(engine, cnet, 32)
        traj = ra.Trajectory(engine, n, T_, env.D)
        if source == "rollout":
            ra.rollout(env, pol, traj)
            planes = traj.read_all()
            assert sorted(np.unique(planes["action"])) == [0, 1, 2]
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


def test_begin_finish_equals_the_joint_call(engine):
    outs = []
    for how in ("joint", "begin-finish"):
        env = ra.MemoryEnv(engine, 70, 3, 2, seed_env=5, seed_actor=6)
        pol, cri = module(engine, R.Net("gru", 5, 12, 2, 6, True, 3), 2), module(engine, R.Net("gru", 5, 12, 1, 0, True, 1), 3)
        opt = ra.Adam(cri)
        ccfg = ra.values_opt_config_default()
        ccfg.opt_steps_per_update = 3
        traj = ra.Trajectory(engine, 70, 9, 5)
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.95)
        if how == "joint":
            pst, cst, losses = ra.actor_critic_update(pol, cri, opt, traj, None, ccfg, want_losses=True)
        else:
            pst = ra.actor_critic_update_begin(pol, cri, opt, traj, None, ccfg)
            cst, losses = ra.actor_critic_update_finish(traj, want_losses=True)
        outs.append((pol.get_params(), cri.get_params(), pst.as_dict(), losses.copy()))
    a, b = outs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])


# ------------------------------------------------------------------------------------------------ 5. documents, refusals
@pytest.mark.parametrize("net", [R.Net("gru", 5, 12, 2, 6, True, 3), R.Net("lstm", 5, 9, 1, 0, False, 3)], ids=R.net_id)
def test_actor_documents(engine, net):
    """a round trip on MemoryGame::new(3, 2): the head tensors are [A, H2] / [A, H]; meta lanes stay refused"""
    env = ra.MemoryEnv(engine, 64, 3, 2)
    m = module(engine, net, 19)
    doc = ra.actor_to_cbor(env, m)
    chain = cbor_ref.decode(doc)["policy_module"]
    p, A = m.get_params(), net.A
    if net.H2 == 0:
        assert chain["second"]["kernel"]["shape"] == [A, net.H] and chain["second"]["bias"]["shape"] == [A]
        assert bytes(chain["second"]["kernel"]["data"]) == p[-A * net.H - A:-A].tobytes()
        assert bytes(chain["second"]["bias"]["data"]) == p[-A:].tobytes()
    else:
        assert p[-A * net.H2 - A:-A].tobytes() in bytes(doc) and p[-A:].tobytes() in bytes(doc)
    assert chain["first"]["weights"]["has_biases"] is net.bias
    other = module(engine, net)
    ra.module_from_cbor(other, doc)
    assert np.array_equal(other.get_params(), p)
    two = module(engine, net._replace(A=2), 5)  # a document of another action count is refused
    before = two.get_params()
    assert code_of(lambda: ra.module_from_cbor(two, doc)) == ra.ERR_INVALID_ARGUMENT
    assert np.array_equal(two.get_params(), before)
    meta = ra.MetaBanditEnv(engine, 8, 3, 2)
    m7 = module(engine, net._replace(D=7), 1)
    assert code_of(lambda: ra.actor_to_cbor(meta, m7)) == ra.ERR_UNSUPPORTED


def test_refusals(engine):
    h = C.c_void_p()

    def create(**kw):
        cfg = ra.rnn_chain_config_default("gru")
        assert (cfg.cell, cfg.in_dim, cfg.hidden, cfg.num_layers, cfg.rnn_bias, cfg.mlp_hidden, cfg.out_dim) == (0, 5, 128, 1, 1, 128, 2)
        for k, v in kw.items():
            setattr(cfg, k, v)
        return ra.lib().rl_rnn_chain_create(engine.h, C.byref(cfg), C.byref(h))

    assert create(out_dim=0) == ra.ERR_BUILD_AGENT and not h.value
    assert create(out_dim=9) == ra.ERR_BUILD_AGENT and not h.value
    assert create(num_layers=0) == ra.ERR_BUILD_AGENT
    assert create(num_layers=5) == ra.ERR_UNSUPPORTED
    for kw in (dict(in_dim=0), dict(in_dim=9), dict(hidden=0), dict(hidden=257), dict(mlp_hidden=257), dict(rnn_bias=2), dict(cell=2)):
        assert create(**kw) == ra.ERR_BUILD_AGENT, kw
        assert not h.value
    cfg = ra.rnn_chain_config_default("lstm")
    assert cfg.cell == 1
    assert ra.lib().rl_rnn_chain_create(engine.h, C.byref(cfg), None) == ra.ERR_INVALID_ARGUMENT
    assert ra.lib().rl_rnn_chain_create(engine.h, None, C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    assert ra.lib().rl_rnn_chain_config_default(C.c_int32(2), C.byref(cfg)) == ra.ERR_BUILD_AGENT
    for kw in (dict(in_dim=1, hidden=1, mlp_hidden=0, out_dim=1), dict(in_dim=8, hidden=256, num_layers=4, mlp_hidden=256, out_dim=8, cell=1)):
        assert create(**kw) == ra.OK  # the corners of the range build
        assert ra.lib().rl_mlp_destroy(h) == ra.OK
    # the five old constructors remain the two-action shorthand
    u32, i32 = C.c_uint32, C.c_int32
    L = ra.lib()
    assert L.rl_gru_mlp_create(engine.h, u32(5), u32(8), u32(8), u32(3), C.byref(h)) == ra.ERR_BUILD_AGENT
    assert L.rl_lstm_mlp_create(engine.h, u32(5), u32(8), u32(8), u32(3), C.byref(h)) == ra.ERR_BUILD_AGENT
    assert L.rl_rnn_mlp_create(engine.h, i32(0), u32(5), u32(8), u32(1), u32(8), u32(3), C.byref(h)) == ra.ERR_BUILD_AGENT
    assert L.rl_rnn_mlp_create_config(engine.h, i32(0), u32(5), u32(8), u32(1), i32(1), u32(8), u32(3), C.byref(h)) == ra.ERR_BUILD_AGENT
    assert L.rl_rnn_linear_create(engine.h, i32(0), u32(5), u32(8), u32(1), i32(1), u32(3), C.byref(h)) == ra.ERR_BUILD_AGENT
    # for out_dim <= 2 the new constructor builds what the old ones build: same P, same bits through the same kernels
    n = 64
    traj, hist = written(engine, R.Net("gru", 5, 128, 1, 128, True, 2), n, 9)
    old, new = ra.GruMlp(engine, 5, 2), ra.RnnChain(engine, "gru", 5, 128, 2, mlp_hidden=128)
    old.init(7)
    new.init(7)
    assert old.P == new.P and np.array_equal(old.get_params(), new.get_params())
    assert np.array_equal(old.seq_forward(traj)[0], new.seq_forward(traj)[0])
    assert np.array_equal(ra.policy_gradient(old, traj)[0], ra.policy_gradient(new, traj)[0])
    # shapes against envs
    env4 = ra.MemoryEnv(engine, n, 4, 1)  # five features, four actions
    env3 = ra.MemoryEnv(engine, n, 3, 2)  # five features, three actions
    three = module(engine, R.Net("gru", 5, 8, 1, 6, True, 3), 1)
    two = module(engine, R.Net("gru", 5, 8, 1, 6, True, 2), 1)
    assert code_of(lambda: ra.rollout(env4, three, ra.Trajectory(engine, n, 4, 5))) == ra.ERR_INVALID_ARGUMENT
    assert code_of(lambda: ra.rollout(env3, two, ra.Trajectory(engine, n, 4, 5))) == ra.ERR_UNSUPPORTED
    # rl_dqn_create is untouched: a recurrent action-value module is refused, and so are more than two actions
    env2 = ra.MemoryEnv(engine, n, 2, 3)
    assert code_of(lambda: ra.Dqn(env2, two, ra.Adam(two), ra.dqn_config_default())) == ra.ERR_BUILD_AGENT
    assert code_of(lambda: ra.Dqn(env3, three, ra.Adam(three), ra.dqn_config_default())) == ra.ERR_UNSUPPORTED
    # a trajectory collected on three actions does not update a policy of four outputs
    t3 = ra.Trajectory(engine, n, 4, 5)
    ra.rollout(env3, three, t3)
    four = module(engine, R.Net("gru", 5, 8, 1, 6, True, 4), 1)
    assert code_of(lambda: ra.policy_gradient(four, t3)) == ra.ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------ 6. a shared trajectory
def test_a_trajectory_serves_two_and_eight_outputs_in_turn(engine):
    """lp0, dz and the output planes grow where the eight-output module first meets the trajectory; the two-output
    module's results before and after equal those on a fresh trajectory, bit for bit"""
    n = 70
    net2, net8 = R.Net("gru", 5, 9, 2, 6, True, 2), R.Net("lstm", 5, 7, 1, 0, True, 8)
    h2 = R.history(net2, n, T, 11)
    h8 = dict(h2, action=R.history(net8, n, T, 11)["action"])

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

    m2, m8 = module(engine, net2, 21), module(engine, net8, 22)
    fresh = two_output_results(ra.Trajectory(engine, n, T, 5), m2)
    shared = ra.Trajectory(engine, n, T, 5)
    first = two_output_results(shared, m2)
    fill(shared, h8)
    spec8, full8 = R.spec_of(net8), R.to_oracle(net8, m8.get_params())
    z8, _, _ = S.forward(spec8, full8, h8, want_succ=False)
    g64 = R.restrict(net8, S.backward(spec8, full8, h8, R.surrogate_dlogits(z8, h8["action"], h8["adv"])[0]))
    g8 = ra.policy_gradient(m8, shared)[0]
    assert rel_err(g8, g64) < GRAD_RTOL
    out8, _ = m8.seq_forward(shared)
    assert np.array_equal(out8, O.stack_seq_forward(R.shape_of(net8), 1, full8, h8)[0])
    ra.trpo_update(m8, shared)  # (a whole update: CG vectors, line search, the P-sized workspace at the wider module)
    assert np.all(np.isfinite(m8.get_params()))
    after = two_output_results(shared, m2)
    assert same(fresh, first) and same(fresh, after)
    # and the eight-output module again, on the planes the two-output module has used since
    fill(shared, h8)
    m8.set_params(R.restrict(net8, full8))
    assert np.array_equal(ra.policy_gradient(m8, shared)[0], g8)


# ------------------------------------------------------------------------------------------------ 7. learning
LEARNING = dict(lanes=1024, episodes_per_trial=6, trials_per_period=2, hidden=32, seed=40)
PERIODS = 18  # twice the smallest count that clears the bar with three seeds (profiles/seq_multi_learning.json)


def learn(engine, n, E, trials, H, periods, seed, arms=3, curve=None):
    T_ = trials * (2 * E - 1)
    env = ra.MetaBanditEnv(engine, n, arms, E, "one_hot", seed_env=seed, seed_actor=seed + 1)
    pol = ra.RnnChain(engine, "gru", env.D, H, arms)
    cri = ra.RnnChain(engine, "gru", env.D, H, 1)
    pol.init(seed + 2)
    cri.init(seed + 3)
    opt = ra.Adam(cri)
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = 10
    traj = ra.Trajectory(engine, n, T_, env.D)

    def evaluate():
        ev_env = ra.MetaBanditEnv(engine, 4096, arms, E, "one_hot", seed_env=seed + 10, seed_actor=seed + 11)
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


def test_the_rl2_model_learns_to_use_its_memory_on_three_arms(engine):
    """OneHotBandits::new(3) (the reference's meta test distribution, src/agents/meta.rs:239), six episodes per trial,
    GRU(32) -> ReLU -> Linear as policy and critic, rl_actor_critic_update with GAE lambda 0.3 and 10 critic steps (the
    configuration of tests/test_gpu_chain_linear.py's two-arm run).  A policy without memory across inner episodes earns
    at most 6 / 3 = 2.0 per trial in expectation; trying the arms in turn earns 6 - 1 = 5.0.  The bar is the midpoint: an
    evaluation mean above 3.5 on 4,096 fresh trials (standard error below 0.03).
    Measured on an MI355X with this configuration, evaluated after every period (profiles/seq_multi_learning.json): seed
    40 first exceeds 3.5 after 8 periods (3.54) and reads 4.83 after 18, 4.99 after 30; seed 50 after 8 (3.61); seed 60
    after 9 (3.73, from 3.36 after 8); all three stay above the bar from then on and level off at 4.99.  The test runs
    18 = twice the smallest count sufficient for all three; the 18 periods and the evaluation take 0.5 s."""
    c = LEARNING
    mean, se = learn(engine, c["lanes"], c["episodes_per_trial"], c["trials_per_period"], c["hidden"], PERIODS, c["seed"])
    print("mean trial reward after %d periods: %.3f (se %.3f)" % (PERIODS, mean, se))
    assert se < 0.03
    assert mean > 3.5
