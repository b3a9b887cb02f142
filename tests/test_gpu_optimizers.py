"""SGD, RMSProp and AdamW beside Adam (rl_optimizer_*, ra.Optimizer): the rule kernels of kernels_update.hip against the
numpy restatement tests/optim_ref.py (itself checked against torch.optim by tests/test_optimizers_cpu.py), through every
launcher that applies an optimiser step — the stand-alone step, the fused reduce + step (narrow and wide), the step behind
an all-reduce — and every entry point that takes an optimiser."""
import os
import threading

import numpy as np
import pytest

import optim_ref as R
import relearn_amd as ra

pytestmark = pytest.mark.gpu

H = 128
KIND = {"sgd": ra.OPTIMIZER_SGD, "rmsprop": ra.OPTIMIZER_RMSPROP, "adamw": ra.OPTIMIZER_ADAMW}
CASES = {name: (rule, kw) for name, rule, kw in R.CASES}
CASES["rmsprop_centered"] = ("rmsprop", dict(centered=True))  # centered without momentum: slots 0 and 2
SGD_MOMENTUM = ("sgd", dict(lr=1e-3, momentum=0.9))
RMSPROP_FULL = CASES["rmsprop_full"]


def config(rule, kw):
    c = ra.optimizer_config_default(KIND[rule])
    names = dict(lr="learning_rate")
    for k, v in kw.items():
        setattr(c, names.get(k, k), int(v) if isinstance(v, bool) else v)
    return c


def optimizer(module, case):
    rule, kw = case
    return ra.Optimizer(module, config(rule, kw))


def slots(opt, rule):
    """the state slots the optimiser has, by the restatement's names"""
    out = {}
    for i, name in enumerate(R.SLOTS[rule]):
        try:
            out[name] = opt.state(i)
        except ra.RelearnError as e:
            assert e.code == ra.ERR_INVALID_ARGUMENT and "no such slot" in str(e)
    return out


def rollout_pair(engine, n=2048, T=32, seeds=(31, 32)):
    env = ra.CartPoleEnv(engine, n, max_steps=60, seed_env=seeds[0], seed_actor=seeds[1])
    pol, cri = ra.Mlp(engine, 5, H, 2), ra.Mlp(engine, 5, H, 1)
    pol.init(2)
    cri.init(3)
    traj = ra.Trajectory(engine, n, T, 5)
    ra.rollout(env, pol, traj)
    ra.gae(traj, cri, 0.99, 0.95)
    return pol, cri, traj


# ---------------------------------------------------------------- 1. the stand-alone step
@pytest.mark.parametrize("case", sorted(CASES))
def test_step_host_matches_the_restatement(engine, case):
    """Five steps from host gradients (the sequence of test_gpu_parity.py::test_adam_step_matches_oracle).  SGD and RMSProp:
    parameters and every state slot bit for bit — each written operation is one correctly rounded f32 operation on both
    sides (RMSProp's square root is the correctly rounded one, not the native instruction) and the scalars are rounded from
    f64 once on both.  AdamW: the 2e-7 the Adam test grants for the f64 pow / sqrt of the bias corrections."""
    rule, kw = CASES[case]
    m = ra.Mlp(engine, 5, H, 1)
    m.init(9)
    p = m.get_params()
    opt = optimizer(m, (rule, kw))
    rng = np.random.default_rng(3)
    state = {}
    for k in range(5):
        g = (rng.standard_normal(len(p)) * 10.0 ** rng.integers(-6, 2)).astype(np.float32)
        opt.step_host(g)
        p = R.RULES[rule](p, g, state, **kw)
    got = slots(opt, rule)
    assert sorted(got) == sorted(k for k in state if k != "step")
    diff = {"params": float(np.abs(m.get_params() - p).max())}
    diff.update({k: float(np.abs(got[k] - state[k]).max()) for k in got})
    print(case, diff)
    assert opt.step_count == 5
    if rule == "adamw":
        assert all(d <= 2e-7 for d in diff.values())
    else:
        assert np.array_equal(m.get_params(), p)
        for k in got:
            assert np.array_equal(got[k], state[k]), k
    with pytest.raises(ra.RelearnError):
        opt.state(3)


# ---------------------------------------------------------------- 2. Adam is Adam
def test_optimizer_of_kind_adam_is_adam(engine):
    pol, cri, traj = rollout_pair(engine)
    twin = ra.Mlp(engine, 5, H, 1)
    twin.set_params(cri.get_params())
    a, b = ra.Adam(cri), ra.Optimizer(twin, ra.optimizer_config_default(ra.OPTIMIZER_ADAM))
    _, la = ra.critic_update(cri, a, traj, 5, want_losses=True)
    _, lb = ra.critic_update(twin, b, traj, 5, want_losses=True)
    assert np.array_equal(cri.get_params(), twin.get_params()) and np.array_equal(la, lb)
    assert b.step_count == 5 and np.any(b.state(0) != 0) and np.any(b.state(1) != 0)
    g = np.random.default_rng(5).standard_normal(cri.P).astype(np.float32)
    a.step_host(g)
    b.step_host(g)
    assert np.array_equal(cri.get_params(), twin.get_params())


# ---------------------------------------------------------------- 3. the fused reduce + step, and the launchers around it
def one_step_from_the_read_back_gradient(module, opt, case, gradient, update):
    """g at p0 through the gradient entry point, one update step, the restatement's step from (p0, g): bit for bit.  The
    step consumes vec[0..P) and the gradient entry points return it unscaled; rl_critic_gradient and the fused reduce + step
    launch choose the reduction's width from P alone (reduce_width, kernels_update.hip), so both sum the slab rows in the
    same order."""
    rule, kw = case
    p0 = module.get_params()
    g = gradient()
    assert np.array_equal(module.get_params(), p0) and np.all(np.isfinite(g)) and np.any(g != 0)
    update()
    want = R.RULES[rule](p0, g, {}, **kw)
    got = module.get_params()
    print(rule, kw, "max |device - restatement| =", float(np.abs(got - want).max()))
    assert np.array_equal(got, want)
    assert not np.array_equal(got, p0)
    assert opt.step_count == 1


@pytest.mark.parametrize("case", ["sgd_plain", "sgd_nesterov", "rmsprop_full"])
def test_fused_reduce_and_step_matches_the_restatement(engine, case):
    pol, cri, traj = rollout_pair(engine)
    c0 = cri.get_params()
    opt = optimizer(cri, CASES[case])
    one_step_from_the_read_back_gradient(cri, opt, CASES[case], lambda: ra.critic_gradient(cri, traj)[0],
                                         lambda: ra.critic_update(cri, opt, traj, 1))
    # K steps in one call (steps 2..K read the weight image the step kernel left) equal K one-step calls (each rebuilds
    # the image from the flat vector): the pattern of test_weight_image_kept_by_the_parameter_writers_equals_a_fresh_one
    K = 5
    cri.set_params(c0)
    o1 = optimizer(cri, CASES[case])
    _, losses = ra.critic_update(cri, o1, traj, K, want_losses=True)
    one_call, state_one = cri.get_params(), slots(o1, CASES[case][0])
    cri.set_params(c0)
    o2 = optimizer(cri, CASES[case])
    step_losses = [ra.critic_update(cri, o2, traj, 1, want_losses=True)[1][0] for _ in range(K)]
    assert np.all(np.isfinite(one_call))
    assert np.array_equal(one_call, cri.get_params())
    assert np.array_equal(losses, np.asarray(step_losses, dtype=np.float32))
    state_steps = slots(o2, CASES[case][0])
    assert sorted(state_one) == sorted(state_steps)
    for k in state_one:
        assert np.array_equal(state_one[k], state_steps[k]), k
    assert o1.step_count == o2.step_count == K


@pytest.mark.parametrize("case", ["sgd_nesterov", "rmsprop_full"])
@pytest.mark.parametrize("module", ["mlp_64_64", "gru_mlp"])
def test_step_behind_the_general_and_recurrent_reductions(engine, module, case):
    """the launchers that are not the fused one: a [64, 64] MLP critic (wide reduce + step: P > 2,048) and a GRU-MLP critic
    (the recurrent pass's own reduction, then the stand-alone step)"""
    if module == "mlp_64_64":
        pol, _, traj = rollout_pair(engine, 1024, 32)
        cri = ra.Mlp(engine, 5, [64, 64], 1)
        cri.init(4)
    else:
        env = ra.ChainEnv(engine, 64, max_steps=100, seed_env=3, seed_actor=4)
        pol = ra.GruMlp(engine, 5, 2)
        pol.init(11)
        cri = ra.GruMlp(engine, 5, 1)
        cri.init(12)
        traj = ra.Trajectory(engine, 64, 20, 5)
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.95)
    opt = optimizer(cri, CASES[case])
    one_step_from_the_read_back_gradient(cri, opt, CASES[case], lambda: ra.critic_gradient(cri, traj)[0],
                                         lambda: ra.critic_update(cri, opt, traj, 1))


def test_reinforce_and_ppo_with_sgd_on_the_policy(engine):
    """REINFORCE is one step on the gradient rl_policy_gradient returns (the surrogate's gradient at ratio 1, the loss being
    minus the surrogate): p1 == p0 + (-lr) g.  PPO's first step is taken at ratio 1 as well, by the clipped pass: the same
    check for one step."""
    case = ("sgd", dict(lr=1e-2))
    pol, cri, traj = rollout_pair(engine)
    p0 = pol.get_params()
    opt = optimizer(pol, case)
    one_step_from_the_read_back_gradient(pol, opt, case, lambda: ra.policy_gradient(pol, traj)[0],
                                         lambda: ra.reinforce_update(pol, opt, traj))
    pol.set_params(p0)
    opt = optimizer(pol, case)
    cfg = ra.ppo_config_default()
    cfg.opt_steps_per_update = 1
    one_step_from_the_read_back_gradient(pol, opt, case, lambda: ra.policy_gradient(pol, traj)[0],
                                         lambda: ra.ppo_update(pol, opt, traj, cfg))
    # several PPO steps with momentum: finite, improving, counted
    pol.set_params(p0)
    opt = optimizer(pol, ("sgd", dict(lr=1e-2, momentum=0.9, nesterov=True)))
    st, losses = ra.ppo_update(pol, opt, traj, want_losses=True)
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0] and opt.step_count == st.steps == 10


# ---------------------------------------------------------------- 4. the combined update
def test_actor_critic_update_with_an_sgd_critic_equals_the_two_updates_in_turn(engine):
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = 12

    def run(combined):
        env = ra.CartPoleEnv(engine, 2048, max_steps=60, seed_env=21, seed_actor=22)
        pol, cri = ra.Mlp(engine, 5, H, 2), ra.Mlp(engine, 5, H, 1)
        pol.init(2)
        cri.init(3)
        opt = optimizer(cri, SGD_MOMENTUM)
        traj = ra.Trajectory(engine, 2048, 32, 5)
        out = []
        for period in range(2):
            ra.rollout(env, pol, traj)
            ra.gae(traj, cri, 0.99, 0.95)
            if combined:
                pst, cst, losses = ra.actor_critic_update(pol, cri, opt, traj, None, ccfg, want_losses=True)
            else:
                pst = ra.trpo_update(pol, traj)
                cst, losses = ra.values_opt_update(cri, opt, traj, ccfg, want_losses=True)
            out.append((pol.get_params(), cri.get_params(), opt.state(0), losses.copy(), pst.as_dict()))
        assert opt.step_count == 24
        return out

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert np.array_equal(a[3], b[3]) and a[4] == b[4]
        assert np.all(np.isfinite(a[1])) and a[3][-1] < a[3][0]


# ---------------------------------------------------------------- 5. refused whole
N, T = 1024, 32


def history(scale, seed):
    """a synthetic history: observations N(0, 1) x scale, random actions, advantages and returns
    (as tests/test_gpu_numeric_range.py builds them)"""
    rng = np.random.default_rng(seed)
    obs = (rng.standard_normal((5, T + 1, N)) * scale).astype(np.float32)
    return dict(obs=obs, action=rng.integers(0, 2, size=(T, N)).astype(np.uint8),
                reward=np.ones((T, N), dtype=np.float32), flag=np.zeros((T, N), dtype=np.uint8),
                term_obs=np.zeros((5, T, N), dtype=np.float32),
                adv=rng.standard_normal((T, N)).astype(np.float32), rtg=(10.0 * rng.standard_normal((T, N))).astype(np.float32))


def load(engine, h):
    traj = ra.Trajectory(engine, N, T, 5)
    traj.write_all(h)
    traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
    traj.write(ra.TRAJ_RETURNS, h["rtg"])
    return traj


@pytest.mark.parametrize("good_first", [2, 0], ids=["refused_third", "refused_first"])
@pytest.mark.parametrize("case", [("sgd", dict(lr=1e-3, momentum=0.9)), RMSPROP_FULL], ids=["sgd_momentum", "rmsprop_full"])
def test_a_refused_update_is_refused_whole(engine, case, good_first):
    """the pattern of test_gpu_numeric_range.py::test_a_refused_update_is_refused_whole: [good updates, a refused one, 2 good
    updates] leaves exactly what [good updates, 2 good updates] leaves on a twin — parameters, every state slot, the step
    count.  With no good update before it the refused update is the optimiser's FIRST: SGD's first-step rule (the buffer
    starts as a copy of the gradient) must then apply to the step after it."""
    tg, tb = load(engine, history(1.0, 1)), load(engine, history(1e10, 2))  # 5 x 0.2 x 1e10 >= 2^31 for Glorot rows
    m, twin = ra.Mlp(engine, 5, H, 1), ra.Mlp(engine, 5, H, 1)
    m.init(11)
    twin.init(11)
    opt, opt_twin = optimizer(m, case), optimizer(twin, case)
    for _ in range(good_first):
        ra.critic_update(m, opt, tg, 3)
        ra.critic_update(twin, opt_twin, tg, 3)
    before, state_before, count_before = m.get_params(), slots(opt, case[0]), opt.step_count
    assert np.array_equal(before, twin.get_params()) and count_before == 3 * good_first
    with pytest.raises(ra.RelearnError) as err:
        ra.critic_update(m, opt, tb, 3)
    assert err.value.code == ra.ERR_UNSUPPORTED and "not applied" in str(err.value)
    assert np.array_equal(m.get_params(), before) and opt.step_count == count_before
    state_after = slots(opt, case[0])
    assert sorted(state_after) == sorted(state_before) and len(state_after) == (1 if case[0] == "sgd" else 3)
    for k in state_before:
        assert np.array_equal(state_after[k], state_before[k]), k
    for _ in range(2):
        ra.critic_update(m, opt, tg, 3)
        ra.critic_update(twin, opt_twin, tg, 3)
    assert np.array_equal(m.get_params(), twin.get_params()) and not np.array_equal(m.get_params(), before)
    for k, v in slots(opt_twin, case[0]).items():
        assert np.array_equal(slots(opt, case[0])[k], v), k
    assert opt.step_count == opt_twin.step_count == count_before + 6


# ---------------------------------------------------------------- 6. DQN
def test_dqn_with_rmsprop_updates_and_is_refused_whole(engine):
    env = ra.CartPoleEnv(engine, 256, max_steps=60, seed_env=9, seed_actor=10)
    q = ra.Mlp(engine, 5, H, 2)
    q.init(77)
    cfg = ra.dqn_config_default()
    cfg.exploration_kind, cfg.exploration_start = ra.SCHEDULE_CONSTANT, 0.5
    cfg.minibatch_steps, cfg.opt_steps_per_update, cfg.buffer_capacity = 2000, 3, 128
    opt = optimizer(q, RMSPROP_FULL)
    dqn = ra.Dqn(env, q, opt, cfg)
    dqn.collect(60)
    p0 = q.get_params()
    st, losses = dqn.update(want_losses=True)
    assert st.opt_steps == 3 and np.all(np.isfinite(losses)) and opt.step_count == 3
    assert np.all(np.isfinite(q.get_params())) and not np.array_equal(q.get_params(), p0)
    state = slots(opt, "rmsprop")
    assert sorted(state) == ["buf", "ga", "sq"] and all(np.any(v != 0) for v in state.values())
    # rows of ~2e8: 5 x 2e8 x max|obs| >= 2^31 (test_dqn_update_checks_its_weights_against_the_measured_observation_range)
    p = q.get_params()
    p[:5 * H] *= np.float32(1e9)
    p[6 * H:] *= np.float32(1e-9)
    q.set_params(p)
    with pytest.raises(ra.RelearnError) as err:
        dqn.update()
    assert err.value.code == ra.ERR_UNSUPPORTED and "numeric range" in str(err.value)
    assert np.array_equal(q.get_params(), p) and opt.step_count == 3
    for k, v in slots(opt, "rmsprop").items():
        assert np.array_equal(v, state[k]), k


# ---------------------------------------------------------------- 7. two loopback ranks
def run_rank(rank, world, uid, n, T, out):
    try:
        eng = ra.Engine(0)
        if world > 1:
            eng.comm_init(rank, world, uid)
        env = ra.CartPoleEnv(eng, n, max_steps=40, lane_offset=rank * n, seed_env=5, seed_actor=6)
        pol, cri = ra.Mlp(eng, 5, H, 2), ra.Mlp(eng, 5, H, 1)
        pol.init(2)
        cri.init(3)
        opt = optimizer(cri, SGD_MOMENTUM)
        traj = ra.Trajectory(eng, n, T, 5)
        res = {}
        for period in range(2):
            ra.rollout(env, pol, traj)
            ra.gae(traj, cri, 0.99, 0.95)
            if period == 0:
                res["gc"] = ra.critic_gradient(cri, traj)[0]
            _, losses = ra.critic_update(cri, opt, traj, 5, want_losses=True)
            res[period] = dict(critic=cri.get_params(), buf=opt.state(0), losses=losses)
        res["steps"] = opt.step_count
        out[rank] = res
    except BaseException as exc:  # surface the failure in the main thread
        out[rank] = exc
        raise


def launch(world, n_total, T):
    os.environ["RELEARN_LOOPBACK_COMM"] = "1"
    try:
        uid, out = ra.comm_unique_id(), {}
        threads = [threading.Thread(target=run_rank, args=(r, world, uid, n_total // world, T, out)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        for r in range(world):
            assert r in out and not isinstance(out[r], BaseException), out.get(r)
        return out
    finally:
        os.environ.pop("RELEARN_LOOPBACK_COMM", None)


def test_two_loopback_ranks_with_sgd_momentum_keep_identical_replicas():
    """two engines in one process joined by the in-process loopback collective (tests/test_gpu_multirank.py): the critic steps
    with SGD + momentum behind the all-reduce (reduce, all-reduce, stand-alone step).  The replicas are bit-identical after
    two updates; against one rank on all lanes the all-reduced gradient, the parameters and the momentum buffer agree to
    the rounding of test_gpu_multirank.py::check_probe_vectors (2e-6 of the largest entry: same samples, another order of
    the f32 partial sums — the rule is linear in the gradient, so the bound carries over to what it writes)."""
    two, one = launch(2, 1024, 32), launch(1, 1024, 32)[0]
    for period in range(2):
        for k in ("critic", "buf", "losses"):
            assert np.array_equal(two[0][period][k], two[1][period][k]), (period, k)
    assert two[0]["steps"] == two[1]["steps"] == one["steps"] == 10
    pairs = [("gc", two[0]["gc"], one["gc"])] + [(k, two[0][1][k], one[1][k]) for k in ("critic", "buf")]
    for name, a, b in pairs:
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        print(name, "max |two ranks - one rank| / max |one rank| =", np.abs(a - b).max() / np.abs(b).max())
        assert np.abs(a - b).max() <= 2e-6 * np.abs(b).max(), name
    assert not np.array_equal(one[1]["critic"], one[0]["critic"])


# ---------------------------------------------------------------- 8. the reference's quadratic on the device
@pytest.mark.parametrize("rule", ["sgd", "rmsprop"])
def test_the_reference_quadratic_on_the_device(engine, rule):
    """optimizers/mod.rs:140-169 with the steps taken by the device: default configuration at learning rate 0.1, 500 steps
    on the first two parameters of a module from 0, within 1e-3 of [-1, 1]; the other parameters get a zero gradient,
    which both rules leave in place"""
    m = ra.Mlp(engine, 5, H, 1)
    m.init(9)
    p0 = m.get_params()
    p0[:2] = 0.0
    m.set_params(p0)
    opt = optimizer(m, (rule, dict(lr=0.1)))
    g = np.zeros(m.P, dtype=np.float32)
    for _ in range(500):
        g[:2] = R.quadratic_gradient(m.get_params()[:2])
        opt.step_host(g)
    p = m.get_params()
    err = float(np.linalg.norm(p[:2].astype(np.float64) - np.array([-1.0, 1.0])))
    print(rule, "|x - [-1, 1]| =", err)
    assert err < 1e-3
    assert np.array_equal(p[2:], p0[2:]) and opt.step_count == 500
