"""Categorical policies over 3 to 8 actions (`IndexSpace::new(n)`, spaces/index.rs:19-22) on feed-forward modules:
`MemoryGame::new(num_actions, history_len)` lanes (src/envs/memory.rs) and k-armed `DeterministicBandit::from_values`
lanes (src/envs/bandits.rs:109-116) with policies of out_dim = the action count, through rollouts, the policy-gradient
family and the actor document.  The yardsticks are the oracle's lanes, forward, sampler, f64 gradients and f32 TRPO step
(all general in the action count), and an f64 torch-autograd restatement of `Trpo::update`'s closure,
`HessianVectorProduct` and `Ppo::update` written here for shapes the oracle's single-hidden-layer functions do not take.
Tolerances are those tests/test_gpu_general_mlp.py and tests/test_gpu_parity.py use for the same quantities at two
actions."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle as O
import relearn_amd as ra

pytestmark = pytest.mark.gpu

# (num_actions, history_len): 7, 8, 5 and 8 observation features
SIZES = [(3, 4), (4, 4), (3, 2), (7, 1)]


def make(engine, in_dim, hidden, out_dim, seed, act="Relu", out_act="Identity"):
    m = ra.Mlp(engine, in_dim, hidden, out_dim, act, out_act)
    m.init(seed)
    return m


def replay_env_side(sim, got, T):
    """the recorded env side through the oracle's lanes, fed the device's actions"""
    assert np.array_equal(got["obs"][:, 0, :], sim.observe())
    for t in range(T):
        reward, flag, obs, term = sim.step(got["action"][t])
        assert np.array_equal(got["reward"][t], reward) and np.array_equal(got["flag"][t], flag), t
        assert np.array_equal(got["obs"][:, t + 1, :], obs), t


# ------------------------------------------------------------------------------------------------ 1. rollouts
@pytest.mark.parametrize("A,L", SIZES)
def test_rollout_is_bit_exact_against_the_oracle_lanes(engine, A, L):
    n, T, D = 256, 3 * (L + 1) + 1, A + L
    env = ra.MemoryEnv(engine, n, A, L, seed_env=7, seed_actor=8)
    assert (env.D, env.A) == (D, A)
    pol = make(engine, D, [32], A, 11)
    traj = ra.Trajectory(engine, n, T, D)
    sim = O.MemoryLaneSim(n, A, L, seed_env=7, seed_actor=8)
    for _ in range(2):  # the second rollout continues the lanes and the streams
        ra.rollout(env, pol, traj)
        got = traj.read_all()
        want = sim.rollout_mlp(O.MlpShape(D, 32, A), pol.get_params(), T)
        for k in ("obs", "action", "reward", "flag"):
            assert np.array_equal(got[k], want[k]), k
    assert sorted(np.unique(got["action"])) == list(range(A))
    assert (got["flag"] == O.TERMINATE).any() and (got["reward"] == 1.0).any() and (got["reward"] == -1.0).any()


def test_rollout_of_a_two_layer_policy_replays_through_the_oracle_lanes(engine):
    A, L, n, T = 4, 3, 192, 17
    D = A + L
    env = ra.MemoryEnv(engine, n, A, L, seed_env=3, seed_actor=4)
    pol = make(engine, D, [16, 16], A, 13, "Tanh")
    traj = ra.Trajectory(engine, n, T, D)
    sim = O.MemoryLaneSim(n, A, L, seed_env=3, seed_actor=4)
    for _ in range(2):
        ra.rollout(env, pol, traj)
        got = traj.read_all()
        replay_env_side(sim, got, T)
    assert sorted(np.unique(got["action"])) == list(range(A))


def test_rollout_under_a_visible_step_limit(engine):
    """num_actions + history_len + the remaining-steps feature: the interrupted successor observations too"""
    A, L, n, T = 3, 4, 128, 14
    D = A + L + 1
    env = ra.MemoryEnv(engine, n, A, L, max_steps=3, limit=ra.LIMIT_VISIBLE, seed_env=5, seed_actor=6)
    assert (env.D, env.A) == (D, A)
    pol = make(engine, D, [32], A, 17)
    traj = ra.Trajectory(engine, n, T, D)
    ra.rollout(env, pol, traj)
    got = traj.read_all()
    sim = O.MemoryLaneSim(n, A, L, max_steps=3, limit=O.LIMIT_VISIBLE, seed_env=5, seed_actor=6)
    want = sim.rollout_mlp(O.MlpShape(D, 32, A), pol.get_params(), T)
    for k in ("obs", "action", "reward", "flag"):
        assert np.array_equal(got[k], want[k]), k
    m = got["flag"] == O.INTERRUPT
    assert m.any() and np.array_equal(got["term_obs"][:, m], want["term_obs"][:, m])


# ------------------------------------------------------------------------------------------------ 2. logits, sampling
@pytest.mark.parametrize("A,L,hidden,act", [(a, l, [32], "Relu") for a, l in SIZES] + [(4, 3, [16, 16], "Tanh")])
def test_logits_and_one_step_of_actions(engine, A, L, hidden, act):
    n, D = 320, A + L
    env = ra.MemoryEnv(engine, n, A, L, seed_env=21, seed_actor=22)
    pol = make(engine, D, hidden, A, 23, act)
    x = np.ascontiguousarray(env.observe().T)
    z = pol.forward(x)
    assert z.shape == (n, A)
    assert np.array_equal(z, O.mlp_layers_forward(D, hidden, A, pol.get_params(), x, act, "Identity"))
    traj = ra.Trajectory(engine, n, 1, D)
    ra.rollout(env, pol, traj)
    got = traj.read(ra.TRAJ_ACTION)[0]
    for i in range(n):
        w = engine.stream_words(22, i, 0, 1)[0]  # the lane's actor stream, word = the global step
        u = np.float32(w >> 8) * np.float32(1.0 / (1 << 24))
        zi = z[i].astype(np.float32)
        lp = np.zeros(A, dtype=np.float32)
        O.lib().oracle_log_softmax_f32(O.f32p(np.ascontiguousarray(zi)), A, O.f32p(lp), 0)
        assert got[i] == O.lib().oracle_categorical_sample_u(O.f32p(lp), A, C.c_float(u), 0), i


# ------------------------------------------------------------------------------------------------ 3. gradients, FVP
def torch_restatement(params, in_dim, hidden, A, act, x, a, adv, vec=None, params0=None, clip=None):
    """f64 autograd statement of Trpo::update's closure (policies/trpo.rs:97-146), HessianVectorProduct
    (conjugate_gradient.rs:262-339) and Ppo::update's clipped surrogate (policies/ppo.rs:124-137)"""
    import torch
    dims = [in_dim] + list(hidden) + [A]
    fn = {"Relu": torch.relu, "Tanh": torch.tanh, "Sigmoid": torch.sigmoid, "Identity": lambda t: t}[act]
    xt = torch.tensor(np.asarray(x, dtype=np.float64))
    at = torch.tensor(np.asarray(a, dtype=np.int64))[:, None]
    advt = torch.tensor(np.asarray(adv, dtype=np.float64))

    def log_probs(p):
        h, k = xt, 0
        for i, (fi, fo) in enumerate(zip(dims[:-1], dims[1:])):
            W = p[k:k + fi * fo].reshape(fo, fi)
            b = p[k + fi * fo:k + fi * fo + fo]
            k += fi * fo + fo
            h = h @ W.T + b
            if i + 2 < len(dims):
                h = fn(h)
        return torch.log_softmax(h, dim=1)

    p = torch.tensor(np.asarray(params, dtype=np.float64), requires_grad=True)
    lp = log_probs(p)
    with torch.no_grad():
        lp0 = lp.detach() if params0 is None else log_probs(torch.tensor(np.asarray(params0, dtype=np.float64)))
    ratio = torch.exp(lp.gather(1, at)[:, 0] - lp0.gather(1, at)[:, 0])
    if clip is None:
        loss = -(ratio * advt).mean()
    else:
        loss = -torch.minimum(ratio * advt, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * advt).mean()
    kl = (lp0.exp() * (lp0 - lp)).sum(dim=1).mean()
    out = {"loss": loss.item(), "kl": kl.item(), "entropy": -(lp.exp() * lp).sum(dim=1).mean().item()}
    out["grad"] = torch.autograd.grad(loss, p, retain_graph=True)[0].numpy().copy()
    if vec is not None:
        gk = torch.autograd.grad(kl, p, create_graph=True)[0]
        out["fvp"] = torch.autograd.grad((gk * torch.tensor(np.asarray(vec, dtype=np.float64))).sum(), p)[0].numpy().copy()
    return out


def oracle_history(engine, A, L, hidden, act, n, T, seed):
    """a trajectory rolled out by the oracle's lanes (one hidden layer) or by the device (other shapes), loaded into a
    device trajectory with drawn advantages"""
    D = A + L
    pol = make(engine, D, hidden, A, seed, act)
    traj = ra.Trajectory(engine, n, T, D)
    if len(hidden) == 1 and act == "Relu":
        h = O.MemoryLaneSim(n, A, L, seed_env=seed + 1, seed_actor=seed + 2).rollout_mlp(
            O.MlpShape(D, hidden[0], A), pol.get_params(), T)
        traj.write_all(h)
    else:
        ra.rollout(ra.MemoryEnv(engine, n, A, L, seed_env=seed + 1, seed_actor=seed + 2), pol, traj)
        h = traj.read_all()
    adv = np.random.default_rng(seed).normal(size=(T, n)).astype(np.float32)
    traj.write(ra.TRAJ_ADVANTAGES, adv)
    x, a = O.flat_samples(h)
    assert sorted(np.unique(a)) == list(range(A))
    return pol, traj, x, a, adv.reshape(-1)


def close(got, want, rel, floor=1e-9):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, bound = np.abs(got - want).max(), rel * np.abs(want).max() + floor
    print("max error %.3e, bound %.3e" % (err, bound))
    return err <= bound


@pytest.mark.parametrize("A,L,hidden,act", [(a, l, [32], "Relu") for a, l in SIZES] + [(4, 3, [16, 16], "Tanh")])
def test_gradient_fisher_vector_product_loss_and_kl(engine, A, L, hidden, act):
    n, T, D = 160, 11, A + L
    pol, traj, x, a, adv = oracle_history(engine, A, L, hidden, act, n, T, 31)
    p0 = pol.get_params()
    vec = np.random.default_rng(5).normal(size=pol.P).astype(np.float32)
    ref = torch_restatement(p0, D, hidden, A, act, x, a, adv, vec)
    if len(hidden) == 1:  # the oracle's f64 functions take one hidden layer
        shape = O.MlpShape(D, hidden[0], A)
        g64, loss64 = O.grad_f64_mt("policy", shape, p0, x, a, adv)
        f64, _ = O.grad_f64_mt("fvp", shape, p0, x, a, None, vec)
        assert close(g64, ref["grad"], 1e-12, 1e-15) and close(f64, ref["fvp"], 1e-12, 1e-15)  # the two yardsticks agree
        assert abs(loss64 - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
        want_g, want_f, want_loss = g64, f64, loss64
    else:
        want_g, want_f, want_loss = ref["grad"], ref["fvp"], ref["loss"]
    got_g, loss, ent = ra.policy_gradient(pol, traj)
    assert close(got_g, want_g, 2e-5)
    assert abs(loss - want_loss) <= 2e-5 * abs(want_loss) + 1e-7
    assert abs(ent - ref["entropy"]) <= 2e-5 * abs(ref["entropy"]) + 1e-7
    assert close(ra.policy_fvp(pol, traj, vec, 0.0), want_f, 5e-5)
    assert close(ra.policy_fvp(pol, traj, vec, 1e-5), want_f + 1e-5 * vec.astype(np.float64), 5e-5)
    # loss and KL of moved parameters against the old ones (the line search's evaluation)
    moved = (p0 + 0.01 * vec).astype(np.float32)
    pol.set_params(moved)
    loss1, kl1 = ra.policy_loss_kl(pol, traj, p0)
    ref1 = torch_restatement(moved, D, hidden, A, act, x, a, adv, params0=p0)
    assert abs(loss1 - ref1["loss"]) <= 2e-5 * abs(ref1["loss"]) + 1e-7
    assert abs(kl1 - ref1["kl"]) <= 2e-4 * abs(ref1["kl"]) + 1e-8
    pol.set_params(p0)
    assert ra.policy_loss_kl(pol, traj, p0)[1] == 0.0


# ------------------------------------------------------------------------------------------------ 4. update steps
def oracle_trpo_cfg(dcfg):
    cfg = O.TrpoCfg()
    O.lib().oracle_trpo_cfg_default(C.byref(cfg))
    cfg.iterations, cfg.max_backtracks = dcfg.iterations, dcfg.max_backtracks
    cfg.backtrack_ratio, cfg.hpv_reg_coeff = dcfg.backtrack_ratio, dcfg.hpv_reg_coeff
    cfg.max_kl, cfg.accept_violation = dcfg.max_policy_step_kl, dcfg.accept_violation
    return cfg


@pytest.mark.parametrize("iterations,tol", [(1, 3e-4), (2, 2e-3)])  # tests/test_gpu_parity.py's tight TRPO parity
@pytest.mark.parametrize("A,L", [(3, 4), (7, 1)])
def test_trpo_update_against_the_f32_oracle(engine, A, L, iterations, tol):
    n, T, D = 256, 12, A + L
    pol, traj, x, a, adv = oracle_history(engine, A, L, [32], "Relu", n, T, 41)
    p0 = pol.get_params()
    dcfg = ra.trpo_config_default()
    dcfg.iterations = iterations
    st_d = ra.trpo_update(pol, traj, dcfg)
    p_d = pol.get_params()
    p_o, st_o, _ = O.trpo_update(O.MlpShape(D, 32, A), p0, x, a, adv, oracle_trpo_cfg(dcfg))
    print(st_d.as_dict(), st_o.status, st_o.num_backtracks, st_o.cg_iterations, st_o.step_size)
    assert st_d.status == st_o.status == ra.OPT_OK
    assert st_d.num_backtracks == st_o.num_backtracks
    assert st_d.cg_iterations == st_o.cg_iterations == iterations
    assert abs(st_d.entropy - st_o.entropy) < 1e-5
    assert abs(st_d.loss_initial - st_o.loss_initial) <= 1e-5 * max(1.0, abs(st_o.loss_initial))
    assert abs(st_d.step_size - st_o.step_size) <= tol * st_o.step_size
    assert abs(st_d.loss_final - st_o.loss_final) <= 1e-5 * max(1.0, abs(st_o.loss_final))
    assert np.abs(p_d - p_o).max() <= tol * np.abs(p_o - p0).max() + 1e-7


@pytest.mark.parametrize("rule", ["ppo", "reinforce"])
@pytest.mark.parametrize("A,L,hidden,act", [(3, 4, [32], "Relu"), (4, 3, [16, 16], "Tanh")])
def test_one_first_order_step_against_the_restatement(engine, rule, A, L, hidden, act):
    """One Adam step from zero moments moves entry i by -lr g_i / (|g_i| + eps'): where the gradient entry is larger than
    twice the gradient tolerance (2e-5 of the largest entry, the bound of the gradient test above) its sign is certain
    and the step differs by rounding only (1e-6 at lr 1e-2 and parameters below 1); any other entry moves by at most lr
    either way."""
    from optim_ref import adamw_step
    n, T, D = 160, 11, A + L
    pol, traj, x, a, adv = oracle_history(engine, A, L, hidden, act, n, T, 51)
    p0 = pol.get_params()
    acfg = ra.adam_config_default()
    acfg.learning_rate = 1e-2
    opt = ra.Adam(pol, acfg)
    if rule == "ppo":
        cfg = ra.ppo_config_default()
        cfg.opt_steps_per_update = 1
        st, losses = ra.ppo_update(pol, opt, traj, cfg, want_losses=True)
        ref = torch_restatement(p0, D, hidden, A, act, x, a, adv, clip=cfg.clip_distance)
        assert abs(losses[0] - ref["loss"]) <= 2e-5 * abs(ref["loss"]) + 1e-7
    else:
        st = ra.reinforce_update(pol, opt, traj)
        ref = torch_restatement(p0, D, hidden, A, act, x, a, adv)
    assert abs(st.entropy - ref["entropy"]) <= 2e-5 * abs(ref["entropy"]) + 1e-7
    g = ref["grad"].astype(np.float32)
    want = adamw_step(p0, g, {}, lr=acfg.learning_rate, beta1=acfg.beta1, beta2=acfg.beta2, weight_decay=0.0, eps=acfg.eps)
    got = pol.get_params()
    sure = np.abs(g) > 4e-5 * np.abs(g).max()
    print("entries with a certain sign: %d of %d; max error there %.3e, elsewhere %.3e" % (
        sure.sum(), g.size, np.abs(got - want)[sure].max(), np.abs(got - want)[~sure].max() if (~sure).any() else 0.0))
    assert sure.mean() > 0.5 and np.abs(got - want)[sure].max() <= 1e-6
    assert np.abs(got - want).max() <= 2.0 * acfg.learning_rate * (1.0 + 1e-3)
    assert np.abs(got - p0).max() > 0.5 * acfg.learning_rate


def test_actor_critic_update_over_four_actions(engine):
    """rl_actor_critic_update (and _begin / _finish) on a 4-action policy equal the two updates in turn, bit for bit"""
    A, L, n, T = 4, 4, 256, 15
    D = A + L
    out = []
    for mode in ("separate", "combined", "pipelined"):
        env = ra.MemoryEnv(engine, n, A, L, seed_env=1, seed_actor=2)
        pol, cri = make(engine, D, [32], A, 61), make(engine, D, [32], 1, 62)
        opt = ra.Adam(cri)
        ccfg = ra.values_opt_config_default()
        ccfg.opt_steps_per_update = 3
        traj = ra.Trajectory(engine, n, T, D)
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.95)
        if mode == "separate":
            pst = ra.trpo_update(pol, traj)
            ra.values_opt_update(cri, opt, traj, ccfg)
        elif mode == "combined":
            pst, _ = ra.actor_critic_update(pol, cri, opt, traj, None, ccfg)
        else:
            pst = ra.actor_critic_update_begin(pol, cri, opt, traj, None, ccfg)
            ra.actor_critic_update_finish(traj)
        assert pst.status == ra.OPT_OK and pst.loss_final < pst.loss_initial and 0 < pst.constraint_val_final <= 0.01
        out.append((pol.get_params(), cri.get_params()))
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0]) and np.array_equal(out[0][1], other[1])


def test_two_loopback_ranks_sum_the_gradient_of_a_five_action_policy(engine):
    """the all-reduce of the policy passes follows P: two ranks of half the lanes each give the gradient and the
    Fisher-vector product of all lanes (sums of per-rank partial sums: f32 tolerance, not bit for bit)"""
    import threading
    A, L, n, T = 5, 3, 128, 9
    D = A + L
    pol, traj, x, a, adv = oracle_history(engine, A, L, [32], "Relu", n, T, 71)
    p0 = pol.get_params()
    vec = np.random.default_rng(6).normal(size=pol.P).astype(np.float32)
    want_g, want_f = ra.policy_gradient(pol, traj)[0], ra.policy_fvp(pol, traj, vec, 0.0)
    whole = traj.read_all()
    import os
    os.environ["RELEARN_LOOPBACK_COMM"] = "1"
    res, errs = [None, None], []
    try:
        uid = ra.comm_unique_id()

        def rank(r):
            try:
                eng = ra.Engine(0)
                eng.comm_init(r, 2, uid)
                m = ra.Mlp(eng, D, [32], A)
                m.set_params(p0)
                half = slice(r * (n // 2), (r + 1) * (n // 2))
                t = ra.Trajectory(eng, n // 2, T, D)
                t.write_all({k: np.ascontiguousarray(v[..., half]) for k, v in whole.items()})
                t.write(ra.TRAJ_ADVANTAGES, np.ascontiguousarray(adv.reshape(T, n)[:, half]))
                res[r] = (ra.policy_gradient(m, t)[0], ra.policy_fvp(m, t, vec, 0.0))
                eng.comm_destroy()
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        threads = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
    finally:
        del os.environ["RELEARN_LOOPBACK_COMM"]
    assert not errs, errs
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert close(res[0][0], want_g, 2e-5) and close(res[0][1], want_f, 5e-5)


# ------------------------------------------------------------------------------------------------ 5. k-armed bandits
@pytest.mark.parametrize("values", [(0.25, -1.0, 1.5), (0.0, 0.0, 0.0, 1.0), tuple(float(i) for i in range(8))])
def test_bandit_lanes_bit_exact(engine, values):
    n, T, A = 128, 6, len(values)
    env = ra.BanditEnv(engine, n, values=values, seed_env=5, seed_actor=6)
    assert (env.D, env.A) == (5, A)
    one_hot = np.zeros((5, n), dtype=np.float32)
    one_hot[0] = 1.0
    assert np.array_equal(env.observe(), one_hot)
    rng = np.random.default_rng(0)
    v32 = np.asarray(values, dtype=np.float32)
    for _ in range(3):
        act = rng.integers(0, A, n).astype(np.uint8)
        reward, flag, obs, _ = env.step(act)
        assert np.array_equal(reward, v32[act]) and (flag == O.TERMINATE).all() and np.array_equal(obs, one_hot)
    pol = make(engine, 5, [32], A, 3)
    traj = ra.Trajectory(engine, n, T, 5)
    ra.rollout(env, pol, traj)
    got = traj.read_all()
    assert sorted(np.unique(got["action"])) == list(range(A))
    assert np.array_equal(got["reward"], v32[got["action"]]) and (got["flag"] == O.TERMINATE).all()
    assert np.array_equal(got["obs"], np.broadcast_to(one_hot[:, None, :], (5, T + 1, n)))


def adam(module, lr):
    cfg = ra.adam_config_default()
    cfg.learning_rate = lr
    return ra.Adam(module, cfg)


def train_deterministic_bandit(engine, values, policy_rule, n=32, num_periods=10, threshold=0.9):
    """`train_deterministic_bandit` (src/agents/testing.rs:14-64) as tests/test_gpu_bandit.py runs it, on `values`"""
    A, best = len(values), int(np.argmax(values))
    env = ra.BanditEnv(engine, n, values=values, seed_env=18, seed_actor=19)
    pol = ra.Mlp(engine, 5, 128, A)
    pol.init(19)
    popt = adam(pol, 0.1) if policy_rule != "trpo" else None
    ppo = ra.ppo_config_default()
    ppo.opt_steps_per_update = 1
    traj = ra.Trajectory(engine, n, 1, 5)
    for _ in range(num_periods):
        ra.rollout(env, pol, traj)
        ra.reward_to_go(traj, 1.0)  # RewardToGo with the env's own discount factor (bandits.rs:52-54)
        if policy_rule == "trpo":
            ra.trpo_update(pol, traj)
        elif policy_rule == "ppo":
            ra.ppo_update(pol, popt, traj, ppo)
        else:
            ra.reinforce_update(pol, popt, traj)
    ev = ra.Trajectory(engine, n, (1000 + n - 1) // n, 5)
    ra.rollout(env, pol, ev)
    actions = ev.read(ra.TRAJ_ACTION).reshape(-1)[:1000]
    print("best arm in %d of 1000 evaluation steps after %d periods" % ((actions == best).sum(), num_periods))
    assert (actions == best).sum() >= int(1000 * threshold), ((actions == best).sum(), values, policy_rule)


@pytest.mark.parametrize("values", [(0.0, 0.0, 0.0, 1.0), (0.0,) * 7 + (1.0,)])
@pytest.mark.parametrize("policy_rule", ["reinforce", "ppo"])
def test_learns_k_armed_deterministic_bandit(engine, values, policy_rule):
    train_deterministic_bandit(engine, values, policy_rule)


@pytest.mark.parametrize("values", [(0.0, 0.0, 0.0, 1.0), (0.0,) * 7 + (1.0,)])
def test_trpo_learns_k_armed_deterministic_bandit(engine, values):
    """A step of KL <= max_kl moves at most sqrt(2 max_kl) in Fisher-Rao distance; from the uniform policy to 0.9 on one
    arm it is d = 2 acos(sum sqrt(p_i q_i)) (1.45 at four arms), so the reference's 10 periods cannot suffice:
    periods = 2 ceil(d / sqrt(2 max_kl)), the factor 2 for backtracked steps; 1,024 lanes, so that the sampled gradient
    is close to the exact one."""
    k, max_kl = len(values), ra.trpo_config_default().max_policy_step_kl
    q = np.full(k, 0.1 / (k - 1))
    q[int(np.argmax(values))] = 0.9
    d = 2.0 * math.acos(np.sqrt(q / k).sum())
    periods = 2 * math.ceil(d / math.sqrt(2.0 * max_kl))
    print("Fisher-Rao distance %.3f, %d periods" % (d, periods))
    train_deterministic_bandit(engine, values, "trpo", n=1024, num_periods=periods)


# ------------------------------------------------------------------------------------------------ 6. guards
def code_of(fn):
    with pytest.raises(ra.RelearnError) as e:
        fn()
    return e.value.code


def test_guards(engine):
    n = 64
    env3 = ra.MemoryEnv(engine, n, 3, 2)  # five features, three actions
    env2 = ra.MemoryEnv(engine, n, 2, 3)  # five features, two actions
    pol2, pol3, pol4 = make(engine, 5, [32], 2, 1), make(engine, 5, [32], 3, 1), make(engine, 5, [32], 4, 1)
    traj = ra.Trajectory(engine, n, 6, 5)
    # a policy of another action count than the env's / than the env's the trajectory was collected on
    assert code_of(lambda: ra.rollout(env3, pol2, traj)) == ra.ERR_INVALID_ARGUMENT
    assert code_of(lambda: ra.rollout(env3, pol4, traj)) == ra.ERR_INVALID_ARGUMENT
    assert code_of(lambda: ra.rollout(env2, pol3, traj)) == ra.ERR_INVALID_ARGUMENT
    ra.rollout(env3, pol3, traj)
    traj.write(ra.TRAJ_ADVANTAGES, np.ones((6, n), dtype=np.float32))
    vec = np.ones(pol2.P, dtype=np.float32)
    for bad, v in ((pol2, vec), (pol4, np.ones(pol4.P, dtype=np.float32))):
        assert code_of(lambda: ra.policy_gradient(bad, traj)) == ra.ERR_INVALID_ARGUMENT
        assert code_of(lambda: ra.policy_fvp(bad, traj, v, 0.0)) == ra.ERR_INVALID_ARGUMENT
        assert code_of(lambda: ra.policy_loss_kl(bad, traj, bad.get_params())) == ra.ERR_INVALID_ARGUMENT
        assert code_of(lambda: ra.trpo_update(bad, traj)) == ra.ERR_INVALID_ARGUMENT
        assert code_of(lambda: ra.ppo_update(bad, ra.Adam(bad), traj)) == ra.ERR_INVALID_ARGUMENT
        assert code_of(lambda: ra.reinforce_update(bad, ra.Adam(bad), traj)) == ra.ERR_INVALID_ARGUMENT
    cri = make(engine, 5, [32], 1, 2)
    assert code_of(lambda: ra.actor_critic_update(pol2, cri, ra.Adam(cri), traj)) == ra.ERR_INVALID_ARGUMENT
    # host-written actions: the policy must have an output for the largest index
    traj.write(ra.TRAJ_ACTION, np.full((6, n), 2, dtype=np.uint8))
    assert code_of(lambda: ra.policy_gradient(pol2, traj)) == ra.ERR_INVALID_ARGUMENT
    ra.policy_gradient(pol3, traj)
    ra.policy_gradient(pol4, traj)
    # DQN over more than two actions is not built
    q3 = make(engine, 5, [32], 3, 3)
    assert code_of(lambda: ra.Dqn(env3, q3, ra.Adam(q3), ra.dqn_config_default())) == ra.ERR_UNSUPPORTED
    # recurrent chains stay at {1, 2} outputs and refuse envs of more actions
    assert code_of(lambda: ra.GruMlp(engine, 5, 3)) == ra.ERR_BUILD_AGENT
    assert code_of(lambda: ra.LstmMlp(engine, 5, 4)) == ra.ERR_BUILD_AGENT
    gru = ra.GruMlp(engine, 5, 2)
    gru.init(1)
    assert code_of(lambda: ra.rollout(env3, gru, traj)) == ra.ERR_UNSUPPORTED
    # action indices outside the env's space
    acts = np.zeros(n, dtype=np.uint8)
    acts[5] = 3
    assert code_of(lambda: env3.step(acts)) == ra.ERR_INVALID_ARGUMENT
    assert code_of(lambda: env3.upload_actions(acts)) == ra.ERR_INVALID_ARGUMENT
    acts[5] = 2
    env3.step(acts)
    env3.upload_actions(acts)
    # sizes
    for A, L, kw in ((2, 7, {}), (2, 1, {}), (1, 3, {}), (3, 0, {}), (9, 1, {}), (4, 4, dict(max_steps=5, limit=ra.LIMIT_VISIBLE))):
        assert code_of(lambda: ra.MemoryEnv(engine, n, A, L, **kw)) == ra.ERR_BUILD_ENV, (A, L)
    assert code_of(lambda: ra.BanditEnv(engine, n, values=(1.0,))) == ra.ERR_BUILD_ENV
    assert code_of(lambda: ra.BanditEnv(engine, n, values=(0.0,) * 9)) == ra.ERR_BUILD_ENV
    h = C.c_void_p()
    assert ra.lib().rl_mlp_create(engine.h, C.c_uint32(5), C.c_uint32(32), C.c_uint32(3), C.byref(h)) == ra.ERR_BUILD_AGENT
    for out_dim in (0, 9):
        assert code_of(lambda: ra.Mlp(engine, 5, [32], out_dim)) == ra.ERR_BUILD_AGENT
    assert "rl_env_create_bandit" in ra.ABI_SYMBOLS and ra.lib().rl_abi_version() == 6


# ------------------------------------------------------------------------------------------------ 7. documents
def tensor(arr):
    return {"kind": "Float", "shape": list(arr.shape), "requires_grad": True, "byte_order": "LittleEndian",
            "data": np.ascontiguousarray(arr, dtype="<f4").tobytes()}


def test_actor_document_of_a_four_action_policy(engine):
    """PolicyActor { observation_space: NonEmptyFeatures<IndexSpace>, action_space: IndexSpace, policy_module: Mlp }
    of MemoryGame::new(4, 3) (memory.rs:58-68): byte-identical to the independent encoder's document, and it loads back"""
    from cbor_ref import decode, encode
    A, L = 4, 3
    D = A + L
    env = ra.MemoryEnv(engine, 64, A, L)
    pol = make(engine, D, [24, 12], A, 5, "Tanh")
    p = pol.get_params()
    layers, k = [], 0
    for fi, fo in ((D, 24), (24, 12), (12, A)):
        layers.append({"kernel": tensor(p[k:k + fi * fo].reshape(fo, fi)), "bias": tensor(p[k + fi * fo:k + fi * fo + fo])})
        k += fi * fo + fo
    want = {"observation_space": {"inner": {"size": D}}, "action_space": {"size": A},
            "policy_module": {"layers": layers, "activation": "Tanh", "output_activation": "Identity"}}
    data = bytes(ra.actor_to_cbor(env, pol))
    assert decode(data) == want and data == encode(want)
    twin = ra.Mlp(engine, D, [24, 12], A, "Tanh")
    ra.module_from_cbor(twin, data)
    assert np.array_equal(twin.get_params(), p)
    other = ra.Mlp(engine, D, [24, 12], 3, "Tanh")
    with pytest.raises(ra.RelearnError):  # a document of four outputs is not a three-output module's
        ra.module_from_cbor(other, data)
    bandit = ra.BanditEnv(engine, 64, values=(0.0, 0.0, 1.0))
    doc = decode(bytes(ra.actor_to_cbor(bandit, make(engine, 5, [16], 3, 1))))
    assert doc["action_space"] == {"size": 3} and doc["observation_space"] == {"inner": {"size": 5}}
    assert ra.indexed_type_space_to_cbor() == encode({})
