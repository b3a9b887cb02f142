"""DQN over 3 to 8 actions (rl_dqn_create_finite / ra.FiniteDqn) through the C ABI, feed-forward and recurrent
action-value modules: collection bit for bit — every ring plane, the second record array, flags, actor positions and env
state against the restated lanes stepped with the recorded actions, every action against the restated DqnActor of
tests/finite_dqn_ref.py (gen_range(0..A) on an exploring step, the first maximal of A outputs on a greedy one; a recurrent
module's state held over an exploring step), the ring words against tests/dqn_ring_ref.py — then minibatches, both
targets, gradient and loss against f64, the SGD step, the all-or-nothing update, the identity with the two older
constructors at two actions, the refusals, the actor document, and the reference's own acceptance test
(src/agents/testing.rs:14-64: train_deterministic_bandit) at four and eight arms.

Every test constructs ra.FiniteDqn at more than two actions.  The cases and the reason for their shapes:
tests/finite_dqn_cases.py; tests/test_finite_dqn_cases.py holds the conditions that let every step be compared.  The bars
are those of tests/test_gpu_dqn_index_envs.py and tests/test_gpu_recurrent_dqn.py."""
import os
import threading

import numpy as np
import pytest

import finite_dqn_cases as FC
import finite_dqn_ref as F
import oracle as O
from dqn_ring_ref import RingStore
from oracle import stacked as S
from steps_summary_ref import close, period_summaries

pytestmark = pytest.mark.gpu

ra = pytest.importorskip("relearn_amd")

from test_gpu_dqn_index_envs import dqn_cfg, last_collection  # noqa: E402
from test_gpu_stacked import GRAD_RTOL, rel_err  # noqa: E402  (the bar the recurrent gradients are held to)


def device_env(engine, name, n, lane_offset=0):
    e = FC.ENVS[name]
    if e.kind == "bandit":
        env = ra.BanditEnv(engine, n, e.values, lane_offset=lane_offset, **FC.SEEDS)
    elif e.limit:
        env = ra.MemoryEnv(engine, n, e.k, e.h, max_steps=e.limit, limit=ra.LIMIT_VISIBLE, lane_offset=lane_offset,
                           **FC.SEEDS)
    else:
        env = ra.MemoryEnv(engine, n, e.k, e.h, lane_offset=lane_offset, **FC.SEEDS)
    assert (env.D, env.A) == (e.D, e.A)
    return env


def device_module(engine, case):
    e = FC.ENVS[case.env]
    if FC.is_recurrent(case):
        m = F.module_of(case)
        q = ra.RnnChain(engine, m.cell, e.D, m.H, e.A, num_layers=m.L, bias=m.bias, mlp_hidden=m.H2)
        q.init_with(case.seed, bias=F.R.BIAS_INIT)
    else:
        hidden, act = FC.FF_MODULES[case.module]
        q = ra.Mlp(engine, e.D, hidden, e.A, act, "Identity")
        q.init(case.seed)
    assert np.array_equal(q.get_params(), F.case_params(case))
    return q


def make(engine, case, opt=None, **kw):
    env, sim = device_env(engine, case.env, case.n), F.make_sim(case.env, case.n)
    F.warm_up(case.env, sim, env)
    q = device_module(engine, case)
    kw.setdefault("gamma", FC.ENVS[case.env].gamma)
    kw.setdefault("capacity", FC.CAPACITY)
    dqn = ra.FiniteDqn(env, q, opt(q) if opt else ra.Adam(q), dqn_cfg(**kw))
    return dqn, sim, q


def check_collection(dqn, sim, actor, T, eps, store):
    """one collection: the env side against the restated lanes stepped with the recorded actions, every action against the
    restated actor, no step left out; the planes go into the restated ring, which is then compared word for word.
    -> (explored, greedy, horizon cuts, the least top-two gap of the greedy steps)"""
    n = dqn.n
    rec = last_collection(dqn, T)
    actor.begin_collection()
    cur, explored, cuts, margin = sim.observe(), 0, 0, np.inf
    flags, succs = [], []
    for t in range(T):
        assert np.array_equal(rec["obs"][t], cur), t
        want_a, explore, gap = actor.act(cur, eps)
        margin = min(margin, gap)
        assert np.array_equal(rec["action"][t], want_a), (t, np.flatnonzero(rec["action"][t] != want_a)[:8])
        explored += int(explore.sum())
        reward, fl, nxt, term = sim.step(rec["action"][t])
        actor.end_step(fl)
        want_flag, succ = fl.copy(), term
        if t == T - 1:  # the horizon rule: the open episode closes as Interrupt(successor) and the env carries on
            cut = fl == O.CONTINUE
            want_flag[cut] = O.INTERRUPT
            succ = np.where(cut[None], nxt, term)
            cuts = int(cut.sum())
        assert np.array_equal(rec["flag"][t], want_flag), t
        assert np.array_equal(rec["reward"][t], reward), t
        m = want_flag == O.INTERRUPT
        assert np.array_equal(rec["next"][t][:, m], succ[:, m]), t
        flags.append(want_flag)
        succs.append(succ)
        cur = nxt
    assert np.array_equal(dqn.replay_read(ra.REPLAY_LAST_FLAGS), rec["flag"])
    assert np.array_equal(dqn.replay_read(ra.REPLAY_ACTOR_POS), actor.positions())
    for a, b in zip(dqn.env.get_state(), sim.get_state()):
        assert np.array_equal(a, b)
    store.write_collection(rec["obs"], rec["action"], rec["reward"], np.array(flags), np.array(succs))
    store.check_device(dqn, ra)
    return explored, n * T - explored, cuts, margin


@pytest.mark.parametrize("eps", FC.EPSILONS)
@pytest.mark.parametrize("case", FC.COLLECT_CASES, ids=FC.case_id)
def test_collection_bit_exact(engine, case, eps):
    """two collections of 9 and 7 steps: the first cuts every MemoryGame lane mid-episode, the episode continues into the
    second, a recurrent state restarts at a collection's first step.  k_dqn_lane_step<IndexOps, D, 64, A> behind the
    per-layer kernels, k_stack_collect_dqn<CELL, IndexOps, D, LIN, A> for the recurrent chains."""
    e = FC.ENVS[case.env]
    dqn, sim, q = make(engine, case, eps=eps)
    params = q.get_params()
    actor = F.FiniteActor(case, params)
    store = RingStore(dqn.n, FC.CAPACITY, dqn.D)
    counts, taken = np.zeros(2, dtype=np.int64), np.zeros(e.A, dtype=np.int64)
    summary, rewards, flags = ra.StepsSummary(engine, dqn.n), [], []
    for k, T in enumerate(FC.HORIZONS):
        st = dqn.collect(T)
        summary.push_dqn(dqn)  # rl_summary_push_dqn takes the handle: the period's StepsSummary against numpy
        got = summary.read()
        summary.clear()
        explored, greedy, cuts, margin = check_collection(dqn, sim, actor, T, eps, store)
        counts += (explored, greedy)
        assert margin >= FC.MARGIN  # (on the device's own parameters, at what occurred)
        assert st.steps == T * dqn.n
        if k == 0:  # the first collection ends mid-episode on every MemoryGame lane
            assert cuts == (dqn.n if e.kind == "memory" else 0)
        rec = last_collection(dqn, T)
        taken += np.bincount(rec["action"].ravel(), minlength=e.A)
        rewards.append(rec["reward"])
        flags.append(rec["flag"])
        want = period_summaries(rewards, flags)[-1]
        for f in ("step_reward", "episode_reward", "episode_length"):
            close(getattr(got, f), want[f], f)
    assert np.array_equal(dqn.replay_read(ra.REPLAY_TOTAL), np.full(dqn.n, sum(FC.HORIZONS), dtype=np.uint32))
    assert np.array_equal(q.get_params(), params)
    if eps == 1.0:
        assert counts[1] == 0 and taken.min() > 0  # every action index was drawn
    elif eps == 0.0:
        assert counts[0] == 0
    else:
        assert counts.min() > 0.3 * dqn.n * sum(FC.HORIZONS) and taken.min() > 0
    dqn.close()


# ---------------------------------------------------------------- minibatches
def filled(engine, case, td, minibatch=300, opt_steps=3, opt=None):
    """an agent after the 9 + 7 collections at eps = 0.5, and the restated ring of its store"""
    dqn, sim, q = make(engine, case, eps=0.5, minibatch=minibatch, opt_steps=opt_steps, td=td, opt=opt)
    actor = F.FiniteActor(case, q.get_params())
    store = RingStore(dqn.n, FC.CAPACITY, dqn.D)
    for T in FC.HORIZONS:
        dqn.collect(T)
        check_collection(dqn, sim, actor, T, 0.5, store)
    return dqn, q, store


@pytest.mark.parametrize("td", [False, True], ids=["reward-to-go", "one-step-td"])
@pytest.mark.parametrize("case", FC.MINIBATCH_CASES, ids=FC.case_id)
def test_minibatch_targets_and_gradient(engine, case, td):
    """the sampled episodes exist in the restated ring; the gathered observations and actions are the stored ones bit for
    bit; reward-to-go and one-step TD targets (amax over A values, 0 beyond a Terminate, the stored successor after an
    Interrupt) against f64 at rtol = atol = 2e-5; gradient and loss against f64 — forward64 / backward64 for the
    feed-forward modules, oracle/stacked.py on the padded layout for the recurrent ones; then an update"""
    from test_gpu_general_mlp import backward64, forward64, unflatten
    e = FC.ENVS[case.env]
    recurrent = FC.is_recurrent(case)
    dqn, q, store = filled(engine, case, td)
    gamma = dqn.cfg.discount_factor
    ne, ns = dqn.minibatch_sample()
    obs, a, tgt = dqn.minibatch_read(ra.MB_OBS), dqn.minibatch_read(ra.MB_ACTION), dqn.minibatch_read(ra.MB_TARGET)
    lanes, starts, lens = (dqn.minibatch_read(f) for f in (ra.MB_EP_LANE, ra.MB_EP_START, ra.MB_EP_LEN))
    assert ne == len(lanes) and ns == int(lens.sum()) and 300 <= ns < 300 + FC.CAPACITY
    if recurrent:
        m = F.module_of(case)
        _, spec, full, index = F.embedded(m, e.D, e.A, q.get_params())
    else:
        hidden, act = FC.FF_MODULES[case.module]
        net = unflatten(q.get_params(), e.D, hidden, e.A)
    want_t, k, episodes, kinds = np.zeros(ns), 0, [], set()
    for ln, st, le in zip(lanes, starts, lens):
        le = int(le)
        ring = store.rings[ln]
        assert (int(st), le) in [ring.episode(x) for x in range(ring.num_episodes())], (ln, st, le)
        steps = [store.step_data(int(ln), int(st) + j) for j in range(le)]
        o = np.array([s[0] for s in steps], dtype=np.float32)
        act_e = np.array([s[1] for s in steps], dtype=np.uint8)
        r = np.array([s[2] for s in steps], dtype=np.float64)
        fl = np.array([s[3] for s in steps])
        succ = np.array([s[4] for s in steps], dtype=np.float32)
        assert np.array_equal(obs[:, k:k + le], o.T) and np.array_equal(a[k:k + le], act_e)
        assert fl[-1] != O.CONTINUE and np.all(fl[:-1] == O.CONTINUE)
        kinds.add(int(fl[-1]))
        if not td:
            want_t[k:k + le] = F.reward_to_go(r, gamma)
            if e.kind == "bandit":
                assert np.array_equal(tgt[k:k + le], r.astype(np.float32))  # bit-exactly the rewards
        elif recurrent:
            _, v = F.recurrent_episode_values(spec, full, o, fl, succ)
            want_t[k:k + le] = F.td_targets(v, r, fl, gamma)
        else:
            nxt = np.array([succ[j] if fl[j] == O.INTERRUPT or j == le - 1 else o[j + 1] for j in range(le)])
            zn, _ = forward64(net, nxt, act, "Identity")
            want_t[k:k + le] = F.td_targets(zn.max(axis=1), r, fl, gamma)
        episodes.append((o, act_e, fl))
        k += le
    print("%s td=%s: targets vs f64 %.3g" % (FC.case_id(case), td, np.abs(tgt - want_t).max()))
    assert k == ns and np.allclose(tgt, want_t, rtol=2e-5, atol=2e-5)
    assert len(np.unique(a)) == e.A  # every action index is in the minibatch
    if e.kind == "memory":  # Terminates (0 beyond them) and Interrupts (the stored successor) are both sampled
        assert kinds == ({O.INTERRUPT} if e.limit else {O.TERMINATE, O.INTERRUPT})
    g_d, loss_d = dqn.minibatch_gradient()
    if recurrent:
        T, n = int(lens.max()), len(lens)
        traj = dict(obs=np.zeros((e.D, T + 1, n)), flag=np.full((T, n), O.TERMINATE, dtype=np.uint8))
        for x, (o, _, fl) in enumerate(episodes):
            traj["obs"][:, :len(o), x] = o.T
            traj["flag"][:len(o), x] = fl
        qv, _, _ = S.forward(spec, full, traj, want_succ=False)
        dz, loss64, k = np.zeros((e.A, T, n)), 0.0, 0
        for x, (o, act_e, _) in enumerate(episodes):
            for t in range(len(o)):
                d = qv[act_e[t], t, x] - float(tgt[k])
                dz[act_e[t], t, x] = 2.0 * d / ns
                loss64 += d * d / ns
                k += 1
        g64 = S.backward(spec, full, traj, dz)[index]
        print("%s td=%s: gradient vs f64 %.3g (bar %.3g), loss %.9g vs %.9g" % (FC.case_id(case), td, rel_err(g_d, g64),
                                                                                 GRAD_RTOL, loss_d, loss64))
        assert g_d.shape == g64.shape and np.abs(g64).max() > 0
        assert rel_err(g_d, g64) < GRAD_RTOL
        assert abs(loss_d - loss64) <= 1e-5 * loss64
    else:
        z, acts = forward64(net, obs.T, act, "Identity")
        qa = z[np.arange(ns), a]
        want_loss = ((qa - tgt) ** 2).mean()
        dz = np.zeros_like(z)
        dz[np.arange(ns), a] = 2.0 * (qa - tgt.astype(np.float64)) / ns
        want_g = backward64(net, obs.T, acts, dz)
        print("%s td=%s: gradient vs f64 %.3g of max, loss %.9g vs %.9g" % (
            FC.case_id(case), td, np.abs(g_d - want_g).max() / np.abs(want_g).max(), loss_d, want_loss))
        assert np.abs(g_d - want_g).max() <= 2e-5 * np.abs(want_g).max() + 1e-9
        assert abs(loss_d - want_loss) <= 1e-5 * want_loss
    p0 = q.get_params()
    st, losses = dqn.update(want_losses=True)
    assert st.opt_steps == 3 and np.all(np.isfinite(losses)) and not np.array_equal(q.get_params(), p0)
    dqn.close()


def sgd(lr):
    def of(q):
        cfg = ra.optimizer_config_default(ra.OPTIMIZER_SGD)
        assert (cfg.momentum, cfg.weight_decay, cfg.dampening, cfg.nesterov) == (0.0, 0.0, 0.0, 0)
        cfg.learning_rate = lr
        return ra.Optimizer(q, cfg)
    return of


@pytest.mark.parametrize("td", [False, True], ids=["reward-to-go", "one-step-td"])
@pytest.mark.parametrize("case", FC.STEP_CASES, ids=FC.case_id)
def test_sgd_step_is_the_minibatch_gradient(engine, case, td):
    """one optimisation step under plain SGD: (p0 - p1) / lr is rl_dqn_minibatch_gradient's vector of the update's first
    minibatch within the read-back term (tests/test_gpu_recurrent_dqn.py), losses_out[0] that minibatch's loss"""
    lr, ULP = 0.05, 2.0 ** -24
    probe, qp, _ = filled(engine, case, td, opt_steps=1, opt=sgd(lr))
    probe.minibatch_sample()
    g0, loss0 = probe.minibatch_gradient()
    dqn, q, _ = filled(engine, case, td, opt_steps=1, opt=sgd(lr))
    p0 = q.get_params().astype(np.float64)
    assert np.array_equal(q.get_params(), qp.get_params())
    st, losses = dqn.update(want_losses=True)
    p1 = q.get_params().astype(np.float64)
    assert dqn.agent_rng_pos() == probe.agent_rng_pos()  # the same episodes were drawn
    g0 = g0.astype(np.float64)
    assert np.abs(g0).max() > 0
    readback = ULP * (np.abs(p1) + lr * np.abs(g0)) / lr
    diff = np.abs((p0 - p1) / lr - g0)
    print("%s td=%s: worst excess over the read-back term %.3g of max|g|; loss %.9g vs %.9g" % (
        FC.case_id(case), td, np.maximum(diff - readback, 0.0).max() / np.abs(g0).max(), losses[0], loss0))
    assert np.all(diff <= readback)
    assert abs(losses[0] - loss0) <= 2e-6 * abs(loss0) and st.loss_first == losses[0]
    probe.close()
    dqn.close()


def adam(q):
    return ra.Optimizer(q, ra.optimizer_config_default(ra.OPTIMIZER_ADAM))


# (a feed-forward k-action module trains on the per-layer kernels: its update draws in chunks — where the injected failure
# is raised — under reward-to-go targets; one-step TD minibatches are drawn in one launch before the first step)
@pytest.mark.parametrize("case,td", [(FC.STEP_CASES[0], False), (FC.STEP_CASES[1], False), (FC.STEP_CASES[1], True)],
                         ids=["feed-forward-reward-to-go", "recurrent-reward-to-go", "recurrent-one-step-td"])
def test_a_failed_chunk_leaves_the_agent_as_it_was(engine, case, td):
    """RELEARN_DQN_FAIL_CHUNK: parameters, optimiser state, step count and agent_rng_pos come back as an agent's that
    failed before its first step; both then update alike"""
    dqn, q, _ = filled(engine, case, td, minibatch=100, opt_steps=12, opt=adam)
    ref, qr, _ = filled(engine, case, td, minibatch=100, opt_steps=12, opt=adam)
    for agent in (dqn, ref):  # one good update first: the optimiser has state to lose
        agent.update()
    before = q.get_params()
    state = [dqn.opt.state(0), dqn.opt.state(1), dqn.opt.step_count]
    assert state[2] == 12 and np.abs(state[0]).max() > 0 and np.array_equal(before, qr.get_params())
    for agent, chunk in ((dqn, "2"), (ref, "0")):  # (the failed call consumed its draws: the reference agent fails too)
        os.environ["RELEARN_DQN_FAIL_CHUNK"] = chunk
        try:
            with pytest.raises(ra.RelearnError) as err:
                agent.update()
            assert err.value.code == ra.ERR_INVALID_ARGUMENT
        finally:
            os.environ.pop("RELEARN_DQN_FAIL_CHUNK", None)
    assert np.array_equal(q.get_params(), before) and np.array_equal(qr.get_params(), before)
    assert np.array_equal(dqn.opt.state(0), state[0]) and np.array_equal(dqn.opt.state(1), state[1])
    assert dqn.opt.step_count == state[2]
    assert dqn.agent_rng_pos() == ref.agent_rng_pos()
    _, la = dqn.update(want_losses=True)
    _, lb = ref.update(want_losses=True)
    assert np.array_equal(la, lb) and np.array_equal(q.get_params(), qr.get_params())
    assert not np.array_equal(q.get_params(), before) and dqn.opt.step_count == 24
    dqn.close()
    ref.close()


# ---------------------------------------------------------------- two actions: what the older constructors build
REPLAY_FIELDS = ("REPLAY_HEAD", "REPLAY_COUNT", "REPLAY_EP_HEAD", "REPLAY_EP_COUNT", "REPLAY_TOTAL", "REPLAY_EP_END",
                 "REPLAY_OBS", "REPLAY_NEXT_OBS", "REPLAY_ACTION", "REPLAY_REWARD", "REPLAY_FLAG", "REPLAY_ACTOR_POS",
                 "REPLAY_LAST_FLAGS")


@pytest.mark.parametrize("kind", ["fused-128-memory-2-3", "gru-mlp-chain"])
def test_two_actions_build_what_the_older_constructors_build(engine, kind):
    """FiniteDqn beside Dqn (the fused [128] module on MemoryGame(2, 3)) and beside RecurrentDqn (a GRU-MLP on Chain): two
    collections and one update, then every replay field, the losses and the parameters are equal — and a three-action
    FiniteDqn on the same engine, which the older constructor refuses"""
    n = 200
    env3 = device_env(engine, "memory-3-2", 64)
    q3 = ra.Mlp(engine, env3.D, [32], 3)
    q3.init(1)
    with pytest.raises(ra.RelearnError) as err:
        ra.Dqn(env3, q3, ra.Adam(q3), dqn_cfg(16, 0.5))
    assert err.value.code == ra.ERR_UNSUPPORTED
    ra.FiniteDqn(env3, q3, ra.Adam(q3), dqn_cfg(16, 0.5)).close()
    results = []
    for cls in (ra.FiniteDqn, ra.RecurrentDqn if kind == "gru-mlp-chain" else ra.Dqn):
        if kind == "gru-mlp-chain":
            env = ra.ChainEnv(engine, n, max_steps=7, limit=ra.LIMIT_LATENT, **FC.SEEDS)
            q = ra.GruMlp(engine, 5, 2, 8, 8)
        else:
            env = ra.MemoryEnv(engine, n, 2, 3, **FC.SEEDS)
            q = ra.Mlp(engine, 5, 128, 2)
        q.init(77)
        # (a capacity of the 16 collected steps: every step slot has been written when the planes are compared)
        dqn = cls(env, q, ra.Adam(q), dqn_cfg(sum(FC.HORIZONS), 0.5, minibatch=300, opt_steps=4, td=True,
                                              gamma=0.95 if kind == "gru-mlp-chain" else 1.0))
        for T in FC.HORIZONS:
            dqn.collect(T)
        _, losses = dqn.update(want_losses=True)
        fields = {f: dqn.replay_read(getattr(ra, f)) for f in REPLAY_FIELDS}
        # (the episode table's slots are written as episodes end: the stored episodes' entries are compared, the slots no
        # episode has reached yet hold nothing)
        eph, epc, ends = fields["REPLAY_EP_HEAD"], fields["REPLAY_EP_COUNT"], fields.pop("REPLAY_EP_END")
        table = [ends[(int(eph[i]) + k) % dqn.E, i] for i in range(n) for k in range(int(epc[i]))]
        results.append(list(fields.values()) + [np.array(table), losses, q.get_params(), np.array(dqn.agent_rng_pos())])
        dqn.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    assert np.all(np.isfinite(results[0][-3])) and len(results[0][-3]) == 4


# ---------------------------------------------------------------- refusals
def refusal(f):
    with pytest.raises(ra.RelearnError) as e:
        f()
    return e.value.code, str(e.value)


def test_refusals(engine):
    cfg = dqn_cfg(16, 0.5)
    meta = ra.MetaBanditEnv(engine, 64, n_arms=3, episodes_per_trial=3)
    for qm in (ra.Mlp(engine, meta.D, [16], 3), ra.RnnChain(engine, "gru", meta.D, 8, 3, mlp_hidden=8)):
        code, msg = refusal(lambda: ra.FiniteDqn(meta, qm, ra.Adam(qm), cfg))
        assert code == ra.ERR_UNSUPPORTED and "rl_dqn_create_finite" in msg, msg
    meta2 = ra.MetaBanditEnv(engine, 64, n_arms=2, episodes_per_trial=3)
    q2 = ra.Mlp(engine, meta2.D, [16], 2)
    code, msg = refusal(lambda: ra.FiniteDqn(meta2, q2, ra.Adam(q2), cfg))
    assert code == ra.ERR_UNSUPPORTED and "rl_dqn_create_finite" in msg, msg
    env4 = device_env(engine, "bandit-4", 64)
    env3 = device_env(engine, "memory-3-2", 64)
    for env, q in ((env4, ra.Mlp(engine, 5, [16], 3)), (env4, ra.Mlp(engine, 5, [16], 2)), (env4, ra.Mlp(engine, 4, [16], 4)),
                   (env3, ra.RnnChain(engine, "lstm", 5, 8, 4)), (env3, ra.GruMlp(engine, 5, 2, 8, 8))):
        code, msg = refusal(lambda: ra.FiniteDqn(env, q, ra.Adam(q), cfg))
        assert code == ra.ERR_INVALID_ARGUMENT and "rl_dqn_create_finite" in msg, msg
    # what builds: every chain of rl_rnn_chain_create and any feed-forward module of (obs_dim -> n_actions)
    for q in (ra.RnnChain(engine, "gru", 5, 8, 3, mlp_hidden=8), ra.RnnChain(engine, "lstm", 5, 8, 3, num_layers=4),
              ra.RnnChain(engine, "gru", 5, 8, 3, bias=False), ra.Mlp(engine, 5, [], 3), ra.Mlp(engine, 5, [200, 3], 3)):
        q.init(1)
        ra.FiniteDqn(env3, q, ra.Adam(q), cfg).close()


def test_recurrent_update_is_refused_with_two_ranks():
    """a communicator of two ranks (the in-process loopback collective of tests/test_gpu_multirank.py): rl_dqn_update of a
    recurrent three-action agent answers RL_ERR_UNSUPPORTED before anything is changed"""
    def run_rank(rank, uid, out):
        try:
            eng = ra.Engine(0)
            eng.comm_init(rank, 2, uid)
            env = device_env(eng, "memory-3-2", 64, lane_offset=rank * 64)
            q = ra.RnnChain(eng, "gru", env.D, 8, 3, mlp_hidden=8)
            q.init(3)
            dqn = ra.FiniteDqn(env, q, ra.Adam(q), dqn_cfg(16, 0.5, minibatch=50, opt_steps=2))
            dqn.collect(9)
            p0, pos0 = q.get_params(), dqn.agent_rng_pos()
            code, msg = refusal(dqn.update)
            out[rank] = (code, "rl_dqn_update" in msg, np.array_equal(q.get_params(), p0), dqn.agent_rng_pos() == pos0)
        except BaseException as exc:  # surface the failure in the main thread
            out[rank] = exc
            raise

    os.environ["RELEARN_LOOPBACK_COMM"] = "1"
    try:
        uid, out = ra.comm_unique_id(), {}
        threads = [threading.Thread(target=run_rank, args=(r, uid, out)) for r in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        for r in range(2):
            assert out.get(r) == (ra.ERR_UNSUPPORTED, True, True, True), out.get(r)
    finally:
        os.environ.pop("RELEARN_LOOPBACK_COMM", None)


def test_actor_document(engine):
    """DqnActor of a four-action feed-forward agent: action_space { size: 4 }, the four-row last layer, a round trip; a
    recurrent DqnActor stays refused"""
    from cbor_ref import decode
    case = FC.FF_CASES[9]
    env, q = device_env(engine, case.env, 64), device_module(engine, case)
    ra.FiniteDqn(env, q, ra.Adam(q), dqn_cfg(16, 0.5)).close()
    data = ra.actor_to_cbor(env, q, ra.ACTOR_DQN, exploration_rate=0.25)
    doc = decode(data)
    assert list(doc) == ["observation_space", "action_space", "action_value_fn", "exploration_rate"]
    assert doc["action_space"] == {"size": 4} and doc["exploration_rate"] == 0.25
    layers = doc["action_value_fn"]["layers"]
    assert len(layers) == 3 and list(layers[-1]["kernel"]["shape"]) == [4, 16] and list(layers[-1]["bias"]["shape"]) == [4]
    other = ra.Mlp(engine, 5, [16, 16], 4, "Tanh", "Identity")
    ra.module_from_cbor(other, data)
    assert np.array_equal(other.get_params(), q.get_params())
    g = ra.RnnChain(engine, "gru", 5, 8, 4, mlp_hidden=8)
    g.init(1)
    code, msg = refusal(lambda: ra.actor_to_cbor(env, g, ra.ACTOR_DQN, exploration_rate=0.0))
    assert code == ra.ERR_UNSUPPORTED and "rl_actor_to_cbor" in msg


# ---------------------------------------------------------------- the reference's own test
# src/agents/testing.rs:14-64 (train_deterministic_bandit) with the settings of src/torch/agents/tests/dqn.rs as
# tests/test_gpu_dqn_index_envs.py has them: learning rate 0.1, minibatch_steps 10, update size 10, 10 periods, discount
# 1; then the best arm in at least 900 of 1,000 greedy evaluation steps.
ARM_VALUES = {"4-arms": (0.0, 0.0, 0.0, 1.0), "8-arms": (0.0,) * 7 + (1.0,)}
LEARNERS = [("16x16", False), ("16x16", True), ("gru-16-mlp-16", False)]


def bandit_agent(engine, q, values, n_lanes, td=False, greedy=False):
    env = ra.BanditEnv(engine, n_lanes, values, seed_env=1, seed_actor=2)
    acfg = ra.adam_config_default()
    acfg.learning_rate = 0.1
    cfg = ra.dqn_config_default()  # linear exploration 1.0 -> 0.1 over 10^7 steps, 50 optimisation steps per update
    cfg.target = ra.DQN_TARGET_ONE_STEP_TD if td else ra.DQN_TARGET_REWARD_TO_GO
    cfg.minibatch_steps = 10
    cfg.update_kind, cfg.update_first, cfg.update_rest = ra.COLLECT_FIRST_REST, 10, 10
    cfg.buffer_capacity = 128
    cfg.discount_factor = 1.0
    if greedy:  # the evaluation actor: exploration rate 0 (schedules.rs:38)
        cfg.exploration_kind, cfg.exploration_start = ra.SCHEDULE_CONSTANT, 0.0
    for i in range(8):
        cfg.agent_key[i] = i + 1
    return ra.FiniteDqn(env, q, ra.Adam(q, acfg), cfg)


def train_k_bandit(engine, arms, module, td):
    """ten periods of ten steps (ten lanes x one step), then 1,000 greedy steps of a second agent at rate 0 on the trained
    module (its recorded actions are the greedy ones) -> (the trained module, how often the best arm was pulled)"""
    values, n_lanes = ARM_VALUES[arms], 10
    A = len(values)
    if module == "16x16":
        q = ra.Mlp(engine, 5, [16, 16], A)
        q.init(7)
    else:
        q = ra.RnnChain(engine, "gru", 5, 16, A, mlp_hidden=16)
        q.init_with(7)  # the module configuration's default initializers (host/agents.hpp build_module)
    dqn = bandit_agent(engine, q, values, n_lanes, td=td)
    for _ in range(10):
        m, _slack = dqn.min_update_size()
        assert m == 10
        dqn.collect((m + n_lanes - 1) // n_lanes)
        st = dqn.update()
        assert st.opt_steps == 50 and np.isfinite(st.loss_last)
    greedy = bandit_agent(engine, q, values, n_lanes, greedy=True)
    greedy.collect(100)
    best = int((greedy.replay_read(ra.REPLAY_ACTION)[:100] == A - 1).sum())
    dqn.close()
    greedy.close()
    return q, best


@pytest.mark.parametrize("module,td", LEARNERS, ids=["16x16-reward-to-go", "16x16-one-step-td", "gru-reward-to-go"])
@pytest.mark.parametrize("arms", sorted(ARM_VALUES))
def test_learns_deterministic_bandit(engine, arms, module, td):
    """the reference's bar: the best arm in at least 900 of 1,000 greedy steps.  DESIGN.md section 39 has the counts."""
    _, best = train_k_bandit(engine, arms, module, td)
    print("%s %s td=%s: the best arm in %d of 1000 greedy steps" % (arms, module, td, best))
    assert best >= 900
