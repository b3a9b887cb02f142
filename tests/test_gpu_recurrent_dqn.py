"""DQN with a recurrent action-value module (rl_dqn_create_recurrent / ra.RecurrentDqn) through the C ABI: the one-launch
collection kernel k_stack_collect_dqn<CELL, Env, D, LIN> (kernels_seq_stack.hip) bit for bit — every ring plane, the
second record array, flags, actor positions and env state against the oracle's lanes stepped with the recorded actions,
every action against the restated DqnActor of tests/recurrent_dqn_ref.py (an exploring step holds the lane's recurrent
state: tests/test_recurrent_dqn_ref_cpu.py shows that these cases fail a kernel that advances it), the ring words against
tests/dqn_ring_ref.py — then the sampler, both targets bit for bit, gradient and loss against f64 at the bar of
tests/test_gpu_stacked.py, the SGD step, the all-or-nothing update, the refusals, and the reference's own acceptance test
(src/torch/agents/tests/dqn.rs: default_gru_mlp_learns_derministic_bandit).

The shapes are the smallest at which the kernel can go wrong: 70 lanes (a full workgroup plus six live lanes), a GRU of
5 units under an MLP of 6 (one partial unit quad), two LSTM layers of 33 units under a Linear tail without recurrent
bias vectors (a second trip of the unit loop for wave 0 alone), and the 5 -> 128 -> 128 -> 2 shape on one env."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import oracle as O
import recurrent_dqn_ref as R
from dqn_ring_ref import RingStore
from oracle import stacked as S
from steps_summary_ref import close, period_summaries

pytestmark = pytest.mark.gpu

ra = pytest.importorskip("relearn_amd")

from test_gpu_dqn_index_envs import KEY, dqn_cfg, last_collection  # noqa: E402
from test_gpu_stacked import GRAD_RTOL, rel_err  # noqa: E402  (the bar the recurrent gradients are held to)

SEEDS = R.SEEDS
DEVICE_ENVS = {
    "chain-latent-7": lambda e, n: ra.ChainEnv(e, n, max_steps=7, limit=ra.LIMIT_LATENT, **SEEDS),
    "chain-visible-7": lambda e, n: ra.ChainEnv(e, n, max_steps=7, limit=ra.LIMIT_VISIBLE, **SEEDS),
    "bandit": lambda e, n: ra.BanditEnv(e, n, (0.0, 1.0), **SEEDS),
    "memory-2-3": lambda e, n: ra.MemoryEnv(e, n, 2, 3, **SEEDS),
    "memory-2-6": lambda e, n: ra.MemoryEnv(e, n, 2, 6, **SEEDS),
    "cartpole-visible-7": lambda e, n: ra.CartPoleEnv(e, n, max_steps=7, limit=ra.LIMIT_VISIBLE, **SEEDS),
}


def device_module(engine, m, D, seed=None):
    if m.H2 is None:
        q = (ra.GruLinear if m.cell == "gru" else ra.LstmLinear)(engine, D, 2, m.H, num_layers=m.L, rnn_bias=m.bias)
    else:
        q = (ra.GruMlp if m.cell == "gru" else ra.LstmMlp)(engine, D, 2, m.H, m.H2, num_layers=m.L, rnn_bias=m.bias)
    if seed is not None:
        if m.bias:
            q.init_with(seed, bias=R.BIAS_INIT)
        else:
            q.init(seed)
        assert np.array_equal(q.get_params(), R.module_params(m, D, seed))
    return q


def make(engine, case, n=R.N_LANES, opt=None, **kw):
    env_name, mod, seed = case
    sim_of, D, gamma = R.ENVS[env_name]
    env, sim = DEVICE_ENVS[env_name](engine, n), sim_of(n)
    assert (env.D, env.A, sim.D) == (D, 2, D)
    R.warm_up(env_name, sim, env)
    q = device_module(engine, R.MODULES[mod], D, seed)
    kw.setdefault("gamma", gamma)
    return ra.RecurrentDqn(env, q, opt(q) if opt else ra.Adam(q), dqn_cfg(**kw)), sim, q


def check_collection(dqn, sim, actor, T, eps, store):
    """one collection: the env side against the oracle's lanes stepped with the recorded actions, every action against
    the restated actor; the collection's planes go into the restated ring.  -> (explored, greedy, horizon cuts)"""
    n = dqn.n
    rec = last_collection(dqn, T)
    actor.begin_collection()
    cur, explored, cuts = sim.observe(), 0, 0
    flags, succs = [], []
    for t in range(T):
        assert np.array_equal(rec["obs"][t], cur), t
        want_a, explore, _, _ = actor.act(cur, eps)
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
    return explored, n * T - explored, cuts


@pytest.mark.parametrize("eps", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("case", R.COLLECT_CASES, ids=R.case_id)
def test_collection_bit_exact(engine, case, eps):
    """two collections of 9 and 7 steps: episodes start and end mid-collection, the state restarts at a collection's
    first step; no step is left out of the action comparison"""
    dqn, sim, q = make(engine, case, capacity=sum(R.HORIZONS), eps=eps)
    params = q.get_params()
    actor = R.RecurrentActor(R.MODULES[case[1]], dqn.D, params, dqn.n, SEEDS["seed_actor"])
    store = RingStore(dqn.n, sum(R.HORIZONS), dqn.D)
    counts = np.zeros(2, dtype=np.int64)
    summary, rewards, flags = ra.StepsSummary(engine, dqn.n), [], []
    for T in R.HORIZONS:
        st = dqn.collect(T)
        summary.push_dqn(dqn)  # rl_summary_push_dqn takes the handle: the period's StepsSummary against numpy
        got = summary.read()
        summary.clear()
        explored, greedy, cuts = check_collection(dqn, sim, actor, T, eps, store)
        counts += (explored, greedy)
        assert st.steps == T * dqn.n and (cuts > 0 or case[0] == "bandit")
        rec = last_collection(dqn, T)
        rewards.append(rec["reward"])
        flags.append(rec["flag"])
        want = period_summaries(rewards, flags)[-1]
        for f in ("step_reward", "episode_reward", "episode_length"):
            close(getattr(got, f), want[f], f)
    assert np.array_equal(dqn.replay_read(ra.REPLAY_TOTAL), np.full(dqn.n, sum(R.HORIZONS), dtype=np.uint32))
    assert np.array_equal(q.get_params(), params)
    if eps == 1.0:
        assert counts[1] == 0
    elif eps == 0.0:
        assert counts[0] == 0
    else:
        assert counts.min() > 0.3 * dqn.n * sum(R.HORIZONS)
    dqn.close()


def test_eviction_matches_the_restated_ring(engine):
    """bandit lanes with capacity 8: every step is an episode, the episode table fills and wraps with the steps"""
    case = ("bandit", "gru-5-mlp-6", 77)
    dqn, sim, q = make(engine, case, capacity=8, eps=0.5)
    actor = R.RecurrentActor(R.MODULES[case[1]], dqn.D, q.get_params(), dqn.n, SEEDS["seed_actor"])
    store = RingStore(dqn.n, 8, dqn.D)
    for T in (5, 5, 5):
        dqn.collect(T)
        check_collection(dqn, sim, actor, T, 0.5, store)
    assert dqn.replay_read(ra.REPLAY_HEAD).min() > 0 and dqn.replay_read(ra.REPLAY_EP_HEAD).min() > 0
    assert (dqn.replay_read(ra.REPLAY_EP_HEAD) + dqn.replay_read(ra.REPLAY_EP_COUNT)).min() > dqn.E
    dqn.close()


# ---------------------------------------------------------------- minibatches
MINIBATCH_CASES = [("chain-latent-7", "gru-5-mlp-6", 88), ("memory-2-3", "lstm-2x33-linear-nobias", 85),
                   ("cartpole-visible-7", "gru-5-mlp-6", 90), ("chain-visible-7", "lstm-2x33-linear-nobias", 113),
                   ("chain-latent-7", "gru-128-mlp-128", 86)]


def filled(engine, case, td, minibatch=300, opt_steps=3, opt=None):
    """an agent after the 9 + 7 collections at eps = 0.5, and the restated ring of its store"""
    dqn, sim, q = make(engine, case, capacity=sum(R.HORIZONS), eps=0.5, minibatch=minibatch, opt_steps=opt_steps, td=td,
                       opt=opt)
    actor = R.RecurrentActor(R.MODULES[case[1]], dqn.D, q.get_params(), dqn.n, SEEDS["seed_actor"])
    store = RingStore(dqn.n, sum(R.HORIZONS), dqn.D)
    for T in R.HORIZONS:
        dqn.collect(T)
        check_collection(dqn, sim, actor, T, 0.5, store)
    return dqn, q, store


def minibatch_reference(dqn, q, store, case, td, lanes, starts, lens):
    """the restated minibatch in episode-after-episode order: observations, actions, f32 targets, flags"""
    m = R.MODULES[case[1]]
    shape, _, full, _ = R.embedded(m, dqn.D, q.get_params())
    obs, act, tgt, flags = [], [], [], []
    for ln, st, le in zip(lanes, starts, lens):
        steps = [store.step_data(int(ln), int(st) + j) for j in range(int(le))]
        o = np.array([s[0] for s in steps], dtype=np.float32)
        fl = np.array([s[3] for s in steps], dtype=np.uint8)
        assert fl[-1] != O.CONTINUE and np.all(fl[:-1] == O.CONTINUE)
        obs.append(o)
        act.append(np.array([s[1] for s in steps], dtype=np.uint8))
        flags.append(fl)
        tgt.append(R.episode_targets(shape, m.L, full, o, [s[2] for s in steps], fl,
                                     np.array([s[4] for s in steps], dtype=np.float32), dqn.cfg.discount_factor, td))
    return obs, act, tgt, flags


@pytest.mark.parametrize("td", [False, True], ids=["reward-to-go", "one-step-td"])
@pytest.mark.parametrize("case", MINIBATCH_CASES, ids=R.case_id)
def test_sampling_targets_and_gradient(engine, case, td):
    """the episode lists and the agent-Prng position against the restated sampler; the gathered steps against the restated
    ring; RL_MB_TARGET bit for bit against the restatement; gradient and loss against f64 (oracle/stacked.py backward
    with the DQN dz) on the padded layout — episodes of unequal length"""
    dqn, q, store = filled(engine, case, td)
    agent = R.agent_stream(KEY)
    for _ in range(2):  # (the second minibatch continues the agent's stream)
        ne, ns = dqn.minibatch_sample()
        lanes, starts, lens = (dqn.minibatch_read(f) for f in (ra.MB_EP_LANE, ra.MB_EP_START, ra.MB_EP_LEN))
        want = R.sample_minibatch(agent, store.rings, 300)
        for got, w in zip((lanes, starts, lens), want):
            assert np.array_equal(got, w)
        assert dqn.agent_rng_pos() == O.lib().oracle_prng_word_pos(C.byref(agent))
        assert ne == len(lanes) and ns == int(lens.sum()) and 300 <= ns < 300 + sum(R.HORIZONS)
        assert np.array_equal(dqn.minibatch_read(ra.MB_EP_OFFSET), np.concatenate([[0], np.cumsum(lens)[:-1]]))
    obs, act, tgt, flags = minibatch_reference(dqn, q, store, case, td, lanes, starts, lens)
    assert np.array_equal(dqn.minibatch_read(ra.MB_OBS), np.concatenate(obs).T)
    assert np.array_equal(dqn.minibatch_read(ra.MB_ACTION), np.concatenate(act))
    got_t = dqn.minibatch_read(ra.MB_TARGET)
    assert np.array_equal(got_t, np.concatenate(tgt)), np.abs(got_t - np.concatenate(tgt)).max()
    # what the case covers
    last = np.array([f[-1] for f in flags])
    assert len(set(lens.tolist())) > 1  # episodes of unequal length: the layout has padding
    if case[0].startswith("chain-latent"):
        assert set(lens.tolist()) >= {7, 2, 5} and np.all(last == O.INTERRUPT)  # true Interrupts and horizon cuts
    if case[0].startswith("memory"):
        assert (last == O.TERMINATE).any() and (last == O.INTERRUPT).any()
    # gradient and loss on the padded layout against f64
    m = R.MODULES[case[1]]
    _, spec, full, index = R.embedded(m, dqn.D, q.get_params())
    T, n = int(lens.max()), len(lens)
    traj = dict(obs=np.zeros((dqn.D, T + 1, n)), flag=np.full((T, n), O.TERMINATE, dtype=np.uint8))
    dz = np.zeros((2, T, n))
    for e in range(n):
        traj["obs"][:, :lens[e], e] = obs[e].T
        traj["flag"][:lens[e], e] = flags[e]
    qv, _, _ = S.forward(spec, full, traj, want_succ=False)
    loss64 = 0.0
    for e in range(n):
        for t in range(int(lens[e])):
            d = qv[act[e][t], t, e] - float(tgt[e][t])
            dz[act[e][t], t, e] = 2.0 * d / ns
            loss64 += d * d / ns
    g64 = S.backward(spec, full, traj, dz)[index]
    g_d, loss_d = dqn.minibatch_gradient()
    print("%s td=%s: gradient vs f64 %.3g (bar %.3g), loss %.9g vs %.9g" % (R.case_id(case), td, rel_err(g_d, g64),
                                                                             GRAD_RTOL, loss_d, loss64))
    assert g_d.shape == g64.shape and np.abs(g64).max() > 0
    assert rel_err(g_d, g64) < GRAD_RTOL
    assert abs(loss_d - loss64) <= 1e-5 * loss64  # tests/test_gpu_stacked.py's bar for a recurrent loss
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
@pytest.mark.parametrize("case", MINIBATCH_CASES[:3], ids=R.case_id)
def test_sgd_step_is_the_minibatch_gradient(engine, case, td):
    """one optimisation step under plain SGD: (p0 - p1) / lr is rl_dqn_minibatch_gradient's vector of the update's first
    minibatch within the read-back term (tests/test_gpu_ppo_clip.py), losses_out[0] that minibatch's loss"""
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
        R.case_id(case), td, np.maximum(diff - readback, 0.0).max() / np.abs(g0).max(), losses[0], loss0))
    assert np.all(diff <= readback)
    assert abs(losses[0] - loss0) <= 2e-6 * abs(loss0) and st.loss_first == losses[0]
    probe.close()
    dqn.close()


def adam(q):
    return ra.Optimizer(q, ra.optimizer_config_default(ra.OPTIMIZER_ADAM))


@pytest.mark.parametrize("td", [False, True], ids=["reward-to-go", "one-step-td"])
def test_a_failed_chunk_leaves_the_agent_as_it_was(engine, td):
    """RELEARN_DQN_FAIL_CHUNK: parameters, optimiser state and step count come back bit for bit; the agent then updates
    like one that failed before its first step"""
    case = MINIBATCH_CASES[0]
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
            with pytest.raises(ra.RelearnError) as e:
                agent.update()
            assert e.value.code == ra.ERR_INVALID_ARGUMENT
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


# ---------------------------------------------------------------- refusals
def refusal(f):
    with pytest.raises(ra.RelearnError) as e:
        f()
    assert "rl_dqn_create_recurrent" in str(e.value) or "rl_dqn_update" in str(e.value), str(e.value)
    return e.value.code, str(e.value)


def test_refusals(engine):
    cfg = dqn_cfg(16, 0.5)
    chain = ra.ChainEnv(engine, 64, max_steps=7, **SEEDS)
    ff = ra.Mlp(engine, 5, 32, 2)
    code, msg = refusal(lambda: ra.RecurrentDqn(chain, ff, ra.Adam(ff), cfg))
    assert code == ra.ERR_BUILD_AGENT and "use rl_dqn_create" in msg
    env3 = ra.MemoryEnv(engine, 64, 3, 2, **SEEDS)  # five features, three actions
    q3 = ra.RnnChain(engine, "gru", env3.D, 8, 3, mlp_hidden=8)
    assert refusal(lambda: ra.RecurrentDqn(env3, q3, ra.Adam(q3), cfg))[0] == ra.ERR_UNSUPPORTED
    q4 = ra.GruMlp(engine, 4, 2, 8, 8)  # four inputs against Chain's five features
    assert refusal(lambda: ra.RecurrentDqn(chain, q4, ra.Adam(q4), cfg))[0] == ra.ERR_INVALID_ARGUMENT
    q1 = ra.GruMlp(engine, 5, 1, 8, 8)  # one output against two actions
    assert refusal(lambda: ra.RecurrentDqn(chain, q1, ra.Adam(q1), cfg))[0] == ra.ERR_INVALID_ARGUMENT
    meta = ra.MetaBanditEnv(engine, 64, n_arms=2, episodes_per_trial=3)
    qm = ra.GruMlp(engine, meta.D, 2, 8, 8)
    assert refusal(lambda: ra.RecurrentDqn(meta, qm, ra.Adam(qm), cfg))[0] == ra.ERR_UNSUPPORTED
    # every recurrent constructor's module builds, and rl_dqn_create keeps refusing them
    for q in (ra.GruMlp(engine, 5, 2, 8, 8), ra.LstmMlp(engine, 5, 2, 8, 8, num_layers=4), ra.GruLinear(engine, 5, 2, 8),
              ra.LstmLinear(engine, 5, 2, 8, rnn_bias=False), ra.RnnChain(engine, "lstm", 5, 8, 2, num_layers=2)):
        q.init(1)
        ra.RecurrentDqn(chain, q, ra.Adam(q), cfg).close()
        with pytest.raises(ra.RelearnError) as e:
            ra.Dqn(chain, q, ra.Adam(q), cfg)
        assert e.value.code == ra.ERR_BUILD_AGENT
    # an actor document of a recurrent DqnActor: no serde fixture to check it against
    g = ra.GruMlp(engine, 5, 2, 8, 8)
    g.init(1)
    with pytest.raises(ra.RelearnError) as e:
        ra.actor_to_cbor(chain, g, ra.ACTOR_DQN, exploration_rate=0.0)
    assert e.value.code == ra.ERR_UNSUPPORTED and "rl_actor_to_cbor" in str(e.value)


def test_update_is_refused_with_two_ranks():
    """a communicator of two ranks (the in-process loopback collective of tests/test_gpu_multirank.py): rl_dqn_update of a
    recurrent agent answers RL_ERR_UNSUPPORTED before anything is changed"""
    def run_rank(rank, uid, out):
        try:
            eng = ra.Engine(0)
            eng.comm_init(rank, 2, uid)
            env = ra.ChainEnv(eng, 64, max_steps=7, lane_offset=rank * 64, **SEEDS)
            q = ra.GruMlp(eng, 5, 2, 8, 8)
            q.init(3)
            dqn = ra.RecurrentDqn(env, q, ra.Adam(q), dqn_cfg(16, 0.5, minibatch=50, opt_steps=2))
            dqn.collect(9)
            p0, pos0 = q.get_params(), dqn.agent_rng_pos()
            code, _ = refusal(dqn.update)
            out[rank] = (code, np.array_equal(q.get_params(), p0), dqn.agent_rng_pos() == pos0)
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
            assert out.get(r) == (ra.ERR_UNSUPPORTED, True, True), out.get(r)
    finally:
        os.environ.pop("RELEARN_LOOPBACK_COMM", None)


# ---------------------------------------------------------------- the reference's own test
# src/torch/agents/tests/dqn.rs:10-20 over src/agents/testing.rs:14-64: DeterministicBandit::from_values([0, 1]), learning
# rate 0.1, minibatch_steps 10, update size 10, 10 periods; then arm 1 in at least 900 of 1,000 greedy steps.
LEARNING_MODULES = {"gru-mlp-default": R.Module("gru", 128, 1, 128, True), "gru-8-mlp-8": R.Module("gru", 8, 1, 8, True),
                    "lstm-linear": R.Module("lstm", 16, 1, None, True)}


def bandit_agent(engine, q, n_lanes, eps_kind=None, td=False):
    env = ra.BanditEnv(engine, n_lanes, (0.0, 1.0), seed_env=1, seed_actor=2)
    acfg = ra.adam_config_default()
    acfg.learning_rate = 0.1
    cfg = ra.dqn_config_default()  # linear exploration 1.0 -> 0.1 over 10^7 steps, 50 optimisation steps per update
    cfg.target = ra.DQN_TARGET_ONE_STEP_TD if td else ra.DQN_TARGET_REWARD_TO_GO
    cfg.minibatch_steps = 10
    cfg.update_kind, cfg.update_first, cfg.update_rest = ra.COLLECT_FIRST_REST, 10, 10
    cfg.buffer_capacity = 128
    cfg.discount_factor = 1.0
    if eps_kind is not None:  # the evaluation actor: exploration rate 0 (schedules.rs:38)
        cfg.exploration_kind, cfg.exploration_start = ra.SCHEDULE_CONSTANT, 0.0
    for i in range(8):
        cfg.agent_key[i] = i + 1
    return ra.RecurrentDqn(env, q, ra.Adam(q, acfg), cfg)


def train_deterministic_bandit(engine, module, td, n_lanes=10):
    """-> (the trained module, how often the greedy actor pulls arm 1 in 1,000 steps).  The evaluation actor
    (ActorMode::Evaluation: exploration rate 0, schedules.rs:38) is a second agent at rate 0 on the trained module, on
    lanes of its own: its recorded actions are the greedy ones."""
    q = device_module(engine, LEARNING_MODULES[module], 5)
    q.init_with(7)  # the module configuration's default initializers (host/agents.hpp build_module)
    dqn = bandit_agent(engine, q, n_lanes, td=td)
    for _ in range(10):
        m, _slack = dqn.min_update_size()
        assert m == 10
        dqn.collect((m + n_lanes - 1) // n_lanes)
        st = dqn.update()
        assert st.opt_steps == 50 and np.isfinite(st.loss_last)
    greedy = bandit_agent(engine, q, n_lanes, eps_kind="greedy")
    greedy.collect(100)
    ones = int(greedy.replay_read(ra.REPLAY_ACTION)[:100].sum())
    dqn.close()
    greedy.close()
    return q, ones


@pytest.mark.parametrize("td", [False, True], ids=["reward-to-go", "one-step-td"])
@pytest.mark.parametrize("module", sorted(LEARNING_MODULES))
def test_learns_deterministic_bandit(engine, module, td):
    _, ones = train_deterministic_bandit(engine, module, td)
    print("%s td=%s: arm 1 in %d of 1000 greedy steps" % (module, td, ones))
    assert ones >= 900
