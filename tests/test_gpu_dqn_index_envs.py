"""DQN on the index-env lanes — Chain, MemoryGame(2, h), the two-armed DeterministicBandit — through the C ABI: the
collection kernels stepping the env's own lane code (fused module: k_rollout_dqn<IndexOps, D, 64, G>; any other module,
and 6..8 observation features: k_dqn_lane_step<IndexOps, D>), the second record array of observations wider than five
floats, the ring through evictions, minibatches, targets, gradients, and the reference's own DQN acceptance test
(src/torch/agents/tests/dqn.rs: testing::train_deterministic_bandit).

The method is tests/test_gpu_dqn.py::test_general_action_value_module_collection's: the env side replays through the
oracle's lanes (O.ChainLaneSim, O.BanditLaneSim, O.MemoryLaneSim) stepped with the recorded actions; DqnActor::act is
restated on the raw actor stream (O.Prng: gen_bool(eps), then gen_range(0, 2)); the greedy action is the argmax of the
oracle's forward on the same parameters (bit for bit for the fused module, the f64 network for the others).  The ring's
bookkeeping is compared with tests/dqn_ring_ref.py, which tests/test_dqn_ring_ref_cpu.py validates against the oracle's
store.  Bars are those of tests/test_gpu_dqn.py and tests/test_gpu_steps_summary.py."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
from dqn_ring_ref import RingStore
from narrow_cases import dqn_group, dqn_lanes_g8
from steps_summary_ref import close, period_summaries

pytestmark = pytest.mark.gpu

ra = pytest.importorskip("relearn_amd")

KEY = [0x9E3779B9, 0x7F4A7C15, 3, 4, 5, 6, 7, 0xFFFFFFFF]
GRAD_RTOL = 2e-6  # tests/test_gpu_dqn.py::test_minibatch_gradient: vs the f64 evaluation, relative to max |g|
SEEDS = dict(seed_env=11, seed_actor=12)

# name -> (device env, oracle lanes, D, discount factor of the env: chain.rs, memory.rs:74-76, bandits.rs:52-54)
ENVS = {
    "chain": (lambda e, n: ra.ChainEnv(e, n, max_steps=7, limit=ra.LIMIT_LATENT, **SEEDS),
              lambda n: O.ChainLaneSim(n, max_steps=7, limit=O.LIMIT_LATENT, **SEEDS), 5, 0.95),
    "bandit": (lambda e, n: ra.BanditEnv(e, n, (0.0, 1.0), **SEEDS),
               lambda n: O.BanditLaneSim(n, (0.0, 1.0), **SEEDS), 5, 1.0),
    "memory-2-3": (lambda e, n: ra.MemoryEnv(e, n, 2, 3, **SEEDS), lambda n: O.MemoryLaneSim(n, 2, 3, **SEEDS), 5, 1.0),
    "memory-2-2": (lambda e, n: ra.MemoryEnv(e, n, 2, 2, **SEEDS), lambda n: O.MemoryLaneSim(n, 2, 2, **SEEDS), 4, 1.0),
    "memory-2-2-visible-3": (lambda e, n: ra.MemoryEnv(e, n, 2, 2, max_steps=3, limit=ra.LIMIT_VISIBLE, **SEEDS),
                             lambda n: O.MemoryLaneSim(n, 2, 2, max_steps=3, limit=O.LIMIT_VISIBLE, **SEEDS), 5, 1.0),
    # six and eight features: the second record array
    "chain-visible-7": (lambda e, n: ra.ChainEnv(e, n, max_steps=7, limit=ra.LIMIT_VISIBLE, **SEEDS),
                        lambda n: O.ChainLaneSim(n, max_steps=7, limit=O.LIMIT_VISIBLE, **SEEDS), 6, 0.95),
    # (a MemoryGame's episodes all have one length, here six steps: a limit of 4 interrupts every one of them ...
    "memory-2-5-visible-4": (lambda e, n: ra.MemoryEnv(e, n, 2, 5, max_steps=4, limit=ra.LIMIT_VISIBLE, **SEEDS),
                             lambda n: O.MemoryLaneSim(n, 2, 5, max_steps=4, limit=O.LIMIT_VISIBLE, **SEEDS), 8, 1.0),
    # ... and a limit of 6 none: every episode reaches its answer step)
    "memory-2-5-visible-6": (lambda e, n: ra.MemoryEnv(e, n, 2, 5, max_steps=6, limit=ra.LIMIT_VISIBLE, **SEEDS),
                             lambda n: O.MemoryLaneSim(n, 2, 5, max_steps=6, limit=O.LIMIT_VISIBLE, **SEEDS), 8, 1.0),
}
FUSED_ENVS = ["chain", "bandit", "memory-2-3", "memory-2-2", "memory-2-2-visible-3"]
GENERAL_ENVS = FUSED_ENVS + ["chain-visible-7", "memory-2-5-visible-4"]
GENERAL_MODULES = {"16-16-tanh": ([16, 16], "Tanh"), "200-relu": ([200], "Relu")}
# An index env has a handful of distinct observations, so a near tie of the two action values at one of them would take
# a whole class of steps out of the greedy comparison.  With init seed 77 the f64 network's |Q1 - Q0| is at least 1.7e-3
# at EVERY observation each of these envs can emit (possible_observations), for both modules; the collection test asserts
# the margin on the f64 network alone before it compares anything, and then leaves out no step.
MARGIN = 1e-4


def possible_observations(name):
    """every observation the env can emit, [rows][D] f32: one-hot states x (under a visible limit) remaining / max_steps"""
    D = ENVS[name][2]
    visible = "visible" in name
    states = 1 if name == "bandit" else (5 if name.startswith("chain") else D - (1 if visible else 0))
    width = D - 1 if visible else D
    max_steps = int(name.rsplit("-", 1)[1]) if visible else 0
    rows = []
    for s in range(states):
        for k in (range(1, max_steps + 1) if visible else [0]):
            x = np.zeros(D, dtype=np.float32)
            if s < width:
                x[s] = 1.0
            if visible:
                x[D - 1] = np.float32(float(k) / float(max_steps))
            rows.append(x)
    return np.array(rows)


def dqn_cfg(capacity, eps, minibatch=100, opt_steps=4, td=False, gamma=0.99, episode_capacity=0):
    cfg = ra.dqn_config_default()
    cfg.target = ra.DQN_TARGET_ONE_STEP_TD if td else ra.DQN_TARGET_REWARD_TO_GO
    cfg.exploration_kind, cfg.exploration_start = ra.SCHEDULE_CONSTANT, eps
    cfg.minibatch_steps, cfg.opt_steps_per_update, cfg.buffer_capacity = minibatch, opt_steps, capacity
    cfg.episode_capacity = episode_capacity
    cfg.discount_factor = gamma
    for i, k in enumerate(KEY):
        cfg.agent_key[i] = k
    return cfg


def make(engine, name, n, hidden, act="Relu", seed=77, **kw):
    env_of, sim_of, D, gamma = ENVS[name]
    env, sim = env_of(engine, n), sim_of(n)
    assert (env.D, env.A, sim.D) == (D, 2, D)
    q = ra.Mlp(engine, D, hidden, 2, act, "Identity")
    q.init(seed)
    kw.setdefault("gamma", gamma)
    return ra.Dqn(env, q, ra.Adam(q), dqn_cfg(**kw)), sim, q


def actor_streams(n, seed_actor=SEEDS["seed_actor"]):
    L, rngs = O.lib(), []
    for i in range(n):
        r = O.Prng()
        L.oracle_prng_seed_from_u64(C.byref(r), seed_actor)
        L.oracle_prng_set_stream(C.byref(r), i)
        L.oracle_prng_set_word_pos(C.byref(r), 0)
        rngs.append(r)
    return rngs


def last_collection(dqn, T):
    """the device's record of the last collection, time-major, out of the ring (T <= capacity): step t of lane i is at
    slot (total_i - T + t) mod C (replay.rs:89-115)"""
    total = dqn.replay_read(ra.REPLAY_TOTAL).astype(np.int64)
    slots = (total[None, :] - T + np.arange(T)[:, None]) % dqn.C
    take = lambda plane: np.take_along_axis(plane, slots, axis=0)
    obs, nobs = dqn.replay_read(ra.REPLAY_OBS), dqn.replay_read(ra.REPLAY_NEXT_OBS)
    return dict(obs=np.stack([take(obs[d]) for d in range(dqn.D)], axis=1),      # [T][D][n]
                next=np.stack([take(nobs[d]) for d in range(dqn.D)], axis=1),
                action=take(dqn.replay_read(ra.REPLAY_ACTION)), reward=take(dqn.replay_read(ra.REPLAY_REWARD)),
                flag=take(dqn.replay_read(ra.REPLAY_FLAG)))


def check_collection(dqn, sim, rec, T, eps, rngs, greedy):
    """one collection against the oracle's lanes stepped with the recorded actions and the restated actor.  `greedy`:
    observations [D][n] -> the greedy action per lane.  Returns the explored and the greedy steps and the lanes the
    horizon cut mid-episode; no step is left out."""
    L = O.lib()
    n = dqn.n
    cur, explored, greedy_steps, cuts = sim.observe(), 0, 0, 0
    for t in range(T):
        assert np.array_equal(rec["obs"][t], cur), t
        want_a, explore = greedy(cur), np.zeros(n, dtype=bool)
        for i in range(n):
            if L.oracle_prng_gen_bool(C.byref(rngs[i]), eps):
                want_a[i] = L.oracle_prng_gen_range_u64(C.byref(rngs[i]), 0, 2)
                explore[i] = True
        assert np.array_equal(rec["action"][t], want_a), (t, np.flatnonzero(rec["action"][t] != want_a)[:8])
        explored += int(explore.sum())
        greedy_steps += int(n - explore.sum())
        reward, fl, nxt, term = sim.step(rec["action"][t])
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
        cur = nxt
    assert np.array_equal(dqn.replay_read(ra.REPLAY_LAST_FLAGS), rec["flag"])
    pos = np.array([L.oracle_prng_word_pos(C.byref(r)) for r in rngs], dtype=np.uint64)
    assert np.array_equal(dqn.replay_read(ra.REPLAY_ACTOR_POS), pos)
    for a, b in zip(dqn.env.get_state(), sim.get_state()):
        assert np.array_equal(a, b)
    return explored, greedy_steps, cuts


def run_collections(engine, name, n, hidden, act, eps, greedy_of, seed=77, Ts=(9, 7)):
    """two collections, the second from carried env state, actor position and (Chain) global step; both cut lanes mid-
    episode; the StepsSummary of each against numpy on the recorded planes"""
    dqn, sim, q = make(engine, name, n, hidden, act, seed=seed, capacity=sum(Ts), eps=eps)
    if name.startswith("memory"):
        # a MemoryGame's episodes all have one length (here 3, 4 or, interrupted, 4 steps), which divides the first
        # collection's 9 steps or the 16 of both: one standalone step first (device and oracle), so that both collections
        # start and end mid-episode on every lane
        zeros = np.zeros(n, dtype=np.uint8)
        got, want = dqn.env.step(zeros), sim.step(zeros)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    greedy = greedy_of(q)
    rngs, summary = actor_streams(n), ra.StepsSummary(engine, n)
    rewards, flags, counts = [], [], np.zeros(2, dtype=np.int64)
    for T in Ts:
        st = dqn.collect(T)
        summary.push_dqn(dqn)
        got = summary.read()
        summary.clear()
        rec = last_collection(dqn, T)
        explored, greedy_steps, cuts = check_collection(dqn, sim, rec, T, eps, rngs, greedy)
        counts += (explored, greedy_steps)
        assert st.steps == T * n and st.episodes_ended == int((rec["flag"] != 0).sum())
        assert cuts > 0 or name == "bandit"  # lanes are cut mid-episode at the end of every collection
        rewards.append(rec["reward"])
        flags.append(rec["flag"])
        want = period_summaries(rewards, flags)[-1]
        for f in ("step_reward", "episode_reward", "episode_length"):
            close(getattr(got, f), want[f], f)
    assert np.array_equal(dqn.replay_read(ra.REPLAY_TOTAL), np.full(n, sum(Ts), dtype=np.uint32))
    if eps == 1.0:
        assert counts[1] == 0
    elif eps == 0.0:
        assert counts[0] == 0
    else:
        assert counts.min() > 0.3 * n * sum(Ts)
    dqn.close()
    return rewards, flags


@pytest.mark.parametrize("lanes", ["200", "g8"])
@pytest.mark.parametrize("hidden", [32, 128])
@pytest.mark.parametrize("name", FUSED_ENVS)
def test_fused_collection_bit_exact(engine, name, hidden, lanes):
    """k_rollout_dqn<IndexOps, D, 64, G>: 200 lanes (no multiple of 64) run G = 16, the second lane count G = 8; a
    collection that always explores (eps = 1.0) runs G = 1.  The fused forward is the oracle's bit for bit, so every
    greedy action is compared."""
    cus = engine.info()[2]
    n = 200 if lanes == "200" else dqn_lanes_g8(cus)
    assert dqn_group(n, cus) == (16 if lanes == "200" else 8)
    D = ENVS[name][2]
    shape = O.MlpShape(D, hidden, 2)

    def greedy_of(q):
        params = q.get_params()
        assert np.array_equal(params, O.mlp_init(shape, 77))

        def greedy(obs):
            z = O.mlp_forward_batch(shape, params, obs.T)
            return (z[:, 1] > z[:, 0]).astype(np.uint8)  # argmax: first maximal index
        return greedy

    taken = set()
    for eps in (1.0, 0.5, 0.0):
        rewards, _ = run_collections(engine, name, n, hidden, "Relu", eps, greedy_of)
        taken |= set(np.unique(np.concatenate(rewards)).tolist())
    if name == "bandit":
        assert taken == {0.0, 1.0}  # both arms were pulled
    elif name == "chain":
        assert {0.0, 2.0} <= taken
    else:
        assert taken == {-1.0, 0.0, 1.0}  # right and wrong answers


@pytest.mark.parametrize("module", sorted(GENERAL_MODULES))
@pytest.mark.parametrize("name", GENERAL_ENVS)
def test_general_collection(engine, name, module):
    """k_dqn_lane_step<IndexOps, D>, D = 4..8, behind the per-layer kernels; the greedy action against the f64 network
    at every step (the margin asserted first, on the f64 network alone)"""
    from test_gpu_general_mlp import forward64, unflatten
    hidden, act = GENERAL_MODULES[module]
    D = ENVS[name][2]
    seen = []

    def greedy_of(q):
        net = unflatten(q.get_params(), D, hidden, 2)

        def greedy(obs):
            z, _ = forward64(net, obs.T, act, "Identity")
            seen.append(np.abs(z[:, 1] - z[:, 0]).min())
            return (z[:, 1] > z[:, 0]).astype(np.uint8)
        return greedy

    z, _ = forward64(unflatten(O.mlp_layers_init(D, hidden, 2, 77), D, hidden, 2), possible_observations(name), act,
                     "Identity")
    assert np.abs(z[:, 1] - z[:, 0]).min() > MARGIN
    for eps in (0.5, 0.0):
        run_collections(engine, name, 200, hidden, act, eps, greedy_of)
    assert min(seen) > MARGIN, min(seen)  # (and on the device's own parameters, at what occurred)


def oracle_planes(sim, action):
    """the oracle's lanes stepped with recorded actions [T][n] -> a collection's planes as the store must hold them"""
    T = len(action)
    obs, nxt_o, rew, flag = [], [], [], []
    cur = sim.observe()
    for t in range(T):
        obs.append(cur)
        r, fl, nxt, term = sim.step(action[t])
        fl, succ = fl.copy(), term
        if t == T - 1:
            cut = fl == O.CONTINUE
            fl[cut] = O.INTERRUPT
            succ = np.where(cut[None], nxt, term)
        rew.append(r)
        flag.append(fl)
        nxt_o.append(succ)
        cur = nxt
    return np.array(obs), action, np.array(rew), np.array(flag), np.array(nxt_o)


@pytest.mark.parametrize("name,capacity,Ts,hidden", [("bandit", 8, (5, 5, 5), 128), ("chain", 20, (9, 7, 9), 128),
                                                      ("chain-visible-7", 20, (9, 7, 9), [16, 16])])
def test_eviction_matches_the_restated_ring(engine, name, capacity, Ts, hidden):
    """bandit lanes: every step is an episode, so the episode table fills and wraps with the steps; Chain lanes: whole
    episodes of up to seven steps leave.  Every ring word and every stored step against tests/dqn_ring_ref.py, fed by the
    oracle's lanes stepped with the device's actions."""
    n = 70
    dqn, sim, q = make(engine, name, n, hidden, capacity=capacity, eps=0.5)
    store = RingStore(n, capacity, dqn.D)
    for T in Ts:
        dqn.collect(T)
        store.write_collection(*oracle_planes(sim, last_collection(dqn, T)["action"]))
        store.check_device(dqn, ra)
    heads = dqn.replay_read(ra.REPLAY_HEAD)
    eph = dqn.replay_read(ra.REPLAY_EP_HEAD)
    assert heads.min() > 0 and eph.min() > 0  # every lane has evicted
    if name == "bandit":
        assert (eph + dqn.replay_read(ra.REPLAY_EP_COUNT)).min() > dqn.E  # the episode table has wrapped


def dqn_grad64(shape, params, obs, actions, targets):
    g, loss = np.zeros(len(params), dtype=np.float64), C.c_double()
    O.lib().oracle_dqn_grad_f64(shape, O.f64p(params.astype(np.float64)),
                                O.f64p(np.ascontiguousarray(obs, dtype=np.float64)),
                                O.i64p(np.ascontiguousarray(actions, dtype=np.int64)),
                                O.f64p(np.ascontiguousarray(targets, dtype=np.float64)), len(actions), O.f64p(g),
                                C.byref(loss))
    return g, loss.value


# (env, hidden, activation, kernel variants): the fused module on both kernel variants, the per-layer kernels have one
MINIBATCH_CASES = [("chain", 128, "Relu", (0, 1)), ("bandit", 128, "Relu", (0, 1)), ("memory-2-3", 128, "Relu", (0, 1)),
                   ("chain-visible-7", [16, 16], "Tanh", (0,)), ("memory-2-5-visible-6", [200], "Relu", (0,)),
                   ("chain", [16, 16], "Tanh", (0,))]
MINIBATCH_PARAMS = [(c[0], c[1], c[2], v) for c in MINIBATCH_CASES for v in c[3]]


@pytest.mark.parametrize("td", [False, True], ids=["reward-to-go", "one-step-td"])
@pytest.mark.parametrize("name,hidden,act,variant", MINIBATCH_PARAMS,
                         ids=["%s-%s-%s" % (c[0], c[1] if isinstance(c[1], int) else "x".join(map(str, c[1])),
                                            ["kernels-best", "kernels-v1"][c[3]]) for c in MINIBATCH_PARAMS])
def test_minibatch_targets_and_gradient(engine, name, hidden, act, variant, td):
    """a minibatch out of an index-env store: the sampled episodes exist in the restated ring, the gathered observations
    and actions are the stored ones bit for bit, the targets are the f64 restatement's from the device's own store
    (reward-to-go with the env's discount; one-step TD with 0 beyond a Terminate and the stored successor after an
    Interrupt), gradient and loss at the bars of tests/test_gpu_dqn.py; then an update"""
    engine.set_kernel_variant(variant)
    try:
        minibatch_case(engine, name, hidden, act, variant, td)
    finally:
        engine.set_kernel_variant(0)


def minibatch_case(engine, name, hidden, act, variant, td):
    from test_gpu_general_mlp import backward64, forward64, unflatten
    fused = isinstance(hidden, int)
    n, Ts = 128, (9, 7, 9)
    gamma = ENVS[name][3]
    dqn, sim, q = make(engine, name, n, hidden, act, capacity=24, eps=0.5, minibatch=600, opt_steps=6, td=td)
    D = dqn.D
    store = RingStore(n, 24, D)
    for T in Ts:
        dqn.collect(T)
        store.write_collection(*oracle_planes(sim, last_collection(dqn, T)["action"]))
    ne, ns = dqn.minibatch_sample()
    obs, a, tgt = dqn.minibatch_read(ra.MB_OBS), dqn.minibatch_read(ra.MB_ACTION), dqn.minibatch_read(ra.MB_TARGET)
    lanes, starts, lens = (dqn.minibatch_read(f) for f in (ra.MB_EP_LANE, ra.MB_EP_START, ra.MB_EP_LEN))
    assert ne == len(lanes) and ns == int(lens.sum()) and 600 <= ns < 600 + 24
    hlist = [hidden] if fused else hidden
    net = unflatten(q.get_params(), D, hlist, 2)
    want_t, k = np.zeros(ns), 0
    for ln, st, le in zip(lanes, starts, lens):
        ring = store.rings[ln]
        assert (int(st), int(le)) in [ring.episode(e) for e in range(ring.num_episodes())], (ln, st, le)
        steps = [store.step_data(ln, int(st) + j) for j in range(int(le))]
        assert np.array_equal(obs[:, k:k + le], np.array([s[0] for s in steps]).T)
        assert np.array_equal(a[k:k + le], np.array([s[1] for s in steps], dtype=np.uint8))
        r = np.array([s[2] for s in steps], dtype=np.float64)
        fl = np.array([s[3] for s in steps])
        assert fl[-1] != O.CONTINUE and np.all(fl[:-1] == O.CONTINUE)
        if td:
            succ = np.array([steps[j][4] if (fl[j] == O.INTERRUPT or j == le - 1) else steps[j + 1][0]
                             for j in range(int(le))])
            zn, _ = forward64(net, succ, act, "Identity")
            vn = np.where(fl == O.TERMINATE, 0.0, zn.max(axis=1))
            want_t[k:k + le] = r + float(np.float32(gamma)) * vn
        else:
            g = 0.0
            for j in range(int(le) - 1, -1, -1):
                g = r[j] + (float(np.float32(gamma)) * g if j < le - 1 else 0.0)
                want_t[k + j] = g
            if name == "bandit":
                assert np.array_equal(tgt[k:k + le], r.astype(np.float32))  # bit-exactly the rewards
        k += int(le)
    assert k == ns and np.allclose(tgt, want_t, rtol=2e-5, atol=2e-5)
    z, acts = forward64(net, obs.T, act, "Identity")
    qa = z[np.arange(ns), a]
    g_d, loss_d = dqn.minibatch_gradient()
    want_loss = ((qa - tgt) ** 2).mean()
    if fused:  # test_minibatch_gradient's bars
        g64, loss64 = dqn_grad64(O.MlpShape(D, hidden, 2), q.get_params(), obs.T, a, tgt)
        err = np.abs(g_d - g64).max() / max(np.abs(g64).max(), 1e-30)
        print("%s td=%s variant %d: gradient vs f64 %.3g (bar %.3g), loss %.9g vs %.9g" % (name, td, variant, err,
                                                                                         GRAD_RTOL, loss_d, loss64))
        assert err < GRAD_RTOL
        assert abs(loss_d - loss64) <= 2e-6 * abs(loss64)
        assert np.isfinite(g_d).all() and np.abs(g_d).max() > 0
    else:  # test_general_action_value_module_update's bars
        dz = np.zeros_like(z)
        dz[np.arange(ns), a] = 2.0 * (qa - tgt.astype(np.float64)) / ns
        want_g = backward64(net, obs.T, acts, dz)
        print("%s td=%s: gradient vs f64 %.3g of max, loss %.9g vs %.9g" % (
            name, td, np.abs(g_d - want_g).max() / np.abs(want_g).max(), loss_d, want_loss))
        assert np.abs(g_d - want_g).max() <= 2e-5 * np.abs(want_g).max() + 1e-9
        assert abs(loss_d - want_loss) <= 1e-5 * want_loss
    p0 = q.get_params()
    st, losses = dqn.update(want_losses=True)
    assert st.opt_steps == 6 and np.all(np.isfinite(losses)) and not np.array_equal(q.get_params(), p0)
    dqn.close()


@pytest.mark.parametrize("limit,visible", [(64, False), (65, True), (130, False)],
                         ids=["64-steps", "65-steps-6-features", "130-steps"])
def test_reward_to_go_of_one_minibatch_across_scan_chunks(engine, limit, visible):
    """rl_dqn_minibatch_sample with reward-to-go targets, the one-at-a-time builder: its scan walks an episode in chunks of
    64 steps from the end.  Chain lanes end an episode at the step limit alone, so every episode is exactly one chunk (64
    steps), one chunk and one step (65; six features: the second record array is read) or two chunks and two steps (130).
    Collections of one step limit each keep every episode whole; a capacity of three episodes and seven steps makes the
    fourth one wrap in the ring.  The discount factor 0.9 has inexact powers in f32: a scan that associated differently
    would round differently.  Three episodes per minibatch.  Observations and actions against the restated store, the
    targets against the oracle's discounted_cumsum_from_end on the stored rewards — all bit for bit."""
    L, n, capacity, gamma = O.lib(), 6, 3 * limit + 7, np.float32(0.9)
    kind, D = (ra.LIMIT_VISIBLE, 6) if visible else (ra.LIMIT_LATENT, 5)
    env = ra.ChainEnv(engine, n, max_steps=limit, limit=kind, **SEEDS)
    sim = O.ChainLaneSim(n, max_steps=limit, limit=O.LIMIT_VISIBLE if visible else O.LIMIT_LATENT, **SEEDS)
    assert (env.D, sim.D) == (D, D)
    q = ra.Mlp(engine, D, [16, 16] if visible else 128, 2, "Tanh" if visible else "Relu", "Identity")
    q.init(77)
    dqn = ra.Dqn(env, q, ra.Adam(q), dqn_cfg(capacity, 0.5, minibatch=2 * limit + 1, opt_steps=1, gamma=float(gamma)))
    store = RingStore(n, capacity, D)
    for _ in range(4):
        dqn.collect(limit)
        store.write_collection(*oracle_planes(sim, last_collection(dqn, limit)["action"]))
    store.check_device(dqn, ra)
    wrapped = False
    for _ in range(8):
        ne, ns = dqn.minibatch_sample()
        obs, a, tgt = dqn.minibatch_read(ra.MB_OBS), dqn.minibatch_read(ra.MB_ACTION), dqn.minibatch_read(ra.MB_TARGET)
        lanes, starts, lens = (dqn.minibatch_read(f) for f in (ra.MB_EP_LANE, ra.MB_EP_START, ra.MB_EP_LEN))
        assert (ne, ns) == (3, 3 * limit) and np.all(lens == limit)
        assert np.array_equal(dqn.minibatch_read(ra.MB_EP_OFFSET), np.cumsum(lens) - lens)
        k = 0
        for ln, st in zip(lanes, starts):
            ring = store.rings[ln]
            assert (int(st), limit) in [ring.episode(e) for e in range(ring.num_episodes())], (ln, st)
            wrapped |= int(st) % capacity + limit > capacity
            steps = [store.step_data(ln, int(st) + j) for j in range(limit)]
            assert np.array_equal(obs[:, k:k + limit], np.array([s[0] for s in steps]).T)
            assert np.array_equal(a[k:k + limit], np.array([s[1] for s in steps], dtype=np.uint8))
            want = np.array([s[2] for s in steps], dtype=np.float32)
            assert np.unique(want).size > 1  # (rewards of 0 and 2: the returns are sums of many powers of 0.9)
            ones = np.ones(limit, dtype=np.uint64)
            L.oracle_discounted_cumsum_from_end_f32(O.f32p(want), limit, float(gamma), O.u64p(ones), limit)
            assert np.array_equal(tgt[k:k + limit], want), (ln, st)
            k += limit
    assert wrapped  # an episode that lies across the ring's end was among the sampled ones
    dqn.close()


@pytest.mark.parametrize("td", [False, True], ids=["reward-to-go", "one-step-td"])
def test_a_failed_draw_leaves_the_bandit_agent_as_it_was(engine, td):
    """the all-or-nothing update (tests/test_gpu_dqn.py) on bandit lanes: a sampler failure injected into a later chunk
    of the pipelined draws leaves network and optimiser as they were"""
    dqn, _, q = make(engine, "bandit", 128, 128, capacity=16, eps=0.5, minibatch=200, opt_steps=12, td=td)
    ref, _, qr = make(engine, "bandit", 128, 128, capacity=16, eps=0.5, minibatch=200, opt_steps=12, td=td)
    dqn.collect(10)
    ref.collect(10)
    before = q.get_params()
    for agent, chunk in ((dqn, "2"), (ref, "0")):  # (the failed call consumed its draws: the reference agent fails too)
        os.environ["RELEARN_DQN_FAIL_CHUNK"] = chunk
        try:
            with pytest.raises(ra.RelearnError) as e:
                agent.update()
            assert e.value.code == ra.ERR_INVALID_ARGUMENT
        finally:
            os.environ.pop("RELEARN_DQN_FAIL_CHUNK", None)
    assert np.array_equal(q.get_params(), before) and np.array_equal(qr.get_params(), before)
    assert dqn.agent_rng_pos() == ref.agent_rng_pos()
    _, la = dqn.update(want_losses=True)
    _, lb = ref.update(want_losses=True)
    assert np.array_equal(la, lb) and np.array_equal(q.get_params(), qr.get_params())
    assert not np.array_equal(q.get_params(), before)


def test_refusals(engine):
    """DQN stays at two actions and feed-forward modules"""
    env3 = ra.MemoryEnv(engine, 64, 3, 2, **SEEDS)
    q3 = ra.Mlp(engine, env3.D, [32], 3)
    q3.init(1)
    with pytest.raises(ra.RelearnError) as e:
        ra.Dqn(env3, q3, ra.Adam(q3), dqn_cfg(16, 0.5))
    assert e.value.code == ra.ERR_UNSUPPORTED
    env = ra.ChainEnv(engine, 64, max_steps=7, **SEEDS)
    g = ra.GruMlp(engine, 5, 2)
    g.init(1)
    with pytest.raises(ra.RelearnError) as e:
        ra.Dqn(env, g, ra.Adam(g), dqn_cfg(16, 0.5))
    assert e.value.code == ra.ERR_BUILD_AGENT


# ---------------------------------------------------------------- the reference's own DQN test
# src/torch/agents/tests/dqn.rs: `testing::train_deterministic_bandit(&config, 10, 0.9)` (src/agents/testing.rs:14-64) on
# DeterministicBandit::from_values([0.0, 1.0]) with learning rate 0.1, minibatch_steps 10, update_size Constant(10) and
# DqnConfig::default() otherwise: 10 training periods, then 1,000 greedy evaluation steps of which at least 900 must pull
# arm 1.
def train_deterministic_bandit(engine, n_lanes, hidden, td=False, seed=7, periods=10):
    env = ra.BanditEnv(engine, n_lanes, (0.0, 1.0), seed_env=1, seed_actor=2)
    q = ra.Mlp(engine, env.D, hidden, 2)
    q.init(seed)
    acfg = ra.adam_config_default()
    acfg.learning_rate = 0.1
    cfg = ra.dqn_config_default()  # linear exploration 1.0 -> 0.1 over 10^7 steps, 50 optimisation steps per update
    cfg.target = ra.DQN_TARGET_ONE_STEP_TD if td else ra.DQN_TARGET_REWARD_TO_GO
    cfg.minibatch_steps = 10
    cfg.update_kind, cfg.update_first, cfg.update_rest = ra.COLLECT_FIRST_REST, 10, 10
    cfg.buffer_capacity = (10_000_000 + n_lanes - 1) // n_lanes
    cfg.buffer_capacity = min(cfg.buffer_capacity, 4096)  # (ten periods write 10 steps per lane at the most)
    cfg.discount_factor = 1.0
    for i in range(8):
        cfg.agent_key[i] = i + 1
    dqn = ra.Dqn(env, q, ra.Adam(q, acfg), cfg)
    for _ in range(periods):
        m, _slack = dqn.min_update_size()
        assert m == 10
        dqn.collect((m + n_lanes - 1) // n_lanes)
        st = dqn.update()
        assert st.opt_steps == 50 and np.isfinite(st.loss_last)
    return env, q, dqn


def greedy_evaluation(env, q, steps=1000):
    """the evaluation actor: the greedy action of q.forward on the env's observation; returns how often arm 1 was pulled"""
    ones = taken = 0
    while taken < steps:
        z = q.forward(np.ascontiguousarray(env.observe().T))
        a = (z[:, 1] > z[:, 0]).astype(np.uint8)
        k = min(env.n, steps - taken)
        ones += int(a[:k].sum())
        taken += k
        env.step(a)
    return ones


@pytest.mark.parametrize("td", [False, True], ids=["reward-to-go", "one-step-td"])
@pytest.mark.parametrize("hidden", [128, [16, 16]], ids=["128-fused", "16x16"])
@pytest.mark.parametrize("n_lanes", [10, 2], ids=["10-lanes-x-1-step", "2-lanes-x-5-steps"])
def test_learns_deterministic_bandit(engine, n_lanes, hidden, td):
    env, q, dqn = train_deterministic_bandit(engine, n_lanes, hidden, td)
    ones = greedy_evaluation(env, q)
    print("arm 1 in %d of 1000 greedy steps" % ones)
    assert ones >= 900


def test_chain_dqn_learns_something(engine):
    """a few collect / update rounds on Chain lanes with reward-to-go targets: the loss is finite and falls (the Chain
    analogue of tests/test_gpu_dqn.py::test_cartpole_dqn_learns_something).  The exploration rate is constant at 1.0:
    reward-to-go targets then do not depend on the network at all, the data of every round come from one distribution,
    and the regression loss of a network that starts near zero against returns of 2 to 40 must fall.  (Under an annealed
    rate the greedy share grows from round to round and with it the returns the loss is measured on.)"""
    env = ra.ChainEnv(engine, 256, max_steps=20, limit=ra.LIMIT_LATENT, **SEEDS)
    q = ra.Mlp(engine, 5, 128, 2)
    q.init(77)
    dqn = ra.Dqn(env, q, ra.Adam(q), dqn_cfg(200, 1.0, minibatch=4000, opt_steps=20, gamma=0.95))
    first = last = None
    for it in range(4):
        dqn.collect(40)
        st = dqn.update()
        first = st.loss_first if first is None else first
        last = st.loss_last
        assert np.isfinite(st.loss_first) and np.isfinite(st.loss_last)
    assert last < first
