"""Recurrent and general modules on TWO ranks, held to one rank's result (tests/sharded_cases.py is the table).

tests/test_gpu_multirank.py shards the fused 5-128 MLPs only; here every module family runs what a sharded update
exchanges through run_pass (relearn_amd/csrc/abi_update.hip): the tile-kernel GRU / LSTM chains (one of them narrow: it
runs on a zero-padded twin and gathers its gradient into flat order before the exchange), the lane-kernel chains
(stacked layers, the linear head, 3..8 actions, the wide ones), a general two-layer MLP over four actions, a narrow
one-layer MLP and, for rl_ppo_update / rl_reinforce_update / the one-step-TD target, the fused 5-128 pair as well.

Two engines of one process, each on its own host thread, joined by the in-process loopback collective
(RELEARN_LOOPBACK_COMM=1, relearn_amd/csrc/abi.hip).  The whole-batch trajectory is collected once on one engine and the
whole case runs there first (the one-rank result; a refusal would surface before a group exists); each rank then gets
its columns of the planes (Trajectory.write_all on v[..., half]), its advantages and returns, and the same parameters.

What a quietly wrong sharded pass would do — scale by the local B instead of B * n_ranks, gather a recurrent gradient
into flat order after the exchange instead of before it, exchange the wrong slice of the vector — moves the probe
vectors by tens of per cent: they are held to the f64 reference of the family at the bar the family's one-rank test
uses (below, with its source), no new tolerance.  RELEARN_LOOPBACK_TEST_WEIGHT is the test of these tests.

A rank that raises must not strand its peer: the groups here run with a 15 s barrier deadline
(RELEARN_LOOPBACK_TIMEOUT_MS), rank threads are daemons joined with a timeout, and a thread still alive after the join
is an assertion failure."""
import os
import threading
import time

import numpy as np
import pytest

import narrow_cases as nc
import oracle as O
import relearn_amd as ra
import seq_multi_ref as R
import sharded_cases as SC
from oracle import stacked as S
from test_gpu_general_mlp import backward64, forward64, jvp64, unflatten

pytestmark = pytest.mark.gpu

WORLD = SC.WORLD
JOIN_S = 120.0
GROUP_DEADLINE_MS = "15000"


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


# ---------------------------------------------------------------------------------------------- modules, envs, data
def build_module(eng, row, net):
    if isinstance(net, SC.Mlp):
        hidden = net.hidden[0] if row.family in ("narrow", "fused") else list(net.hidden)
        m = ra.Mlp(eng, net.D, hidden, net.A, net.act)
    elif row.ctor in ("GruMlp", "LstmMlp"):
        cls = ra.GruMlp if net.cell == "gru" else ra.LstmMlp
        m = cls(eng, net.D, net.A, net.H, net.H2, num_layers=net.L, rnn_bias=net.bias)
    elif row.ctor == "GruLinear":
        cls = ra.GruLinear if net.cell == "gru" else ra.LstmLinear
        m = cls(eng, net.D, net.A, net.H, num_layers=net.L, rnn_bias=net.bias)
    else:
        cls = ra.RnnChain if row.ctor == "RnnChain" else ra.RnnChainWide
        m = cls(eng, net.cell, net.D, net.H, net.A, num_layers=net.L, bias=net.bias, mlp_hidden=net.H2 or None)
    assert m.P == SC.num_params(net), (row.id, m.P)
    return m


def build_env(eng, row, n):
    kind, kw = row.env
    if kind == "chain":
        return ra.ChainEnv(eng, n, **kw)
    if kind == "cartpole":
        return ra.CartPoleEnv(eng, n, **kw)
    if kind == "memory":
        kw = dict(kw)
        return ra.MemoryEnv(eng, n, kw.pop("num_actions"), kw.pop("history_len"), **kw)
    cls = ra.MetaBanditEnv if kind == "meta" else ra.MetaBanditEnvWide
    kw = dict(kw)
    return cls(eng, n, kw.pop("n_arms"), kw.pop("episodes_per_trial"), kw.pop("distribution"), **kw)


_DATA = {}


def case_data(engine, row):
    """the whole-batch planes, advantages and returns of a row, its initial parameters and the fixed tangent: made once
    per session on the session's engine, left unchanged by every user"""
    if row.id in _DATA:
        return _DATA[row.id]
    n, T, D = WORLD * row.lanes, row.T, row.policy.D
    pol, cri = build_module(engine, row, row.policy), build_module(engine, row, row.critic)
    pol.init(row.seeds[0])
    cri.init(row.seeds[1])
    traj = ra.Trajectory(engine, n, T, D)
    if row.env[0] == "history":
        h = R.history(R.Net(*row.policy), n, T, row.env[1])
        traj.write_all(h)
        traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
        traj.write(ra.TRAJ_RETURNS, h["rtg"])
    else:
        env = build_env(engine, row, n)
        assert (env.D, env.A) == (D, row.policy.A), (row.id, env.D, env.A)
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, *row.gae)
        h = traj.read_all()
        h["adv"], h["rtg"] = traj.read(ra.TRAJ_ADVANTAGES), traj.read(ra.TRAJ_RETURNS)
        env.close()
    assert np.abs(h["adv"]).max() > 0 and np.all(np.isfinite(h["adv"])) and np.all(np.isfinite(h["rtg"]))
    d = dict(h=h, p0=pol.get_params(), c0=cri.get_params(), pol=pol, cri=cri, traj=traj,
             v=np.random.default_rng(7).standard_normal(pol.P).astype(np.float32))
    _DATA[row.id] = d
    return d


# ---------------------------------------------------------------------------------------------- f64 references, bars
# family -> (gradient bar, Fisher-vector bar, critic-gradient bar) relative to the vector's largest entry, and where
# each comes from.  "narrow" / "fused": narrow_cases.grad_check's form, GRAD_RTOL + 2 e32 with e32 the f32 oracle's own
# distance from f64 on the same samples (tests/test_gpu_narrow_mlp.py, tests/test_gpu_dqn_update_steps.py).
BARS = {
    # tests/test_gpu_gru.py / test_gpu_lstm.py: GRAD_RTOL = 5e-6; Fisher-vector products 2e-5 AND 4 e32 + 2e-6
    "tile": (5e-6, 2e-5, 5e-6),
    # tests/test_gpu_stacked.py GRAD_RTOL = 5e-6 and 2e-5, taken over by test_gpu_chain_linear.py,
    # test_gpu_seq_multi_action.py and test_gpu_wide_meta.py
    "lane": (5e-6, 2e-5, 5e-6),
    # tests/test_gpu_general_mlp.py test_gradients_and_fisher_vector_products, tests/test_gpu_multi_action.py: 2e-5, 5e-5
    "general": (2e-5, 5e-5, 2e-5),
    "narrow": (nc.GRAD_RTOL, nc.GRAD_RTOL, nc.GRAD_RTOL),
    "fused": (nc.GRAD_RTOL, nc.GRAD_RTOL, nc.GRAD_RTOL),
}
_REFS = {}


def log_softmax_rows(z):
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def references(row, d):
    """f64 policy gradient, Fisher-vector product (reg = 0) of the fixed tangent and critic gradient over ALL lanes, and
    the bar each of the three is held to (a list of bars: every one must hold)"""
    if row.id in _REFS:
        return _REFS[row.id]
    h, p, c, v = d["h"], d["p0"], d["c0"], d["v"]
    B = h["action"].size
    adv64, rtg64 = h["adv"].astype(np.float64), h["rtg"].astype(np.float64)
    bg, bh, bc = ([b] for b in BARS[row.family])
    if row.family == "tile":
        cell = O.CELL_GRU if row.policy.cell == "gru" else O.CELL_LSTM
        pn, cn = row.policy, row.critic  # (a narrow chain: the oracle runs the narrow shape, the device its padded twin)
        ps, cs = O.GruShape(pn.D, pn.H, pn.H2, pn.A, cell), O.GruShape(cn.D, cn.H, cn.H2, cn.A, cell)
        logits, _ = O.gru_seq_forward(ps, p, h, f64=True, want_succ=False)
        dz, _, _ = R.surrogate_dlogits(logits, h["action"], h["adv"])
        g64 = O.gru_seq_backward(ps, p, h, dz, f64=True)
        hv64 = O.gru_policy_fvp(ps, p.astype(np.float64), v.astype(np.float64), h, 0.0, f64=True)
        bh.append(4.0 * rel_err(O.gru_policy_fvp(ps, p, v, h, 0.0), hv64) + 2e-6)
        vv, _ = O.gru_seq_forward(cs, c, h, f64=True, want_succ=False)
        gc64 = O.gru_seq_backward(cs, c, h, 2.0 * (vv - rtg64[None]) / B, f64=True)
    elif row.family == "lane":
        pn, cn = R.Net(*row.policy), R.Net(*row.critic)
        spec, full = R.spec_of(pn), R.to_oracle(pn, p)
        logits, _, _ = S.forward(spec, full, h, want_succ=False)
        dz, _, _ = R.surrogate_dlogits(logits, h["action"], h["adv"])
        g64 = R.restrict(pn, S.backward(spec, full, h, dz))
        hv64 = R.restrict(pn, S.policy_fvp(spec, full, R.to_oracle(pn, v, tangent=True), h, 0.0))
        cspec, cfull = R.spec_of(cn), R.to_oracle(cn, c)
        vv, _, _ = S.forward(cspec, cfull, h, want_succ=False)
        gc64 = R.restrict(cn, S.backward(cspec, cfull, h, 2.0 * (vv - rtg64[None]) / B))
    elif row.family == "general":
        D, hidden, act, A = row.policy
        T = h["action"].shape[0]
        x = h["obs"][:, :T, :].reshape(D, B).T
        a = h["action"].reshape(-1).astype(np.int64)
        pnet, cnet = unflatten(p, D, hidden, A), unflatten(c, D, hidden, 1)
        z, acts = forward64(pnet, x, act)
        pr = np.exp(log_softmax_rows(z))
        g64 = backward64(pnet, x, acts, -adv64.reshape(-1)[:, None] * (np.eye(A)[a] - pr) / B)
        _, tz = jvp64(pnet, unflatten(v, D, hidden, A), x, act)
        hv64 = backward64(pnet, x, acts, pr * (tz - (pr * tz).sum(axis=1, keepdims=True)) / B)
        val, cacts = forward64(cnet, x, act)
        gc64 = backward64(cnet, x, cacts, (2.0 * (val[:, 0] - rtg64.reshape(-1)) / B)[:, None])
    else:
        D, (H,) = row.policy.D, row.policy.hidden
        ps, cs = O.MlpShape(D, H, 2), O.MlpShape(D, H, 1)
        x, a = O.flat_samples(h)
        adv, rtg = np.ascontiguousarray(h["adv"].reshape(-1)), np.ascontiguousarray(h["rtg"].reshape(-1))
        g64, _ = nc.policy_grad64(ps, p, x, a, adv)
        hv64 = nc.policy_fvp64(ps, p, x, v, 0.0)
        gc64, _ = nc.critic_grad64(cs, c, x, rtg)
        bg[0] += 2.0 * rel_err(nc.policy_grad32(ps, p, x, a, adv)[0], g64)
        bh[0] += 2.0 * rel_err(nc.policy_fvp32(ps, p, x, v, 0.0), hv64)
        bc[0] += 2.0 * rel_err(nc.critic_grad32(cs, c, x, rtg)[0], gc64)
    for name, vec in (("g", g64), ("hv", hv64), ("gc", gc64)):
        assert vec.shape == ((len(c),) if name == "gc" else (len(p),)) and np.abs(vec).max() > 0, (row.id, name)
    _REFS[row.id] = dict(g=(g64, bg), hv=(hv64, bh), gc=(gc64, bc))
    return _REFS[row.id]


def check_probe_against_f64(row, sharded, one, refs, report=None):
    """the sharded vectors under the family's bars against f64; the one-rank device error against the same f64 vectors,
    printed beside it.  The sharded run has one more f32 rounding per exchange and another order of the partial sums:
    should that alone take it past a bar, the bar is the larger of the existing one and twice the one-rank error
    measured here (the measured pairs: DESIGN.md §41)."""
    for k in ("g", "hv", "gc"):
        ref, bars = refs[k]
        e_sh, e_one = rel_err(sharded[k], ref), rel_err(one[k], ref)
        print("%s %s: f64 error one rank %.3g, two ranks %.3g (bars %s)" % (row.id, k, e_one, e_sh,
                                                                            ", ".join("%.3g" % b for b in bars)))
        if report is not None:
            report.append((row.id, k, e_one, e_sh, min(bars)))
        for b in bars:
            assert e_one <= b, (row.id, k, "one rank", e_one, b)
            assert e_sh <= max(b, 2.0 * e_one), (row.id, k, "two ranks", e_sh, b, e_one)
    for k in ("loss", "ent", "lc"):  # tests/test_gpu_multirank.py check_probe_vectors
        assert abs(sharded[k] - one[k]) <= 1e-6 * max(1.0, abs(one[k])), (row.id, k, sharded[k], one[k])


# ---------------------------------------------------------------------------------------------- the bodies of a case
def exchanges(eng):
    return eng.profile_read()["allreduce"][1]


def sgd(module):
    return ra.Optimizer(module, ra.optimizer_config_default(ra.OPTIMIZER_SGD))


def values_cfg(target, gamma, steps=SC.CRITIC_STEPS):
    cfg = ra.values_opt_config_default()
    cfg.opt_steps_per_update, cfg.target, cfg.discount_factor = steps, target, gamma
    return cfg


def td_gamma(row):
    return row.gae[0] if row.gae else 0.99


def body_probe(eng, row, pol, cri, traj, d):
    exchanges(eng)
    n = {}
    g, loss, ent = ra.policy_gradient(pol, traj)
    n["policy_gradient"] = exchanges(eng)
    hv = ra.policy_fvp(pol, traj, d["v"], 0.0)
    n["policy_fvp"] = exchanges(eng)
    gc, lc = ra.critic_gradient(cri, traj)
    n["critic_gradient"] = exchanges(eng)
    return dict(g=g, loss=loss, ent=ent, hv=hv, gc=gc, lc=lc, n=n)


def body_first_order(eng, row, pol, cri, traj, d):
    exchanges(eng)
    out, n = {}, {}
    _, out["loss_before_ppo"], _ = ra.policy_gradient(pol, traj)
    exchanges(eng)
    cfg = ra.ppo_config_default()
    cfg.opt_steps_per_update = SC.PPO_STEPS
    st, out["ppo_losses"] = ra.ppo_update(pol, ra.Adam(pol), traj, cfg, want_losses=True)
    n["ppo_update"] = exchanges(eng)
    out["ppo_loss_first"], out["ppo_entropy"], out["ppo_params"] = st.loss_first, st.entropy, pol.get_params()
    pol.set_params(d["p0"])
    st = ra.reinforce_update(pol, sgd(pol), traj)
    n["reinforce_update"] = exchanges(eng)
    out["reinforce_loss"], out["reinforce_entropy"], out["reinforce_params"] = st.loss_first, st.entropy, pol.get_params()
    pol.set_params(d["p0"])
    targets = [("td", ra.VALUE_TARGET_ONE_STEP_TD)]
    if "both_targets" in row.checks:
        targets.append(("rtg", ra.VALUE_TARGET_REWARD_TO_GO))
    for name, target in targets:
        cri.set_params(d["c0"])
        _, out[name + "_losses"] = ra.values_opt_update(cri, ra.Adam(cri), traj, values_cfg(target, td_gamma(row)),
                                                        want_losses=True)
        n["values_opt_update " + name] = exchanges(eng)
        out[name + "_params"] = cri.get_params()
        out[name + "_targets"] = traj.read(ra.TRAJ_TARGETS)
    cri.set_params(d["c0"])
    out["n"] = n
    return out


def body_trpo(eng, row, pol, cri, traj, d):
    exchanges(eng)
    st = ra.trpo_update(pol, traj)
    out = dict(trpo=st.as_dict(), params=pol.get_params(), n=exchanges(eng))
    pol.set_params(d["p0"])
    return out


def body_actor_critic(joint):
    def body(eng, row, pol, cri, traj, d):
        opt = ra.Adam(cri)
        ccfg = values_cfg(ra.VALUE_TARGET_REWARD_TO_GO, 0.99)
        if joint:
            pst, _, losses = ra.actor_critic_update(pol, cri, opt, traj, None, ccfg, want_losses=True)
        else:
            pst = ra.trpo_update(pol, traj)
            _, losses = ra.values_opt_update(cri, opt, traj, ccfg, want_losses=True)
        out = dict(trpo=pst.as_dict(), policy=pol.get_params(), critic=cri.get_params(), losses=losses.copy())
        pol.set_params(d["p0"])
        cri.set_params(d["c0"])
        return out
    return body


def one_rank(engine, row, body):
    """the body on the engine that collected the trajectory: no collective, no exchange"""
    d = case_data(engine, row)
    d["pol"].set_params(d["p0"])
    d["cri"].set_params(d["c0"])
    engine.profile_enable(True)
    try:
        return body(engine, row, d["pol"], d["cri"], d["traj"], d)
    finally:
        engine.profile_read()
        engine.profile_enable(False)


def run_threads(targets, join_s=JOIN_S):
    """one daemon thread per target, joined with a bound: a thread still alive afterwards is a failure, not a wait"""
    threads = [threading.Thread(target=t, daemon=True) for t in targets]
    for t in threads:
        t.start()
    deadline = time.time() + join_s
    for t in threads:
        t.join(timeout=max(0.0, deadline - time.time()))
    assert not [i for i, t in enumerate(threads) if t.is_alive()], "a rank thread did not finish within %g s" % join_s


def two_ranks(row, d, body, env=None):
    """the body on two loopback ranks of `row.lanes` lanes each; returns the two results in rank order"""
    h, n, T = d["h"], row.lanes, row.T
    saved = {k: os.environ.get(k) for k in ("RELEARN_LOOPBACK_COMM", "RELEARN_LOOPBACK_TIMEOUT_MS",
                                            "RELEARN_LOOPBACK_TEST_WEIGHT")}
    os.environ.update(dict(env or {}, RELEARN_LOOPBACK_COMM="1", RELEARN_LOOPBACK_TIMEOUT_MS=GROUP_DEADLINE_MS))
    out = {}
    try:
        uid = ra.comm_unique_id()

        def rank(r):
            owned = []
            try:
                eng = ra.Engine(0)
                owned.append(eng)
                eng.profile_enable(True)
                eng.comm_init(r, WORLD, uid)
                pol, cri = build_module(eng, row, row.policy), build_module(eng, row, row.critic)
                traj = ra.Trajectory(eng, n, T, row.policy.D)
                owned += [pol, cri, traj]
                pol.set_params(d["p0"])
                cri.set_params(d["c0"])
                half = slice(r * n, (r + 1) * n)
                traj.write_all({k: np.ascontiguousarray(h[k][..., half]) for k in ("obs", "action", "reward", "flag",
                                                                                     "term_obs")})
                traj.write(ra.TRAJ_ADVANTAGES, np.ascontiguousarray(h["adv"][:, half]))
                traj.write(ra.TRAJ_RETURNS, np.ascontiguousarray(h["rtg"][:, half]))
                out[r] = body(eng, row, pol, cri, traj, d)
            except BaseException as exc:  # surfaces in the main thread; the peer's barrier ends at the group's deadline
                out[r] = exc
            finally:
                for obj in reversed(owned):
                    try:
                        obj.close()
                    except Exception:
                        pass

        run_threads([lambda r=r: rank(r) for r in range(WORLD)])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for r in range(WORLD):
        if isinstance(out.get(r), BaseException):
            raise out[r]
        assert r in out, "rank %d left no result" % r
    return [out[r] for r in range(WORLD)]


def same_bits(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


# ---------------------------------------------------------------------------------------------- a, b: probe vectors
@pytest.mark.parametrize("row_id", SC.ROW_IDS)
def test_probe_vectors_and_exchange_counts(engine, row_id):
    """rl_policy_gradient, rl_policy_fvp (fixed tangent, reg = 0) and rl_critic_gradient on two ranks: both ranks return
    the same bits, the vectors sit under the family's f64 bars, the scalars agree with one rank's to 1e-6, and every call
    makes the exchanges run_pass prescribes (none on one rank)"""
    row = SC.row(row_id)
    d = case_data(engine, row)
    one = one_rank(engine, row, body_probe)
    ranks = two_ranks(row, d, body_probe)
    for k in ("g", "hv", "gc", "loss", "ent", "lc"):
        assert same_bits(ranks[0][k], ranks[1][k]), (row_id, k)
    check_probe_against_f64(row, ranks[0], one, references(row, d))
    for call in ("policy_gradient", "policy_fvp", "critic_gradient"):
        assert one["n"][call] == 0, (row_id, call, one["n"])
        assert ranks[0]["n"][call] == ranks[1]["n"][call] == SC.prescribed_exchanges(call), (row_id, call, ranks[0]["n"])


# ---------------------------------------------------------------------------------------------- c: first-order updates
def params_close(row, what, got, want):
    """one rank's parameters after the same steps, under the bound the family's one-rank update test holds the device to
    against its restatement; returns what is wrong, or None:
      recurrent rows   tests/test_gpu_gru.py test_ppo_update_recurrent, test_reinforce_and_critic_updates_recurrent (and
                       tests/test_gpu_lstm.py test_ppo_and_critic_updates): 97 % of the entries within 3e-5 — Adam
                       turns a rounding-level difference of a gradient entry near zero into a step of lr either way.
                       The lane-kernel families have no update test against a restatement; they take this one
      feed-forward     tests/test_gpu_narrow_mlp.py test_ppo_update (97 % within 2e-5), test_reinforce_update (99 %
                       within 1e-6), test_values_opt_update_with_td_targets (2e-5 + 1e-3 * steps * 1e-3 on every entry)"""
    diff = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    if row.family in ("tile", "lane"):
        ok, said = np.mean(diff < 3e-5) > 0.97, "share within 3e-5: %.4f" % np.mean(diff < 3e-5)
    elif what == "ppo":
        ok, said = np.mean(diff < 2e-5) > 0.97, "share within 2e-5: %.4f" % np.mean(diff < 2e-5)
    elif what == "reinforce":
        ok, said = np.mean(diff < 1e-6) > 0.99, "share within 1e-6: %.4f" % np.mean(diff < 1e-6)
    else:
        ok, said = diff.max() < 2e-5 + 1e-3 * SC.CRITIC_STEPS * 1e-3, "max %.3g" % diff.max()
    print("%s %s parameters against one rank's: max %.3g, %s" % (row.id, what, diff.max(), said))
    return None if ok else (what + " parameters", said)


def losses_close(row, what, got, want):
    """tests/test_gpu_multirank.py check_sharded_update_against_the_oracles: every step's loss within 1e-5 of one rank's;
    returns what is wrong, or None"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.max(np.abs(got - want) / np.abs(want))
    print("%s %s per-step losses against one rank's: %.3g (%s | %s)" % (row.id, what, err, got, want))
    return None if err < 1e-5 else (what + " losses", err, got, want)


@pytest.mark.parametrize("row_id", SC.ROW_IDS)
def test_first_order_updates(engine, row_id):
    """rl_ppo_update (3 Adam steps; its forward_only init pass exchanges the four sums alone on a recurrent module),
    rl_reinforce_update (SGD) and rl_values_opt_update (3 Adam steps on the one-step-TD target; both targets on the fused
    5-128 and the tile-GRU row): identical replicas, the prescribed exchanges, one rank's losses and parameters.  Every
    figure is printed and every finding gathered before the test fails."""
    row = SC.row(row_id)
    d = case_data(engine, row)
    one = one_rank(engine, row, body_first_order)
    ranks = two_ranks(row, d, body_first_order)
    a, b = ranks
    wrong = []
    for k in a:  # (each rank's targets are those of its own lanes: below)
        if k != "n" and not k.endswith("_targets") and not same_bits(a[k], b[k]):
            wrong.append(("the ranks differ", k))
    if not all(v == 0 for v in one["n"].values()):
        wrong.append(("one rank exchanged", one["n"]))
    want_n = {"ppo_update": SC.prescribed_exchanges("ppo_update", SC.PPO_STEPS),
              "reinforce_update": SC.prescribed_exchanges("reinforce_update"),
              "values_opt_update td": SC.prescribed_exchanges("values_opt_update", SC.CRITIC_STEPS)}
    if "both_targets" in row.checks:
        want_n["values_opt_update rtg"] = SC.prescribed_exchanges("values_opt_update", SC.CRITIC_STEPS)
    if not a["n"] == b["n"] == want_n:
        wrong.append(("exchange counts", a["n"], b["n"], want_n))
    # the first PPO step's ratios are exactly 1 (run_pass on forward_only): its loss is the surrogate's at ratio 1
    print("%s loss of a sharded policy_gradient %r, first PPO loss %r" % (row_id, a["loss_before_ppo"], a["ppo_loss_first"]))
    if not (np.float32(a["ppo_loss_first"]) == np.float32(a["loss_before_ppo"]) == a["ppo_losses"][0]):
        wrong.append(("first PPO loss", a["ppo_loss_first"], a["loss_before_ppo"], a["ppo_losses"][0]))
    wrong.append(losses_close(row, "ppo", a["ppo_losses"], one["ppo_losses"]))
    wrong.append(losses_close(row, "reinforce", [a["reinforce_loss"]], [one["reinforce_loss"]]))
    for k in ("ppo_entropy", "reinforce_entropy"):  # (the scalar bar of check_probe_vectors)
        if not abs(a[k] - one[k]) <= 1e-6 * max(1.0, abs(one[k])):
            wrong.append((k, a[k], one[k]))
    wrong.append(params_close(row, "ppo", a["ppo_params"], one["ppo_params"]))
    wrong.append(params_close(row, "reinforce", a["reinforce_params"], one["reinforce_params"]))
    if same_bits(a["ppo_params"], d["p0"]) or same_bits(a["reinforce_params"], d["p0"]):
        wrong.append(("the policy did not move",))
    for name in ("td", "rtg") if "both_targets" in row.checks else ("td",):
        # the targets come from each rank's own lanes and the critic as it stood: the ranks' planes side by side ARE
        # the one rank's, bit for bit
        both = np.concatenate([ranks[r][name + "_targets"] for r in range(WORLD)], axis=1)
        if not same_bits(both, one[name + "_targets"]):
            wrong.append((name + " targets", np.abs(both - one[name + "_targets"]).max()))
        wrong.append(losses_close(row, "values_opt " + name, a[name + "_losses"], one[name + "_losses"]))
        wrong.append(params_close(row, "critic " + name, a[name + "_params"], one[name + "_params"]))
        if same_bits(a[name + "_params"], d["c0"]):
            wrong.append(("the critic did not move", name))
    wrong = [w for w in wrong if w is not None]
    assert not wrong, (row_id, wrong)


# ---------------------------------------------------------------------------------------------- d: TRPO
@pytest.mark.parametrize("row_id", SC.TRPO_ROWS)
def test_trpo_update(engine, row_id):
    """rl_trpo_update on two ranks: accepted inside the trust region, the iteration count and the sample-weighted scalars
    one rank's, identical replicas, the same number of exchanges on both ranks.  The step itself is not compared: ten f32
    CG iterations amplify the order of the partial sums (tests/test_gpu_multirank.py); the sharp bars are the probe
    vectors'."""
    row = SC.row(row_id)
    d = case_data(engine, row)
    one = one_rank(engine, row, body_trpo)
    a, b = two_ranks(row, d, body_trpo)
    st, st1 = a["trpo"], one["trpo"]
    print("%s TRPO: two ranks %s\n  one rank %s" % (row_id, st, st1))
    assert st["status"] == st1["status"] == ra.OPT_OK
    assert st["cg_iterations"] == st1["cg_iterations"]
    assert abs(st["loss_initial"] - st1["loss_initial"]) < 1e-6 and abs(st["entropy"] - st1["entropy"]) < 1e-6
    assert st["constraint_val_final"] <= ra.trpo_config_default().max_policy_step_kl and st["loss_final"] < st["loss_initial"]
    assert a["trpo"] == b["trpo"] and same_bits(a["params"], b["params"]) and not same_bits(a["params"], d["p0"])
    assert one["n"] == 0 and a["n"] == b["n"] and a["n"] >= 1 + st["cg_iterations"] + 1 + 2


# ---------------------------------------------------------------------------------------------- e: actor_critic_update
@pytest.mark.parametrize("row_id", SC.ACTOR_CRITIC_ROWS)
def test_actor_critic_update_equals_the_two_updates_in_turn(engine, row_id):
    """rl_actor_critic_update with modules off the fused 5-128 pair (chains_can_overlap is false): on two ranks it is
    rl_trpo_update followed by rl_values_opt_update on a second pair of ranks from the same state, bit for bit"""
    row = SC.row(row_id)
    d = case_data(engine, row)
    joint = two_ranks(row, d, body_actor_critic(True))
    split = two_ranks(row, d, body_actor_critic(False))
    for k in ("policy", "critic", "losses"):
        assert same_bits(joint[0][k], joint[1][k]) and same_bits(split[0][k], split[1][k]), (row_id, k)
        assert same_bits(joint[0][k], split[0][k]), (row_id, k)
    assert joint[0]["trpo"] == joint[1]["trpo"] == split[0]["trpo"] == split[1]["trpo"]
    assert joint[0]["trpo"]["status"] == ra.OPT_OK and joint[0]["losses"][-1] < joint[0]["losses"][0]
    assert not same_bits(joint[0]["policy"], d["p0"]) and not same_bits(joint[0]["critic"], d["c0"])


# ---------------------------------------------------------------------------------------------- f: the test of the tests
@pytest.mark.parametrize("row_id", SC.NEGATIVE_ROWS)
def test_a_wrongly_weighted_shard_fails_the_probe_bars(engine, row_id):
    """RELEARN_LOOPBACK_TEST_WEIGHT = "1:1.5" (tests/test_gpu_multirank.py): rank 1's vectors of more than 64 floats enter
    every sum multiplied by 1.5, what a rank that scales by a wrong B contributes.  Both ranks still get the same sums —
    and the gradient, the Fisher-vector product and the critic gradient must each fail the bars of
    check_probe_against_f64"""
    row = SC.row(row_id)
    d = case_data(engine, row)
    assert min(SC.num_params(row.policy), SC.num_params(row.critic)) + 4 > SC.LOOPBACK_SKEW_MIN
    one = one_rank(engine, row, body_probe)
    skewed = two_ranks(row, d, body_probe, env={"RELEARN_LOOPBACK_TEST_WEIGHT": "1:1.5"})
    refs = references(row, d)
    for k in ("g", "hv", "gc"):
        assert same_bits(skewed[0][k], skewed[1][k]), k  # (identical, and identically wrong)
        fair = dict(one, **{k: skewed[0][k]})  # only this vector is the skewed run's: it alone must trip the bars
        with pytest.raises(AssertionError):
            check_probe_against_f64(row, fair, one, refs)
    check_probe_against_f64(row, one, one, refs)  # (and the bars pass what is right)


# ---------------------------------------------------------------------------------------------- the barrier's deadline
def test_a_missing_peer_ends_the_loopback_barrier_at_its_deadline():
    """LoopbackGroup::barrier (relearn_amd/csrc/abi.hip) waits with a deadline (RELEARN_LOOPBACK_TIMEOUT_MS when the
    group is made; 120 s by default): rank 1 of two never calls anything, rank 0's rl_policy_gradient comes back with
    RL_ERR_COMM within seconds, and its engine closes.  Host side only: rank 0 has synchronised its stream before it
    waits, no kernel is in flight."""
    saved = {k: os.environ.get(k) for k in ("RELEARN_LOOPBACK_COMM", "RELEARN_LOOPBACK_TIMEOUT_MS")}
    os.environ.update(RELEARN_LOOPBACK_COMM="1", RELEARN_LOOPBACK_TIMEOUT_MS="500")
    out = {}
    try:
        uid = ra.comm_unique_id()

        def rank0():
            try:
                eng = ra.Engine(0)
                eng.comm_init(0, WORLD, uid)
                pol = ra.Mlp(eng, 5, 17, 2)
                pol.init(2)
                n, T = 8, 3
                rng = np.random.default_rng(0)
                traj = ra.Trajectory(eng, n, T, 5)
                traj.write_all(dict(obs=rng.normal(size=(5, T + 1, n)).astype(np.float32),
                                    action=rng.integers(0, 2, size=(T, n)).astype(np.uint8),
                                    reward=np.ones((T, n), np.float32), flag=np.zeros((T, n), np.uint8),
                                    term_obs=np.zeros((5, T, n), np.float32)))
                traj.write(ra.TRAJ_ADVANTAGES, rng.normal(size=(T, n)).astype(np.float32))
                t0 = time.time()
                try:
                    ra.policy_gradient(pol, traj)
                    out["error"] = None
                except ra.RelearnError as e:
                    out["error"] = (e.code, str(e))
                out["seconds"] = time.time() - t0
                t0 = time.time()
                try:  # the group stays failed: the next collective fails at once
                    ra.policy_gradient(pol, traj)
                    out["again"] = None
                except ra.RelearnError as e:
                    out["again"] = (e.code, str(e), time.time() - t0)
                for obj in (traj, pol, eng):
                    obj.close()
                out["closed"] = True
            except BaseException as exc:
                out["raised"] = exc

        run_threads([rank0, lambda: None], join_s=30.0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert "raised" not in out, out.get("raised")
    assert out["error"] is not None and out["error"][0] == ra.ERR_COMM, out
    assert "loopback collective: a peer did not arrive" in out["error"][1], out
    assert 0.4 <= out["seconds"] < 5.0, out
    assert out["again"] is not None and out["again"][0] == ra.ERR_COMM and out["again"][2] < 0.4, out
    assert out.get("closed") is True
