"""The oracle for recurrent chains over more than two actions, pinned on the CPU (no device): oracle/stacked.py (f64) and
the C forward at A = 3 and A = 8 against torch.nn.GRU / LSTM -> relu -> Linear (-> relu -> Linear)
(tests/golden/torch_golden_seq_multi.json) — logits, the gradient of -mean(adv * ratio) and a Fisher-vector product by
double backward of the mean KL — at the bars tests/test_chain_linear_ref.py uses for the same comparison (1e-11 for
outputs, 1e-10 for gradients); and tests/seq_multi_ref.py against itself: layouts, the per-sample policy terms against
torch autograd, and the margins of the closed-loop rollout cases."""
import json
import os

import numpy as np
import pytest

import meta_lanes_ref as M
import oracle as O
import seq_multi_ref as R
from oracle import stacked as S

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torch_golden_seq_multi.json")) as f:
    GOLD = json.load(f)
CASES = [k for k in GOLD if k != "generator"]


def net_of(c):
    D, H, L, H2, A = c["dims"]
    return R.Net(c["cell"], D, H, L, H2, True, A)


def traj_of(c):
    D, n, T = c["dims"][0], c["n"], c["T"]
    return {"obs": np.array(c["obs"]).reshape(D, T + 1, n), "term_obs": np.array(c["term_obs"]).reshape(D, T, n),
            "flag": np.array(c["flag"], dtype=np.uint8).reshape(T, n),
            "action": np.array(c["action"], dtype=np.uint8).reshape(T, n), "adv": np.array(c["adv"]).reshape(T, n)}


def test_the_golden_file_holds_the_cases():
    assert sorted(CASES) == ["gru_l1_linear_a3", "lstm_l2_mlp_a8"]
    assert sorted(GOLD[k]["dims"][4] for k in CASES) == [3, 8]
    assert any(GOLD[k]["dims"][2] == 2 for k in CASES)  # two layers
    for k in CASES:
        c = GOLD[k]
        flag = np.array(c["flag"]).reshape(c["T"], c["n"])
        assert (flag[:-1] == 1).any() and (flag[:-1] == 2).any() and flag[-1].any()  # episode ends inside and at the horizon
        assert sorted(set(c["action"])) == list(range(c["dims"][4]))  # every action index


@pytest.mark.parametrize("name", CASES)
def test_stacked_oracle_against_torch(name):
    c = GOLD[name]
    net, traj = net_of(c), traj_of(c)
    A, n, T = net.A, c["n"], c["T"]
    spec = R.spec_of(net)
    params = np.array(c["params"])
    assert params.shape == (R.num_params(net),)
    full = R.to_oracle(net, params)
    assert np.array_equal(R.restrict(net, full), params)
    tol = 1e-11
    out, _, _ = S.forward(spec, full, traj, want_succ=False)
    want_out = np.array(c["out"]).reshape(A, T, n)
    assert np.allclose(out, want_out, rtol=tol, atol=tol)
    dz, loss, _ = R.surrogate_dlogits(out, traj["action"], traj["adv"])
    g = R.restrict(net, S.backward(spec, full, traj, dz))
    want = np.array(c["grad"])
    assert np.abs(g - want).max() <= tol * 10 * max(1.0, np.abs(want).max())
    h = R.restrict(net, S.policy_fvp(spec, full, R.to_oracle(net, np.array(c["v"]), tangent=True), traj, 0.0))
    want_h = np.array(c["fvp"])
    assert np.abs(h - want_h).max() <= tol * 10 * max(1.0, np.abs(want_h).max())
    for blk, l, shp, o, _ in R.blocks(net):
        s = slice(o, o + int(np.prod(shp)))
        assert np.abs(want[s]).max() > 0 and np.abs(want_h[s]).max() > 0, (blk, l)
    # the C forward (f32, the contract's fma chains) on the same data: f32 distance from the f64 logits
    z32, _ = O.stack_seq_forward(R.shape_of(net), net.L, full.astype(np.float32),
                                 {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in traj.items()},
                                 want_succ=False)
    assert z32.shape == (A, T, n) and np.abs(z32 - want_out).max() < 1e-5 * max(1.0, np.abs(want_out).max())


def test_layouts():
    for net in (R.Net("gru", 7, 7, 1, 6, True, 3), R.Net("lstm", 8, 9, 2, 0, True, 8), R.Net("gru", 5, 6, 2, 5, False, 5),
                R.Net("lstm", 6, 7, 1, 0, False, 4)):
        G = 4 if net.cell == "lstm" else 3
        P = sum(G * net.H * ((net.D if l == 0 else net.H) + net.H) + (2 * G * net.H if net.bias else 0)
                for l in range(net.L))
        P += net.A * net.H + net.A if net.H2 == 0 else net.H2 * net.H + net.H2 + net.A * net.H2 + net.A
        assert R.num_params(net) == P
        p = np.random.default_rng(1).normal(size=P).astype(np.float32)
        full = R.to_oracle(net, p)
        assert full.dtype == np.float32 and np.array_equal(R.restrict(net, full), p)
        layers, head = R.spec_of(net).unpack(full)
        assert head["W2"].shape[0] == net.A and np.array_equal(head["b2"], p[-net.A:])
        if not net.bias:
            assert not any(w["bih"].any() or w["bhh"].any() for w in layers)
        init = R.init(net, 5)
        assert init.shape == (P,) and np.abs(init[-net.A:]).min() > 0  # the head is drawn at its real A


@pytest.mark.parametrize("A", [3, 8])
def test_policy_terms_against_torch_autograd(A):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(A)
    T, n = 6, 40
    z = rng.normal(size=(A, T, n))
    z0 = z + 0.4 * rng.normal(size=(A, T, n))
    action = rng.integers(0, A, size=(T, n))
    adv = rng.normal(size=(T, n))
    zt = torch.tensor(z, requires_grad=True)
    lp, lp0 = torch.log_softmax(zt, 0), torch.log_softmax(torch.tensor(z0), 0)
    a = torch.tensor(action).unsqueeze(0)
    ratio = torch.exp(torch.gather(lp, 0, a)[0] - torch.gather(lp0, 0, a)[0])
    advt = torch.tensor(adv)
    for clip in (0.2, 0.0):
        loss = -torch.minimum(ratio * advt, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * advt).mean()
        (g,) = torch.autograd.grad(loss, zt, retain_graph=True)
        dz, l64, r64 = R.ppo_dlogits(z, z0, action, adv, clip)
        assert np.allclose(dz, g.numpy(), rtol=1e-12, atol=1e-15) and abs(l64 - loss.item()) < 1e-14
        clipped = (r64 < 1.0 - clip) | (r64 > 1.0 + clip)
        assert clipped.any() and (np.abs(dz).sum(0)[clipped & (np.abs(dz).sum(0) == 0)]).size > 0  # some samples are masked
    loss = -(ratio * advt).mean()
    kl = (torch.exp(lp0) * (lp0 - lp)).sum(0).mean()
    l64, k64 = R.loss_and_kl(z, z0, action, adv)
    assert abs(l64 - loss.item()) < 1e-14 and abs(k64 - kl.item()) < 1e-14
    lpa = torch.gather(lp, 0, a)[0]
    (g,) = torch.autograd.grad(-(torch.exp(lpa - lpa.detach()) * advt).mean(), zt)
    dz, l1, ent = R.surrogate_dlogits(z, action, adv)
    assert np.allclose(dz, g.numpy(), rtol=1e-12, atol=1e-15) and abs(l1 + adv.mean()) < 1e-15
    assert abs(ent - (-(torch.exp(lp) * lp).sum(0).mean()).item()) < 1e-14


def test_histories_use_every_action_index():
    for A in (3, 4, 5, 8):
        h = R.history(R.Net("gru", 5, 7, 1, 6, True, A), 70, 5, A)
        assert sorted(np.unique(h["action"])) == list(range(A))
        assert (h["flag"][-1] == 2).any() and (h["flag"][-1] == 1).any() and (h["flag"][:-1] == 2).any() and (h["flag"][:-1] == 1).any()


@pytest.mark.parametrize("case", R.META_CASES, ids=R.meta_case_id)
def test_meta_rollout_cases_are_decided_by_a_margin(case):
    """every sampled action of the closed-loop reference lies at least 1e-5 from every cumulative boundary (an f32 ulp of a
    probability is 6e-8), so the device's planes can be held to it with no sample excused; every arm is pulled, trials end
    inside both periods, and the reference replays through the env restatement"""
    ref = R.meta_reference(case)
    print("%s: margin %.3g" % (R.meta_case_id(case), ref.margin))
    assert ref.margin >= R.MIN_MARGIN, ref.margin
    k = case.net.A
    action = np.concatenate([p["action"] for p in ref.periods])
    assert sorted(np.unique(action)) == list(range(k))
    lanes = M.MetaLanes(case.n, k, case.E, case.arms, lane_offset=case.offset, seed_env=case.seed + 1)
    for p in ref.periods:
        assert (p["flag"] == M.INTERRUPT).any() and set(np.unique(p["reward"])) <= {0.0, 1.0} and p["reward"].any()
        want = lanes.replay(p["action"])
        for key in ("obs", "reward", "flag", "term_obs"):
            assert np.array_equal(p[key], want[key]), key
    assert np.array_equal(ref.observe, lanes.observe())
