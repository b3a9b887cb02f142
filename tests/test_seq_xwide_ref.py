"""The module's reference at 19 and 20 inputs, pinned on the CPU (no device): oracle/stacked.py (f64) — it takes any
width — and the C forward at (D, A) = (19, 5) and (20, 8), both tails, against torch
(tests/golden/torch_golden_seq_xwide.json, made by tests/golden/make_torch_golden_seq_xwide.py), at the bars of
tests/test_seq_multi_ref.py: 1e-11 for outputs, 1e-10 for gradients and Fisher-vector products.  It is what
tests/test_gpu_meta_mdp_wide.py holds the device to at 19 inputs."""
import json
import os

import numpy as np
import pytest

import oracle as O
import seq_multi_ref as R
from oracle import stacked as S
from test_seq_multi_ref import net_of, traj_of

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torch_golden_seq_xwide.json")) as f:
    GOLD = json.load(f)
CASES = [k for k in GOLD if k != "generator"]


def test_the_golden_file_holds_the_cases():
    assert sorted(CASES) == ["gru_l1_linear_d19_a5", "gru_l1_mlp_d20_a8", "lstm_l1_mlp_d19_a5", "lstm_l2_linear_d20_a8"]
    shapes = sorted((GOLD[k]["dims"][0], GOLD[k]["dims"][4], GOLD[k]["dims"][3] == 0) for k in CASES)
    assert shapes == [(19, 5, False), (19, 5, True), (20, 8, False), (20, 8, True)]  # (D, A) with both tails
    assert any(GOLD[k]["dims"][2] == 2 for k in CASES)
    for k in CASES:
        c = GOLD[k]
        flag = np.array(c["flag"]).reshape(c["T"], c["n"])
        assert (flag[:-1] == 1).any() and (flag[:-1] == 2).any() and flag[-1].any()
        assert sorted(set(c["action"])) == list(range(c["dims"][4]))  # every action index


@pytest.mark.parametrize("name", CASES)
def test_stacked_oracle_against_torch(name):
    c = GOLD[name]
    net, traj = net_of(c), traj_of(c)
    A, n, T = net.A, c["n"], c["T"]
    spec = R.spec_of(net)
    params = np.array(c["params"])
    assert params.shape == (R.num_params(net),) and net.D in (19, 20)
    full = R.to_oracle(net, params)
    tol = 1e-11
    out, _, _ = S.forward(spec, full, traj, want_succ=False)
    want_out = np.array(c["out"]).reshape(A, T, n)
    assert np.allclose(out, want_out, rtol=tol, atol=tol)
    dz, _, _ = R.surrogate_dlogits(out, traj["action"], traj["adv"])
    g = R.restrict(net, S.backward(spec, full, traj, dz))
    want = np.array(c["grad"])
    assert np.abs(g - want).max() <= tol * 10 * max(1.0, np.abs(want).max())
    h = R.restrict(net, S.policy_fvp(spec, full, R.to_oracle(net, np.array(c["v"]), tangent=True), traj, 0.0))
    want_h = np.array(c["fvp"])
    assert np.abs(h - want_h).max() <= tol * 10 * max(1.0, np.abs(want_h).max())
    for blk, l, shp, o, _ in R.blocks(net):
        s = slice(o, o + int(np.prod(shp)))
        assert np.abs(want[s]).max() > 0 and np.abs(want_h[s]).max() > 0, (blk, l)
    wih = want[:R.blocks(net)[0][2][0] * net.D].reshape(-1, net.D)
    assert np.all(np.abs(wih).max(0) > 0)  # every one of the 19 or 20 input columns carries gradient
    z32, _ = O.stack_seq_forward(R.shape_of(net), net.L, full.astype(np.float32),
                                 {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in traj.items()},
                                 want_succ=False)
    assert z32.shape == (A, T, n) and np.abs(z32 - want_out).max() < 1e-5 * max(1.0, np.abs(want_out).max())
