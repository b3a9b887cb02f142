"""The module's reference at 23 and 24 inputs, pinned on the CPU (no device): oracle/stacked.py (f64) — it takes any
width — and the C forward at in_dim 23 and 24, two outputs (the partition-game policy) and one (its critic), both cells
and both tails at each output count, against torch (tests/golden/torch_golden_seq_w24.json, made by
tests/golden/make_torch_golden_seq_w24.py), at the bars of tests/test_seq_xwide_ref.py: 1e-11 for outputs, 1e-10 for gradients and Fisher-vector products.  It is what
tests/test_gpu_partition.py holds the device to."""
import json
import os

import numpy as np
import pytest

import oracle as O
import seq_multi_ref as R
from oracle import stacked as S
from test_seq_multi_ref import net_of

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torch_golden_seq_w24.json")) as f:
    GOLD = json.load(f)
CASES = [k for k in GOLD if k != "generator"]
POLICY = [k for k in CASES if GOLD[k]["dims"][4] == 2]
VALUE = [k for k in CASES if GOLD[k]["dims"][4] == 1]


def traj_of(c):
    """test_seq_multi_ref.traj_of for both kinds of case: a value case has targets in the place of actions"""
    D, n, T = c["dims"][0], c["n"], c["T"]
    t = {"obs": np.array(c["obs"]).reshape(D, T + 1, n), "term_obs": np.array(c["term_obs"]).reshape(D, T, n),
         "flag": np.array(c["flag"], dtype=np.uint8).reshape(T, n)}
    if "action" in c:
        t["action"] = np.array(c["action"], dtype=np.uint8).reshape(T, n)
        t["adv"] = np.array(c["adv"]).reshape(T, n)
    else:
        t["target"] = np.array(c["target"]).reshape(T, n)
    return t


def test_the_golden_file_holds_the_cases():
    shapes = sorted((GOLD[k]["dims"][0], GOLD[k]["dims"][4], GOLD[k]["cell"], GOLD[k]["dims"][3] == 0) for k in CASES)
    # 23 and 24 inputs, both cells and both tails at each output count; the experiment's policy and critic: GRU, MLP tail
    assert shapes == [(23, 1, "gru", True), (23, 2, "lstm", True), (24, 1, "gru", False), (24, 1, "lstm", False),
                      (24, 2, "gru", False)]
    assert len(POLICY) == 2 and len(VALUE) == 3
    for k in CASES:
        c = GOLD[k]
        flag = np.array(c["flag"]).reshape(c["T"], c["n"])
        assert (flag[:-1] == 1).any() and (flag[:-1] == 2).any() and flag[-1].any()
    for k in POLICY:
        assert sorted(set(GOLD[k]["action"])) == [0, 1]


def check_blocks(net, want):
    for blk, l, shp, o, _ in R.blocks(net):
        s = slice(o, o + int(np.prod(shp)))
        assert np.abs(want[s]).max() > 0, (blk, l)
    wih = want[:R.blocks(net)[0][2][0] * net.D].reshape(-1, net.D)
    assert np.all(np.abs(wih).max(0) > 0)  # every one of the 23 or 24 input columns carries gradient


def c_forward(net, full, traj):
    t32 = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in traj.items()}
    return O.stack_seq_forward(R.shape_of(net), net.L, full.astype(np.float32), t32, want_succ=False)[0]


@pytest.mark.parametrize("name", POLICY)
def test_stacked_oracle_against_torch_two_outputs(name):
    c = GOLD[name]
    net, traj = net_of(c), traj_of(c)
    A, n, T = net.A, c["n"], c["T"]
    spec = R.spec_of(net)
    params = np.array(c["params"])
    assert params.shape == (R.num_params(net),) and net.D in (23, 24) and A == 2
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
    check_blocks(net, want)
    check_blocks(net, want_h)
    z32 = c_forward(net, full, traj)
    assert z32.shape == (A, T, n) and np.abs(z32 - want_out).max() < 1e-5 * max(1.0, np.abs(want_out).max())


@pytest.mark.parametrize("name", VALUE)
def test_stacked_oracle_against_torch_one_output(name):
    """the critic: values, and the gradient of mean((V - target)^2) through dV = 2 (V - target) / (T n)"""
    c = GOLD[name]
    net, traj = net_of(c), traj_of(c)
    n, T = c["n"], c["T"]
    spec = R.spec_of(net)
    params = np.array(c["params"])
    assert params.shape == (R.num_params(net),) and net.D in (23, 24) and net.A == 1
    full = R.to_oracle(net, params)
    tol = 1e-11
    out, _, _ = S.forward(spec, full, traj, want_succ=False)
    want_out = np.array(c["out"]).reshape(1, T, n)
    assert np.allclose(out, want_out, rtol=tol, atol=tol)
    assert abs(((out[0] - traj["target"]) ** 2).mean() - c["loss"]) <= tol * max(1.0, c["loss"])
    dz = (2.0 * (out[0] - traj["target"]) / (T * n))[None]
    g = R.restrict(net, S.backward(spec, full, traj, dz))
    want = np.array(c["grad"])
    assert np.abs(g - want).max() <= tol * 10 * max(1.0, np.abs(want).max())
    check_blocks(net, want)
    z32 = c_forward(net, full, traj)
    assert z32.shape == (1, T, n) and np.abs(z32 - want_out).max() < 1e-5 * max(1.0, np.abs(want_out).max())
