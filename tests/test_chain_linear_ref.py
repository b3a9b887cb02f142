"""The reference of the recurrent chains with a Linear tail (tests/chain_linear_ref.py: the module embedded into the
oracle's MLP-tail chain with W1 = I, b1 = 0) pinned without a device: against torch.nn.GRU / LSTM -> relu ->
torch.nn.Linear (tests/golden/torch_golden_chain_linear.json), bit for bit against a direct f32 statement of the head on
the C restatement's own states, the initialisation stream, and the margins of the rollout cases the device tests use."""
import json
import os

import numpy as np
import pytest

import chain_linear_ref as CL
import meta_lanes_ref as M
import meta_rollout_ref as R
import oracle as O
from oracle import stacked as S

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torch_golden_chain_linear.json")) as f:
    GOLD = json.load(f)
CASES = [k for k in GOLD if k != "generator"]
MIN_MARGIN = 1e-5  # as tests/test_meta_rollout_ref.py


def test_the_golden_file_holds_the_cases():
    assert sorted(CASES) == ["gru_l1", "gru_l2", "lstm_l2"]
    for k in CASES:
        assert GOLD[k]["dims"] == [6, 7, 1 if k == "gru_l1" else 2, 2] and (GOLD[k]["n"], GOLD[k]["T"]) == (3, 5)
        flag = np.array(GOLD[k]["flag"]).reshape(5, 3)
        assert (flag[:-1] == 1).any() and (flag[:-1] == 2).any()  # episode ends inside the history


@pytest.mark.parametrize("name", CASES)
def test_embedding_against_torch(name):
    """outputs and successor outputs at 1e-11, the restricted gradient at 1e-10 (the bars of tests/test_oracle_stacked.py
    for the f64 vectors); the embedded gradient's W1, b1 blocks are not compared"""
    c = GOLD[name]
    D, H, L, A = c["dims"]
    n, T = c["n"], c["T"]
    cell = c["cell"]
    spec = CL.spec_of(cell, D, H, L, A)
    traj = {"obs": np.array(c["obs"]).reshape(D, T + 1, n), "term_obs": np.array(c["term_obs"]).reshape(D, T, n),
            "flag": np.array(c["flag"], dtype=np.uint8).reshape(T, n)}
    params = np.array(c["params"])
    assert params.shape == (CL.num_params(cell, D, H, L, A),)
    full = CL.embed(cell, D, H, L, A, True, params)
    assert np.array_equal(CL.restrict(cell, D, H, L, A, True, full), params)
    shp = (A, T, n)
    tol = 1e-11
    out, succ, _ = S.forward(spec, full, traj)
    assert np.allclose(out, np.array(c["out"]).reshape(shp), rtol=tol, atol=tol)
    assert np.allclose(succ, np.array(c["succ_out"]).reshape(shp), rtol=tol, atol=tol)
    assert np.abs(np.array(c["succ_out"])).max() > 0
    g = CL.restrict(cell, D, H, L, A, True, S.backward(spec, full, traj, np.array(c["dout"]).reshape(shp)))
    want = np.array(c["grad"])
    assert np.abs(g - want).max() <= tol * 10 * max(1.0, np.abs(want).max())
    for name_, l, shp_, o, _ in CL.blocks(cell, D, H, L, A):
        assert np.abs(want[o:o + int(np.prod(shp_))]).max() > 0, (name_, l)


def test_layout_and_counts():
    for cell, D, H, L, A, bias in (("gru", 6, 7, 1, 2, True), ("lstm", 5, 36, 2, 1, False), ("gru", 7, 12, 3, 2, True)):
        bl = CL.blocks(cell, D, H, L, A, bias)
        assert [b[0] for b in bl[-2:]] == ["kernel", "bias"] and bl[-2][2] == (A, H) and bl[-1][2] == (A,)
        assert len(bl) == (4 if bias else 2) * L + 2
        P = CL.num_params(cell, D, H, L, A, bias)
        assert bl[-1][3] + A == P == len(CL.index(cell, D, H, L, A, bias))
        p = np.random.default_rng(1).normal(size=P).astype(np.float32)
        full = CL.embed(cell, D, H, L, A, bias, p)
        assert full.dtype == np.float32 and np.array_equal(CL.restrict(cell, D, H, L, A, bias, full), p)
        layers, head = CL.spec_of(cell, D, H, L, A).unpack(full)
        assert np.array_equal(head["W1"], np.eye(H)) and not head["b1"].any()
        assert np.array_equal(head["W2"].reshape(-1), p[bl[-2][3]:bl[-2][3] + A * H]) and np.array_equal(head["b2"], p[-A:])
        if not bias:
            assert not any(w["bih"].any() or w["bhh"].any() for w in layers)
        tang = CL.embed(cell, D, H, L, A, bias, p, tangent=True)
        assert not CL.spec_of(cell, D, H, L, A).unpack(tang)[1]["W1"].any()


@pytest.mark.parametrize("cell,D,H,L,A", [("gru", 6, 7, 1, 2), ("lstm", 8, 33, 2, 1), ("gru", 5, 128, 1, 2)])
def test_embedded_f32_forward_is_the_linear_head_bit_for_bit(cell, D, H, L, A):
    """the C restatement of the embedded chain against the head stated directly: out[q] = bias[q]; out[q] = fma(relu(top[k]),
    kernel[q][k], out[q]), k ascending, in f32, on the top layer's outputs the restatement itself computes (read back
    through an MLP-tail chain whose head is the identity on relu(top): W1 = I, b1 = 0, W2 = I_H rows, b2 = 0)"""
    rng = np.random.default_rng(7)
    n, T = 5, 6
    P = CL.num_params(cell, D, H, L, A)
    p = (rng.uniform(-0.5, 0.5, size=P)).astype(np.float32)
    traj = {"obs": rng.normal(size=(D, T + 1, n)).astype(np.float32),
            "flag": rng.choice(np.array([0, 0, 0, 1, 2], dtype=np.uint8), size=(T, n)),
            "term_obs": rng.normal(size=(D, T, n)).astype(np.float32)}
    out, succ = O.stack_seq_forward(CL.shape_of(cell, D, H, A), L, CL.embed(cell, D, H, L, A, True, p), traj)
    # relu(top) unit by unit: the linear-tail module whose kernel is a row of the identity and whose bias is zero
    kernel, bias = p[-A * H - A:-A].reshape(A, H), p[-A:]
    relu_top = np.zeros((H, T, n), np.float32)
    for k in range(H):
        probe = p[:-A * H - A]
        e = np.zeros(H, np.float32)
        e[k] = 1.0
        pk = np.concatenate([probe, e, np.zeros(1, np.float32)])
        relu_top[k] = O.stack_seq_forward(CL.shape_of(cell, D, H, 1), L, CL.embed(cell, D, H, L, 1, True, pk), traj,
                                          want_succ=False)[0][0]
    assert (relu_top >= 0).all() and (relu_top > 0).any() and (relu_top == 0).any()
    want = np.zeros((A, T, n), np.float32)
    for q in range(A):
        acc = np.full((T, n), bias[q], np.float32)
        for k in range(H):
            # fma in f32: the product of two f32 is exact in f64, and the f64 sum rounded to f32 once is the fused result
            # except at double-rounding ties, which random data does not meet
            acc = (relu_top[k].astype(np.float64) * np.float64(kernel[q, k]) + acc.astype(np.float64)).astype(np.float32)
        want[q] = acc
    assert np.array_equal(out, want)


def test_init_stream():
    """the layers' draws are those of the embedded shape's chain; the Linear's continue the same stream as Linear::new(H,
    A) with fan_in = H + 1 — also stated directly for the default Uniform(FanAvg)"""
    for cell, D, H, L, A, bias in (("gru", 6, 7, 1, 2, True), ("lstm", 5, 36, 2, 1, False), ("gru", 7, 12, 3, 2, True)):
        p = CL.init(cell, D, H, L, A, bias, 17)
        assert p.shape == (CL.num_params(cell, D, H, L, A, bias),)
        emb = O.stack_init(CL.shape_of(cell, D, H, A), L, 17)
        bl = CL.blocks(cell, D, H, L, A, bias)
        for name, l, shp, o, eo in bl[:-2]:
            assert np.array_equal(p[o:o + int(np.prod(shp))], emb[eo:eo + int(np.prod(shp))]), (name, l)
        lim = np.float32(np.sqrt(3.0 * 2.0 / ((H + 1) + A)))
        lin = p[bl[-2][3]:]
        assert np.abs(lin).max() <= lim and np.abs(lin).max() > 0.5 * lim and len(np.unique(lin)) == len(lin)
        # the embedded chain's W1 draws start at the same stream position with another limit: same uniforms, rescaled
        (w1o,) = [o for name, _, _, o in CL.spec_of(cell, D, H, L, A).slices()[0] if name == "W1"]
        lim1 = np.float32(np.sqrt(3.0 * 2.0 / ((H + 1) + H)))
        assert np.allclose(lin[:A * H] / lim, emb[w1o:w1o + A * H] / lim1, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("case", CL.META_CASES, ids=CL.meta_case_id)
def test_rollout_cases_hold_their_margins(case):
    """every sampled action of the closed-loop reference is decided by more than 1e-5, so the device's planes can be held
    to it with no sample excused; the env side replays; the data holds what the cases are there for"""
    ref = CL.meta_reference(case)
    lanes = M.MetaLanes(case.n, R.ARMS, case.E, case.arms, lane_offset=case.offset, seed_env=case.seed + 1)
    for p, planes in enumerate(ref.periods):
        want = lanes.replay(planes["action"])
        for key in ("obs", "reward", "flag", "term_obs"):
            assert np.array_equal(planes[key], want[key]), (p, key)
    print("smallest |u - p0| = %.3g" % ref.margin)
    assert ref.margin >= MIN_MARGIN
    action = np.concatenate([p["action"] for p in ref.periods])
    assert set(np.unique(action)) == {0, 1}
    assert [list(np.flatnonzero((p["flag"] == M.INTERRUPT).all(axis=1))) for p in ref.periods] == \
        R.expected_interrupts(case.T, case.E)
    assert R.expected_interrupts(case.T, case.E)[0] == [4, 9]
    assert case.n == 70  # two workgroups of the rollout kernels
    if case.offset:  # the lanes of a shard are the same lanes of the whole: lanes 25..94 of the 95-lane run at offset 0
        whole = CL.meta_reference(case._replace(n=case.n + case.offset, offset=0))
        for a, b in zip(whole.periods, ref.periods):
            for key in R.PLANES:
                assert np.array_equal(a[key][..., case.offset:], b[key]), key
        assert ref.margin >= whole.margin
    assert sum(1 for c in CL.META_CASES if c.offset == 25) == 1
