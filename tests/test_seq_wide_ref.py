"""The references of the wide meta-bandit lanes and recurrent chains, pinned on the CPU (no device):
  - oracle/stacked.py (f64) and the C forward at (D, A) = (13, 9) and (16, 12), both tails, against torch
    (tests/golden/torch_golden_seq_wide.json, made by tests/golden/make_torch_golden_seq_wide.py), at the bars of
    tests/test_seq_multi_ref.py: 1e-11 for outputs, 1e-10 for gradients and Fisher-vector products;
  - the Python lanes (tests/meta_lanes_ref.py) at 5 and 12 arms: a range of lanes equals the same lanes at a lane
    offset, a trial is 2 E - 1 steps, the features are one-hot over k arms;
  - the lane byte (done, some, action) round-trips for every action 0..11, and is the old byte for actions 0..3;
  - the conditions the case tables of tests/wide_meta_cases.py must meet for the GPU test to excuse no sample."""
import json
import os

import numpy as np
import pytest

import meta_lanes_ref as M
import oracle as O
import relearn_amd as ra
import seq_multi_ref as R
import wide_meta_cases as W
from oracle import stacked as S
from test_seq_multi_ref import net_of, traj_of

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torch_golden_seq_wide.json")) as f:
    GOLD = json.load(f)
CASES = [k for k in GOLD if k != "generator"]


def test_the_golden_file_holds_the_cases():
    assert sorted(CASES) == ["gru_l1_linear_d13_a9", "gru_l1_mlp_d16_a12", "lstm_l1_mlp_d13_a9", "lstm_l2_linear_d16_a12"]
    shapes = sorted((GOLD[k]["dims"][0], GOLD[k]["dims"][4], GOLD[k]["dims"][3] == 0) for k in CASES)
    assert shapes == [(13, 9, False), (13, 9, True), (16, 12, False), (16, 12, True)]  # (D, A) with both tails
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
    assert params.shape == (R.num_params(net),)
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
    z32, _ = O.stack_seq_forward(R.shape_of(net), net.L, full.astype(np.float32),
                                 {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in traj.items()},
                                 want_succ=False)
    assert z32.shape == (A, T, n) and np.abs(z32 - want_out).max() < 1e-5 * max(1.0, np.abs(want_out).max())


# ------------------------------------------------------------------------------------------------ the Python lanes
@pytest.mark.parametrize("k", [5, 12])
@pytest.mark.parametrize("dist", [M.UNIFORM_BERNOULLI, M.ONE_HOT, M.ROUND_ROBIN])
def test_python_lanes_hold_their_lane_range_property(k, dist):
    """lanes 25..39 of a 40-lane run are the 15-lane run at lane offset 25 (the streams are keyed by the global lane);
    a trial is 2 E - 1 steps; the one-hot block of the features is k wide and marks the recorded action"""
    n, E, T = 40, 3, 12
    actions = np.random.default_rng(k).integers(0, k, (T, n)).astype(np.uint8)
    whole = M.MetaLanes(n, k, E, dist, seed_env=9).replay(actions)
    part = M.MetaLanes(n - 25, k, E, dist, lane_offset=25, seed_env=9).replay(actions[:, 25:])
    for key in ("obs", "reward", "flag", "term_obs"):
        assert whole[key].shape[0] in (k + 4, T) and np.array_equal(whole[key][..., 25:], part[key]), key
    want = np.zeros(T, np.uint8)
    want[2 * E - 2::2 * E - 1] = M.INTERRUPT
    assert np.array_equal(whole["flag"], np.repeat(want[:, None], n, axis=1))
    pulls = whole["obs"][0, :-1] == 0.0  # steps that start with no inner episode done: arm pulls
    after = whole["obs"][:, 1:]
    kept = pulls & (whole["flag"] == M.CONTINUE)  # the next observation shows the pull (an Interrupt shows a new trial)
    assert kept.any()
    one_hot = after[2:2 + k][:, kept]
    assert np.array_equal(one_hot.argmax(0), actions[kept]) and np.all(one_hot.sum(0) == 1.0)
    assert sorted(np.unique(actions[kept])) == list(range(k))
    assert set(np.unique(whole["reward"])) == {0.0, 1.0}


def test_lane_byte_round_trips_for_every_action():
    for done in (0, 1):
        for some in (0, 1):
            for action in range(12):  # RL_WIDE_MAX_OUT
                b = W.pack_lane_byte(done, some, action)
                assert 0 <= b < 256 and W.unpack_lane_byte(b) == (done, some, action)
                if action < 4:  # two to four arms: the byte two action bits gave
                    assert b == (done | (some << 1) | (action << 2)) and ((b >> 2) & 3) == action
    assert len({W.pack_lane_byte(d, s, a) for d in (0, 1) for s in (0, 1) for a in range(12)}) == 48


def test_the_library_exports_the_wide_entry_points():
    lib = ra.lib()
    assert hasattr(lib, "rl_env_create_meta_bandit_wide") and hasattr(lib, "rl_rnn_chain_create_wide")
    assert "rl_env_create_meta_bandit_wide" in ra.ABI_SYMBOLS and "rl_rnn_chain_create_wide" in ra.ABI_SYMBOLS
    assert lib.rl_abi_version() == 6
    assert issubclass(ra.MetaBanditEnvWide, ra.MetaBanditEnv) and issubclass(ra.RnnChainWide, ra.RnnChain)


# ------------------------------------------------------------------------------------------------ the case tables
def test_case_tables_cover_the_shapes():
    ks = sorted({c.net.A for c in W.META_CASES})
    assert ks == [5, 9, 10, 12] and all(c.net.D == c.net.A + 4 and c.T == 13 and c.E == 3 for c in W.META_CASES)
    assert {c.n for c in W.META_CASES} == {1, 70} and any(c.offset for c in W.META_CASES)
    for table in (W.NETS, [c.net for c in W.META_CASES]):
        assert {n.cell for n in table} == {"gru", "lstm"} and {n.H for n in table} == {7, 33}
        assert {n.H2 for n in table} == {0, 6} and any(n.L == 2 for n in table) and any(not n.bias for n in table)
    assert sorted({n.A for n in W.NETS}) == [5, 8, 9, 10, 12] and all(n.D == n.A + 4 for n in W.NETS)
    for net in W.NETS + W.CRITICS:
        for n in (1, 70):
            h = R.history(net, n, 5, net.A)
            if n >= net.A:
                assert sorted(np.unique(h["action"])) == list(range(net.A))


@pytest.mark.parametrize("case", W.META_CASES, ids=R.meta_case_id)
def test_meta_rollout_cases_are_decided_by_a_margin(case):
    """every sampled action of the closed-loop reference lies at least R.MIN_MARGIN = 1e-5 from every cumulative boundary
    (an f32 ulp of a probability is 6e-8), so the device's planes are held to it with no sample excused; at 70 lanes every
    arm is pulled; UniformBernoulli cases hold both reward values; the reference replays through the env restatement"""
    ref = R.meta_reference(case)
    print("%s: margin %.3g" % (R.meta_case_id(case), ref.margin))
    assert ref.margin >= R.MIN_MARGIN, ref.margin
    k = case.net.A
    action = np.concatenate([p["action"] for p in ref.periods])
    if case.n >= 70:
        assert sorted(np.unique(action)) == list(range(k))
    lanes = M.MetaLanes(case.n, k, case.E, case.arms, lane_offset=case.offset, seed_env=case.seed + 1)
    for p in ref.periods:
        assert (p["flag"] == M.INTERRUPT).any() and set(np.unique(p["reward"])) <= {0.0, 1.0}
        if case.arms == M.UNIFORM_BERNOULLI:
            assert set(np.unique(p["reward"])) == {0.0, 1.0}
        want = lanes.replay(p["action"])
        for key in ("obs", "reward", "flag", "term_obs"):
            assert np.array_equal(p[key], want[key]), key
    assert np.array_equal(ref.observe, lanes.observe())


def test_every_arm_index_is_sampled_somewhere_in_the_table():
    for k in (5, 9, 10, 12):
        seen = set()
        for case in W.META_CASES:
            if case.net.A == k:
                seen |= set(np.unique(np.concatenate([p["action"] for p in R.meta_reference(case).periods])))
        assert seen == set(range(k)), k


@pytest.mark.parametrize("net,lr", W.PPO_CASES, ids=[R.net_id(c[0]) for c in W.PPO_CASES])
def test_ppo_cases_clip_both_ways_and_away_from_the_bounds(net, lr):
    """the f64 oracle's SGD step of rate `lr` from the case's start: at clip distance 0.2 at least a twentieth of the
    samples are clipped and as many are not, and no ratio lies within 3e-4 of a bound (the GPU test asks 1e-4 of the
    device's own step, which differs from this one by f32 rounding)"""
    h = R.history(net, W.PPO_N, W.PPO_T, W.PPO_HISTORY_SEED)
    spec, p0 = R.spec_of(net), R.init(net, W.PPO_INIT_SEED)
    full0 = R.to_oracle(net, p0.astype(np.float64))
    z0, _, _ = S.forward(spec, full0, h, want_succ=False)
    g = R.restrict(net, S.backward(spec, full0, h, R.surrogate_dlogits(z0, h["action"], h["adv"])[0]))
    p1 = p0.astype(np.float64) - lr * g
    z1, _, _ = S.forward(spec, R.to_oracle(net, p1), h, want_succ=False)
    _, _, ratio = R.ppo_dlogits(z1, z0, h["action"], h["adv"], 0.2)
    clipped = ((h["adv"] > 0) & (ratio > 1.2)) | ((h["adv"] < 0) & (ratio < 0.8))
    margin = min(np.abs(ratio - 0.8).min(), np.abs(ratio - 1.2).min(), np.abs(ratio - 1.0).min())
    print("%s lr %g: %d of %d clipped, nearest ratio to a bound %.3g" % (R.net_id(net), lr, clipped.sum(), ratio.size, margin))
    assert clipped.sum() >= 0.05 * ratio.size and (~clipped).sum() >= 0.05 * ratio.size and margin > 3e-4
