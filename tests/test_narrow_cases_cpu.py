"""The case table of tests/narrow_cases.py, checked with the oracle alone: the data conditions without which the device
tests of tests/test_gpu_narrow_mlp.py would compare little, and the proof that their comparisons see the fault they are
there for — a hidden unit of the tail lost."""
import numpy as np
import pytest

import narrow_cases as nc
import oracle as O

UPDATE_CASES = [(s, k) for s in nc.SHAPES for k in nc.UPDATE_KINDS]
IDS = ["%s-%s" % (nc.shape_id(s), k) for s, k in UPDATE_CASES]


def dead_units(shape, params, x):
    D, H = shape
    pre = x @ params[:D * H].reshape(H, D).T + params[D * H:D * H + H]
    return [j for j in range(H) if not (pre[:, j] > 0).any()]


def test_the_table_covers_what_it_says():
    assert set(nc.UPDATE_SEEDS) == set(nc.MODULE_SEEDS) == set(nc.SHAPES)
    assert {s for s, _, _ in nc.ROLLOUT_CASES} == set(nc.SHAPES)  # every shape rolls out at G = 16 at least
    assert all(16 in gs for _, _, gs in nc.ROLLOUT_CASES)
    for s in ((5, 15), (5, 100), (5, 127)):
        assert [gs for t, _, gs in nc.ROLLOUT_CASES if t == s] == [(16, 8, 4, 2, 1)]
    assert {(l, gs) for t, l, gs in nc.ROLLOUT_CASES if t == (4, 37)} == {(O.LIMIT_NONE, (16, 8, 1)),
                                                                         (O.LIMIT_LATENT, (16, 8, 1))}
    for s in nc.SHAPES:  # B is no multiple of 8 in at least one update case (here: in both)
        assert any((nc.update_case(s, k)["n"] * nc.update_case(s, k)["T"]) % 8 for k in nc.UPDATE_KINDS)
        assert nc.update_case(s, "ragged")["n"] * nc.update_case(s, "ragged")["T"] == 650
        assert nc.update_case(s, "tiny")["n"] * nc.update_case(s, "tiny")["T"] == 15
        D = 5 if nc.update_case(s, "ragged")["limit"] == O.LIMIT_VISIBLE else 4
        assert D == s[0]


@pytest.mark.parametrize("cus", [256, 304, 228, 64])
def test_one_lane_count_inside_every_group_class(cus):
    """the host rules restated; the lane counts sit inside their class, off its edge, and fill no last wave"""
    lanes = nc.rollout_lanes(cus)
    for G, n in lanes.items():
        assert nc.rollout_group(n, cus) == G and n % 64 != 0
        if G > 1:
            assert nc.rollout_group(n - 41, cus) > G or G == 16  # 41 lanes fewer: the next wider class's last count
    assert nc.dqn_group(nc.dqn_lanes_g8(cus), cus) == 8 and nc.dqn_group(200, cus) == 16
    assert nc.dqn_lanes_g8(cus) % 64 != 0


@pytest.mark.parametrize("shape,limit,groups", nc.ROLLOUT_CASES,
                         ids=["%s-limit%d" % (nc.shape_id(s), l) for s, l, _ in nc.ROLLOUT_CASES])
def test_rollout_cases_reset_and_take_both_actions(shape, limit, groups):
    """at the smallest lane count (the larger ones hold these lanes): both actions in both periods; the step limit's
    Interrupts in both where there is a limit (nine steps: every lane resets), a pole that falls within the eighteen
    steps where there is none"""
    periods = nc.oracle_rollout(shape, limit, 96)
    for want, _ in periods:
        assert set(np.unique(want["action"])) == {0, 1}
        assert limit == O.LIMIT_NONE or (want["flag"] == O.INTERRUPT).any()
    if limit == O.LIMIT_NONE:
        assert (periods[-1][0]["flag"] == O.TERMINATE).any()


@pytest.mark.parametrize("shape,kind", UPDATE_CASES, ids=IDS)
def test_update_cases_hold_their_data_conditions(shape, kind):
    r = nc.oracle_update_case(shape, kind)
    case, D, H = r["case"], shape[0], shape[1]
    flag = r["want"]["flag"]
    assert set(np.unique(r["a"])) == {0, 1}
    assert (flag == O.TERMINATE).any()
    assert case["limit"] == O.LIMIT_NONE or (flag == O.INTERRUPT).any()
    assert np.abs(r["adv"]).max() > 0 and np.abs(r["rtg"]).max() > 0
    # units whose ReLU never fires: the listed ones and no others; every other row of the f32 gradients is non-zero
    for params, table, g, A in ((r["pp"], nc.DEAD_POLICY_UNITS, r["g32"], 2), (r["cp"], nc.DEAD_CRITIC_UNITS, r["c32"], 1)):
        dead = dead_units(shape, params, r["x"])
        assert dead == table[(shape, kind)]
        b = nc.blocks(shape, A)
        gW1, gb1, gW2, gb2 = g[b["W1"]].reshape(H, D), g[b["b1"]], g[b["W2"]].reshape(A, H), g[b["b2"]]
        for j in range(H):
            if j in dead:
                assert not gW1[j].any() and gb1[j] == 0 and not gW2[:, j].any()
            else:
                assert gW1[j].any() and gb1[j] != 0 and gW2[:, j].all(), j
        assert gb2.all()
        if H % 16:
            assert H - 1 not in dead  # the unit test_a_lost_tail_unit_is_seen loses
    assert np.abs(r["hv32"]).min() > 0  # (the regulariser alone sees to that; the product itself: below)
    assert nc.rel_err(r["hv32"], nc.FVP_REG * r["v"].astype(np.float64)) > 1.0


@pytest.mark.parametrize("shape", nc.TAIL_SHAPES, ids=[nc.shape_id(s) for s in nc.TAIL_SHAPES])
def test_a_lost_tail_unit_is_seen(shape):
    """The oracle with the last hidden unit's W2 column zeroed — what a kernel computes that drops the last unit of the
    tail — in the device's place: the rollout takes other actions, the values differ, and the gradient comparisons of
    tests/test_gpu_narrow_mlp.py fail by a wide factor.  Observed (error over bar, over the policy gradient, the
    Fisher-vector product and the critic gradient on both trajectories): 6e5 to 1.2e6 at 5-1, 1.4e5 to 5.4e5 at 5-15,
    2.3e4 to 1.4e5 at 5-17, 7e4 to 1.4e5 at 5-100, 8.8e4 to 3.2e5 at 5-127, 2.2e5 to 7.6e5 at 4-37; asserted: above 100."""
    ps, cs = nc.shapes_of(shape)
    for s, limit, _ in nc.ROLLOUT_CASES:
        if s == shape:
            true = nc.oracle_rollout(shape, limit, 96)
            pp = O.mlp_init(ps, nc.MODULE_SEEDS[shape][0])
            lost = nc.oracle_rollout(shape, limit, 96, params=nc.drop_last_unit(shape, 2, pp))
            assert not np.array_equal(true[0][0]["action"], lost[0][0]["action"])
    for kind in nc.UPDATE_KINDS:
        r = nc.oracle_update_case(shape, kind)
        pl, cl = nc.drop_last_unit(shape, 2, r["pp"]), nc.drop_last_unit(shape, 1, r["cp"])
        v_lost, _, _ = O.lanes_gae(cs, cl, r["want"], nc.GAMMA, nc.LAMBDA)
        assert not np.array_equal(v_lost, r["values"])
        assert not np.array_equal(O.lanes_one_step_targets(cs, cl, r["want"], np.float32(nc.GAMMA)), r["td2d"])
        checks = (("policy gradient", 2, nc.policy_grad32(ps, pl, r["x"], r["a"], r["adv"])[0], r["g32"], r["g64"]),
                  ("fisher-vector product", 2, nc.policy_fvp32(ps, pl, r["x"], r["v"], nc.FVP_REG), r["hv32"], r["hv64"]),
                  ("critic gradient", 1, nc.critic_grad32(cs, cl, r["x"], r["rtg"])[0], r["c32"], r["c64"]))
        for name, A, got, f32, f64 in checks:
            err, e32, bar, failures = nc.grad_check("%s, last unit lost, %s" % (name, kind), shape, A, got, f32, f64)
            print("  -> misses the bar by a factor of %.3g" % (err / bar))
            assert failures and err > 100.0 * bar


@pytest.mark.parametrize("shape", nc.SHAPES, ids=[nc.shape_id(s) for s in nc.SHAPES])
def test_the_clipping_active_rate_clips_on_one_trajectory_of_every_shape(shape):
    """tests/test_gpu_ppo.py's second learning rate is there for the clipped branch: on at least one of a shape's two
    trajectories more than 2 % of the ratios leave [0.8, 1.2] (its own threshold), and the default rate lowers the loss"""
    assert max(nc.oracle_ppo(shape, kind, "clipping-active")[3] for kind in nc.UPDATE_KINDS) > 0.02
    for kind in nc.UPDATE_KINDS:
        losses = nc.oracle_ppo(shape, kind, "default")[1]
        assert losses[-1] < losses[0]
        for targets, steps in (("rtg", 20), ("td", 12)):
            losses = nc.oracle_critic_steps(shape, kind, targets, steps)[1]
            assert losses[-1] < losses[0]


@pytest.mark.parametrize("hidden,limit,seed", nc.DQN_CASES)
def test_a_lost_tail_unit_changes_the_dqn_collection(hidden, limit, seed):
    """the greedy branch of the epsilon-greedy collection reads the whole action-value module: with the last unit lost,
    the lanes end their episodes elsewhere (200 lanes, the seeds of tests/test_gpu_dqn.py's make)"""
    D = 5 if limit == O.LIMIT_VISIBLE else 4
    qs, flags = O.MlpShape(D, hidden, 2), []
    for lost in (False, True):
        sim = O.LaneSim(200, max_steps=nc.DQN_COLLECT["max_steps"], limit=limit, seed_env=21, seed_actor=34)
        q = O.mlp_init(qs, seed)
        osim = O.DqnSim(sim, qs, nc.drop_last_unit((D, hidden), 2, q) if lost else q, nc.DQN_COLLECT["capacity"],
                        [1, 2, 3, 4, 5, 6, 7, 8], 500, gamma=np.float32(0.99))
        f, full = osim.collect(nc.DQN_COLLECT["T"], nc.DQN_COLLECT["eps"])
        assert not full
        flags.append(f)
    assert (flags[0] != 0).any() and not np.array_equal(flags[0], flags[1])
