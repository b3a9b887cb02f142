"""The table of the two-rank tests (tests/sharded_cases.py) checked without a device: equal shards of a world of two,
negative rows whose vectors the loopback collective's test weight can reach, every shape present in the table or test it
is said to come from, and the parameter counts in closed form against the references'."""
import numpy as np

import sharded_cases as SC


def test_rows_are_named_once_and_shard_equally():
    assert len(set(SC.ROW_IDS)) == len(SC.ROWS) == 16
    assert SC.WORLD == 2
    for r in SC.ROWS:
        assert r.lanes > 0 and r.T > 0 and (SC.WORLD * r.lanes) % SC.WORLD == 0, r.id  # the whole batch is 2 x lanes
        assert r.policy.D == r.critic.D and r.critic.A == 1 and r.policy.A >= 2, r.id
        assert (r.gae is None) == (r.env[0] == "history"), r.id
        assert set(r.checks) <= {"trpo", "actor_critic", "both_targets", "negative"}, r.id
    by_family = {f: [r for r in SC.ROWS if r.family == f] for f in ("tile", "lane", "general", "narrow", "fused")}
    assert [len(v) for v in by_family.values()] == [4, 9, 1, 1, 1]
    # the lane counts the families' edges need: one and three tiles; off the wave size on a rank and in the sum
    assert sorted(r.lanes for r in by_family["tile"]) == [32, 32, 32, 96]
    assert all(r.lanes % 64 and (2 * r.lanes) % 64 for r in by_family["lane"])
    assert all(r.lanes == 64 and r.T == 9 for f in ("general", "narrow", "fused") for r in by_family[f])


def test_the_longer_checks_sit_on_their_rows():
    """TRPO on one row of four families, the joint update where the chains cannot overlap, the negatives on one tile-kernel,
    one lane-kernel and the general row, both value targets on the fused pair and the tile GRU"""
    assert SC.TRPO_ROWS == ["tile-gru-32", "stacked-gru-2", "multi-gru-A8", "wide-lstm-16-12"]
    assert SC.ACTOR_CRITIC_ROWS == ["tile-gru-32", "general-16-16-tanh-A4"]
    assert [SC.row(i).family for i in SC.NEGATIVE_ROWS] == ["tile", "lane", "general"]
    assert [r.id for r in SC.ROWS if "both_targets" in r.checks] == ["tile-gru-32", "fused-5-128"]
    for i in SC.ACTOR_CRITIC_ROWS:  # neither is the fused 5-128 pair: chains_can_overlap is false
        assert SC.row(i).family != "fused"


def test_negative_rows_are_above_the_test_weights_threshold():
    """RELEARN_LOOPBACK_TEST_WEIGHT skews vectors of more than 64 floats: the exchanged slices are P + 4 (gradients) and P
    (Fisher-vector products) of the policy and P + 4 of the critic"""
    for i in SC.NEGATIVE_ROWS:
        r = SC.row(i)
        assert SC.num_params(r.policy) > SC.LOOPBACK_SKEW_MIN and SC.num_params(r.critic) + 4 > SC.LOOPBACK_SKEW_MIN, i
    assert SC.num_params(SC.Mlp(5, (1,), "Relu", 2)) + 4 <= SC.LOOPBACK_SKEW_MIN  # (a row that could not be used)


def test_parameter_counts_agree_with_the_references():
    import chain_linear_ref as CL
    import seq_multi_ref as R
    for r in SC.ROWS:
        for m in (r.policy, r.critic):
            if isinstance(m, SC.Net):
                assert SC.num_params(m) == R.num_params(R.Net(*m)), (r.id, m)
                if m.H2 == 0:
                    assert SC.num_params(m) == CL.num_params(m.cell, m.D, m.H, m.L, m.A, m.bias)
    assert SC.num_params(SC.Mlp(5, (128,), "Relu", 2)) == 5 * 128 + 128 + 2 * 128 + 2
    assert SC.num_params(SC.Mlp(7, (16, 16), "Tanh", 4)) == 7 * 16 + 16 + 16 * 16 + 16 + 16 * 4 + 4
    assert SC.num_params(SC.Net("lstm", 5, 128, 1, 128, True, 2)) == 4 * 128 * 5 + 4 * 128 * 128 + 8 * 128 + 128 * 128 + 128 + 2 * 128 + 2


def parametrize_args(test_fn, names):
    """the argument tuples of the pytest.mark.parametrize decorator of `test_fn` whose names are `names`"""
    for mark in test_fn.pytestmark:
        if mark.name == "parametrize" and mark.args[0].replace(" ", "") == names:
            return list(mark.args[1])
    raise AssertionError("%s has no parametrize over %s" % (test_fn.__name__, names))


def test_every_shape_exists_where_it_is_said_to_come_from():
    import chain_linear_ref as CL
    import meta_lanes_ref as M
    import narrow_cases as nc
    import oracle as O
    import seq_multi_ref as R
    import test_gpu_chain_linear
    import test_gpu_gru
    import test_gpu_lstm
    import test_gpu_multi_action
    import test_gpu_multirank
    import test_gpu_seq_multi_action
    import test_gpu_stacked
    import wide_meta_cases as W
    row = SC.row

    def dims(shape):
        return (shape.in_dim, shape.hidden, shape.mlp_hidden, shape.out_dim, shape.cell)

    # tile kernels: the one shape of tests/test_gpu_gru.py / test_gpu_lstm.py, at edge shapes of their lists
    for rid, mod, cell in (("tile-gru-32", test_gpu_gru, O.CELL_GRU), ("tile-gru-96", test_gpu_gru, O.CELL_GRU),
                           ("tile-lstm-32", test_gpu_lstm, O.CELL_LSTM)):
        r = row(rid)
        for net, shape in ((r.policy, mod.PS), (r.critic, mod.CS)):
            assert (net.D, net.H, net.H2, net.A, cell) == dims(shape) and net.L == 1 and net.bias
        assert r.env == SC.CHAIN and r.T == 7
    # the narrow chain that runs on the zero-padded twin: (cell, D, H, H2, A) of tests/test_gpu_gru.py's NARROW, five
    # inputs (Chain lanes), one layer, an MLP tail, two outputs at most — and not the kernels' own 5-128-128
    r = row("tile-gru-narrow-32")
    for net in (r.policy, r.critic):
        assert (net.cell, net.D, net.H, net.H2, net.A) in test_gpu_gru.NARROW and net.L == 1 and net.bias and net.H2 > 0
        assert (net.D, net.H, net.H2) != (5, 128, 128) and net.H <= 128 and net.H2 <= 128 and net.A <= 2
    assert r.env == SC.CHAIN and r.T == 7
    edges = parametrize_args(test_gpu_gru.test_gradients_through_time_at_edge_shapes, "n,T,max_steps")
    assert (96, 7, 3) in edges and any(e[0] == 32 for e in edges)
    assert (96, 7, 3) in parametrize_args(test_gpu_lstm.test_critic_gradient_at_edge_shapes, "n,T,max_steps")
    # lane kernels, stacked: (cell, in_dim, hidden, num_layers, mlp_hidden, out_dim)
    as_stacked = lambda n, A=None: (n.cell, n.D, n.H, n.L, n.H2, n.A if A is None else A)
    assert as_stacked(row("stacked-gru-2").policy) == test_gpu_stacked.SHAPES[0] and row("stacked-gru-2").policy.bias
    nobias = parametrize_args(test_gpu_stacked.test_recurrent_layers_without_bias_vectors, "cell,D,H,NL,H2,A")
    assert as_stacked(row("stacked-lstm-2-nobias").policy) in nobias and not row("stacked-lstm-2-nobias").policy.bias
    assert as_stacked(row("stacked-lstm-2-nobias").critic, 2) == test_gpu_stacked.SHAPES[0]
    # linear head: (cell, in_dim, H, L, A, rnn_bias), and the meta case (cell, H, L, bias, ..., E, arms, ..., seed)
    r = row("linear-gru-meta2")
    p = r.policy
    assert (p.cell, p.D, p.H, p.L, p.A, p.bias) in test_gpu_chain_linear.SHAPES and p.H2 == 0 and r.critic.H2 == 0
    c = CL.META_CASES[0]
    assert (c.cell, c.H, c.L, c.bias, c.E, c.arms) == (p.cell, p.H, p.L, p.bias, r.env[1]["episodes_per_trial"],
                                                        M.UNIFORM_BERNOULLI)
    assert (r.seeds[0], r.env[1]["seed_env"], r.env[1]["seed_actor"]) == (c.seed, c.seed + 1, c.seed + 2)
    assert r.T == 2 * c.E - 1 and r.lanes == 33  # one trial
    # 3..8 actions
    nets = test_gpu_seq_multi_action.NETS
    assert R.Net(*row("multi-gru-A3").policy) == nets[0] and R.Net(*row("multi-gru-A8").policy) == nets[2]
    assert R.Net(*row("multi-lstm-A8").policy) == nets[4]
    assert R.Net(*row("multi-lstm-A3").policy) == R.META_CASES[1].net
    assert sorted((row(i).policy.cell, row(i).policy.A) for i in SC.ROW_IDS if i.startswith("multi-")) == [
        ("gru", 3), ("gru", 8), ("lstm", 3), ("lstm", 8)]
    for i in ("multi-gru-A3", "multi-lstm-A3"):  # k arms: k + 4 features, k actions
        assert row(i).env[1]["n_arms"] == row(i).policy.A == row(i).policy.D - 4
    # wide
    assert R.Net(*row("wide-gru-13-9").policy) == W.NETS[2] and R.Net(*row("wide-lstm-16-12").policy) == W.NETS[4]
    assert R.Net(*row("wide-lstm-16-12").critic)._replace(A=2) == W.CRITICS[1]
    for i in ("wide-gru-13-9", "wide-lstm-16-12"):
        r = row(i)
        assert r.env[1]["n_arms"] == r.policy.A == r.policy.D - 4 and r.T == 2 * r.env[1]["episodes_per_trial"] - 1
    # feed-forward
    g = row("general-16-16-tanh-A4")
    cases = parametrize_args(test_gpu_multi_action.test_gradient_fisher_vector_product_loss_and_kl, "A,L,hidden,act")
    env = g.env[1]
    assert (env["num_actions"], env["history_len"], list(g.policy.hidden), g.policy.act) in cases
    assert g.policy.D == env["num_actions"] + env["history_len"] and g.policy.A == env["num_actions"]
    n = row("narrow-5-17")
    assert (n.policy.D, n.policy.hidden[0]) in nc.SHAPES and n.seeds == nc.MODULE_SEEDS[(5, 17)]
    assert (n.env[1]["seed_env"], n.env[1]["seed_actor"]) == (nc.ROLLOUT_SEEDS["seed_env"], nc.ROLLOUT_SEEDS["seed_actor"])
    f = row("fused-5-128")
    ps = test_gpu_multirank.PS
    assert (f.policy.D, f.policy.hidden[0], f.policy.A) == (ps.in_dim, ps.hidden, ps.out_dim) == (5, 128, 2)


def test_prescribed_exchange_counts():
    assert [SC.prescribed_exchanges(c) for c in ("policy_gradient", "policy_fvp", "critic_gradient", "reinforce_update")] == [
        1, 2, 1, 1]
    assert SC.prescribed_exchanges("ppo_update", 3) == 4 and SC.prescribed_exchanges("values_opt_update", 3) == 3
    assert SC.prescribed_exchanges("critic_update", 5) == 5
    assert np.isscalar(SC.PPO_STEPS) and SC.PPO_STEPS == SC.CRITIC_STEPS == 3
