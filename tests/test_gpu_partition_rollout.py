"""Recurrent chains of 23 and 24 inputs (rl_rnn_chain_create_wide24) rolling out on the PartitionGame lanes of
rl_env_create_partition into trajectories of rl_traj_create_wide24, against the closed-loop reference of
tests/partition_ref.py (logits from the oracle's teacher-forced forward over the prefix, the action from the oracle's
sampler, the env from the Python lanes: nothing shared with the kernels) at the cases of tests/partition_cases.py.
At 24 features (a visible limit) — GRU and LSTM, Linear and MLP tail, 64 and 200 lanes, a lane offset — three runs: all
steps in one launch (kernel variant 0: k_stack_rollout<.., PartitionOps, 24, .., 2>), the launch sequence per step
(variant 1), and one then the other on one env; at 23 features variant 0 is the launch sequence too.  T = 7 against
episodes of 3 steps: an episode runs across the two collections.  Whole planes, obs[T] and term_obs included, and the
observation the lanes are left with.  No sample is excused (tests/test_partition_ref.py holds every margin above 1e-5).
Every test here fails on a library without the entry points."""
import numpy as np
import pytest

import oracle as O
import partition_cases as W
import partition_ref as P
import relearn_amd as ra
import seq_multi_ref as R

pytestmark = pytest.mark.gpu


def run(engine, c, variants):
    net = c.net
    try:
        env = ra.PartitionEnv(engine, c.n, max_steps=c.limit.max_steps, limit=c.limit.kind, lane_offset=c.offset,
                              seed_env=c.seed + 1, seed_actor=c.seed + 2)
        assert (env.D, env.A) == (net.D, net.A)
        pol = ra.RnnChainWide24(engine, net.cell, net.D, net.H, net.A, num_layers=net.L, bias=net.bias,
                                mlp_hidden=net.H2 or None)
        if net.bias:
            pol.init_with(c.seed, bias=R.BIAS_INIT)
        else:
            pol.init(c.seed)
        assert np.array_equal(pol.get_params(), W.closed_params(c))
        traj = ra.TrajectoryWide24(engine, c.n, c.T, net.D)
        planes = []
        for variant in variants:
            engine.set_kernel_variant(variant)
            ra.rollout(env, pol, traj)
            planes.append(traj.read_all())
        engine.set_kernel_variant(0)
        logits = pol.seq_forward(traj, want_succ=False)[0]
        return planes, logits, env.observe()
    finally:
        engine.set_kernel_variant(0)


@pytest.mark.parametrize("c", W.CLOSED, ids=W.closed_id)
def test_rollout_equals_the_closed_loop_reference(engine, c):
    ref = W.closed_reference(c)
    net = c.net
    z = O.stack_seq_forward(R.shape_of(net), net.L, R.to_oracle(net, W.closed_params(c)), ref.periods[-1],
                            want_succ=False)[0]
    runs = {}
    for what, variants in (("one launch", (0, 0)), ("per step", (1, 1)), ("one launch, then per step", (0, 1))):
        planes, logits, observe = runs[what] = run(engine, c, variants)
        for p in range(W.PERIODS):
            for key in ("action", "reward", "flag", "obs"):
                assert np.array_equal(planes[p][key], ref.periods[p][key]), (what, p, key)
            cut = ref.periods[p]["flag"] == P.INTERRUPT
            assert np.array_equal(planes[p]["term_obs"][:, cut], ref.periods[p]["term_obs"][:, cut]), (what, p)
        assert all((q["flag"] == P.INTERRUPT).any() == (c.limit.kind != P.LIMIT_NONE) for q in planes), what
        assert np.array_equal(logits, z), what
        assert np.array_equal(observe, ref.observe), what
    for p in range(W.PERIODS):  # the two against each other: every term_obs entry included
        for key in R.PLANES:
            assert np.array_equal(runs["one launch"][0][p][key], runs["per step"][0][p][key]), (p, key)
