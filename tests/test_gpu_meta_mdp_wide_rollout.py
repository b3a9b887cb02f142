"""Recurrent chains of 15, 19 and 20 inputs (rl_rnn_chain_create_wide20) rolling out on the lanes of
rl_env_create_meta_mdp_wide into trajectories of rl_traj_create_wide, against the closed-loop reference of
tests/meta_mdp_ref.py (logits from the oracle's teacher-forced forward over the prefix, the action from the oracle's
sampler, the env from the Python lanes: nothing shared with the kernels) at the cases of tests/meta_mdp_wide_cases.py.
At (10, 5) — GRU and LSTM, Linear and MLP tail, hidden width 8, 70 lanes and the 45 lanes at offset 25 — three runs: all
steps in one launch (kernel variant 0: k_stack_rollout<.., MetaMdpWideOps, 19, .., 5>), the launch sequence per step
(variant 1), and one then the other on one env; at (9, 2) and (10, 6) variant 0 is the launch sequence too.  T = 7
against trials of 5 steps: a trial runs across the two collections.  Whole planes, obs[T] and term_obs included, the
observation and the tables the lanes are left with.  No sample is excused (tests/test_meta_mdp_wide_cases.py holds every
margin above 1e-5).  Every test here fails on a library without the entry points."""
import numpy as np
import pytest

import meta_mdp_ref as M
import meta_mdp_wide_cases as W
import oracle as O
import relearn_amd as ra
import seq_multi_ref as R

pytestmark = pytest.mark.gpu


def run(engine, c, variants):
    net, d = c.net, c.dist
    try:
        env = ra.MetaMdpEnvWide(engine, c.n, d.S, d.A, max_inner_steps=d.L, episodes_per_trial=d.E, alpha=d.alpha,
                                reward_prior_mean=d.prior_mean, reward_prior_stddev=d.prior_stddev,
                                reward_stddev=d.reward_stddev, lane_offset=c.offset, seed_env=c.seed + 1,
                                seed_actor=c.seed + 2)
        assert (env.D, env.A) == (net.D, net.A)
        pol = ra.RnnChainWide20(engine, net.cell, net.D, net.H, net.A, num_layers=net.L, bias=net.bias,
                                mlp_hidden=net.H2 or None)
        if net.bias:
            pol.init_with(c.seed, bias=R.BIAS_INIT)
        else:
            pol.init(c.seed)
        assert np.array_equal(pol.get_params(), W.closed_params(c))
        traj = ra.TrajectoryWide(engine, c.n, c.T, net.D)
        planes = []
        for variant in variants:
            engine.set_kernel_variant(variant)
            ra.rollout(env, pol, traj)
            planes.append(traj.read_all())
        engine.set_kernel_variant(0)
        logits = pol.seq_forward(traj, want_succ=False)[0]
        return planes, logits, env.observe(), env.read_tables()
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
        planes, logits, observe, tables = runs[what] = run(engine, c, variants)
        for p in range(W.PERIODS):
            for key in ("action", "reward", "flag", "obs"):
                assert np.array_equal(planes[p][key], ref.periods[p][key]), (what, p, key)
            cut = ref.periods[p]["flag"] == M.INTERRUPT
            assert np.array_equal(planes[p]["term_obs"][:, cut], ref.periods[p]["term_obs"][:, cut]), (what, p)
        assert all((q["flag"] == M.INTERRUPT).any() for q in planes), what
        assert np.array_equal(logits, z), what
        assert np.array_equal(observe, ref.observe), what
        assert np.array_equal(tables[0], ref.tables[0]) and np.array_equal(tables[1], ref.tables[1]), what
    for p in range(W.PERIODS):  # the two against each other: every term_obs entry included
        for key in R.PLANES:
            assert np.array_equal(runs["one launch"][0][p][key], runs["per step"][0][p][key]), (p, key)
