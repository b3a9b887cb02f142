"""Recurrent chains rolling out on the meta-MDP lanes, against the closed-loop reference of tests/meta_mdp_ref.py (logits
from the oracle's teacher-forced forward over the prefix, the action from the oracle's sampler, the env from the Python
lanes: nothing shared with the kernels).  Every shape of the one-launch table and (3, 3) outside it; both cells, both
tails; 1, 64, 65 and 130 lanes; a lane offset; T = 7 against trials of 3 and 5 steps, so that a trial runs across the two
collections.  All steps in one launch (kernel variant 0; at (3, 3) that is the launch sequence too), the launch sequence
per step (variant 1), and one then the other on one env: whole planes, obs[T] and term_obs included, the observation and
the tables the lanes are left with.  No sample is excused (tests/test_meta_mdp_ref.py holds every margin above 1e-5).
Every test here fails on a library without the constructor."""
import numpy as np
import pytest

import meta_mdp_ref as M
import oracle as O
import relearn_amd as ra
import seq_multi_ref as R

pytestmark = pytest.mark.gpu


def run(engine, c, variants):
    net, d = c.net, c.dist
    try:
        env = ra.MetaMdpEnv(engine, c.n, d.S, d.A, max_inner_steps=d.L, episodes_per_trial=d.E, alpha=d.alpha,
                            reward_prior_mean=d.prior_mean, reward_prior_stddev=d.prior_stddev,
                            reward_stddev=d.reward_stddev, lane_offset=c.offset, seed_env=c.seed + 1,
                            seed_actor=c.seed + 2)
        assert (env.D, env.A) == (net.D, net.A)
        pol = ra.RnnChainWide(engine, net.cell, net.D, net.H, net.A, num_layers=net.L, bias=net.bias,
                              mlp_hidden=net.H2 or None)
        if net.bias:
            pol.init_with(c.seed, bias=R.BIAS_INIT)
        else:
            pol.init(c.seed)
        assert np.array_equal(pol.get_params(), M.closed_params(c))
        traj = ra.Trajectory(engine, c.n, c.T, net.D)
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


@pytest.mark.parametrize("c", M.CLOSED, ids=M.closed_id)
def test_rollout_equals_the_closed_loop_reference(engine, c):
    ref = M.closed_reference(c)
    net = c.net
    z = O.stack_seq_forward(R.shape_of(net), net.L, R.to_oracle(net, M.closed_params(c)), ref.periods[-1],
                            want_succ=False)[0]
    runs = {}
    for what, variants in (("one launch", (0, 0)), ("per step", (1, 1)), ("one launch, then per step", (0, 1))):
        planes, logits, observe, tables = runs[what] = run(engine, c, variants)
        for p in range(M.PERIODS):
            for key in ("action", "reward", "flag", "obs"):
                assert np.array_equal(planes[p][key], ref.periods[p][key]), (what, p, key)
            cut = ref.periods[p]["flag"] == M.INTERRUPT
            assert np.array_equal(planes[p]["term_obs"][:, cut], ref.periods[p]["term_obs"][:, cut]), (what, p)
        assert any((q["flag"] == M.INTERRUPT).any() for q in planes), what
        assert np.array_equal(logits, z), what
        assert np.array_equal(observe, ref.observe), what
        assert np.array_equal(tables[0], ref.tables[0]) and np.array_equal(tables[1], ref.tables[1]), what
    for p in range(M.PERIODS):  # the two against each other: every term_obs entry included
        for key in R.PLANES:
            assert np.array_equal(runs["one launch"][0][p][key], runs["per step"][0][p][key]), (p, key)
