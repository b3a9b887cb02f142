"""A recurrent policy's rollout on the meta-bandit lanes at the shapes where its kernels take other paths
(relearn_amd/csrc/kernels_seq_stack.hip: k_stack_rollout, all steps in one launch = kernel variant 0, and the launch
sequence per step around k_stack_step = variant 1), against the closed-loop reference of tests/meta_rollout_ref.py, which
is built from seeds alone and shares no code with either: whole planes, every lane, every step, two collections in a
row, no sample excused (tests/test_meta_rollout_ref.py holds every sampled action's margin above 1e-5)."""
import numpy as np
import pytest

import meta_lanes_ref as M
import meta_rollout_ref as R
import oracle as O
import relearn_amd as ra

pytestmark = pytest.mark.gpu


def build(engine, case):
    env = ra.MetaBanditEnv(engine, case.n, R.ARMS, case.E, case.arms, lane_offset=case.offset, seed_env=case.seed + 1,
                           seed_actor=case.seed + 2)
    assert (env.D, env.A) == (R.D, R.ARMS)
    cls = ra.GruMlp if case.cell == "gru" else ra.LstmMlp
    pol = cls(engine, R.D, R.ARMS, case.H, case.H2, num_layers=case.L, rnn_bias=case.bias)
    if case.bias:
        pol.init_with(case.seed, bias=R.BIAS_INIT)
    else:
        pol.init(case.seed)
    assert np.array_equal(pol.get_params(), R.case_params(case))
    return env, pol, ra.Trajectory(engine, case.n, case.T, R.D)


def run(engine, case, variants):
    """one env, one trajectory, one collection per entry of `variants`"""
    try:
        env, pol, traj = build(engine, case)
        planes = []
        for variant in variants:
            engine.set_kernel_variant(variant)
            ra.rollout(env, pol, traj)
            planes.append(traj.read_all())
        engine.set_kernel_variant(0)
        logits = pol.seq_forward(traj, want_succ=False)[0]
        observe = env.observe()
        driven = env.step(R.driven_actions(case.n))
    finally:
        engine.set_kernel_variant(0)
    return planes, logits, observe, driven


def against_reference(case, got, ref, what):
    planes, logits, observe, driven = got
    for p in range(R.PERIODS):
        for key in ("action", "reward", "flag", "obs"):
            assert np.array_equal(planes[p][key], ref.periods[p][key]), (what, p, key)
        cut = ref.periods[p]["flag"] == M.INTERRUPT
        assert np.array_equal(planes[p]["term_obs"][:, cut], ref.periods[p]["term_obs"][:, cut]), (what, p)
    R.check_data(case, planes)
    full = R.expand_params(case.cell, case.H, case.L, case.H2, case.bias, R.case_params(case))
    z = O.stack_seq_forward(R.shape_of(case.cell, case.H, case.H2), case.L, full, ref.periods[-1], want_succ=False)[0]
    assert np.array_equal(logits, z), what
    assert np.array_equal(observe, ref.observe), what
    reward, flag, obs, term = driven
    reward_r, flag_r, obs_r, term_r = ref.driven
    assert np.array_equal(reward, reward_r) and np.array_equal(flag, flag_r) and np.array_equal(obs, obs_r), what
    assert np.array_equal(term[:, flag_r == M.INTERRUPT], term_r[:, flag_r == M.INTERRUPT]), what


@pytest.mark.parametrize("case", R.GRID, ids=R.case_id)
def test_rollout_against_the_closed_loop_reference(engine, case):
    ref = R.reference(case)
    fused = run(engine, case, (0, 0))
    stepwise = run(engine, case, (1, 1))
    against_reference(case, fused, ref, "one launch")
    against_reference(case, stepwise, ref, "per step")
    for p in range(R.PERIODS):  # the two against each other: every term_obs entry included
        for key in R.PLANES:
            assert np.array_equal(fused[0][p][key], stepwise[0][p][key]), (p, key)
    # period 0 in one launch, period 1 per step: the one launch stores back all that the launches per step read
    against_reference(case, run(engine, case, (0, 1)), ref, "one launch, then per step")
    if case.offset:  # the lanes of a shard are the same lanes of the whole
        whole = R.reference(case, n=case.n + case.offset, offset=0)
        for p in range(R.PERIODS):
            for key in ("obs", "action", "reward", "flag"):
                assert np.array_equal(fused[0][p][key], whole.periods[p][key][..., case.offset:]), (p, key)
