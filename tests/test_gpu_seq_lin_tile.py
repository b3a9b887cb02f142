"""GRU-Linear chains of 6 to 24 inputs at the RL² experiments' widths (GRU 128 -> ReLU -> Linear(128, A), A = 1 or 3 to
12): their training passes on the tile-resident bf16-pipe kernels with the head in kernels_seq_lin.hip
(PASS_PATH_RECURRENT_TILE), against the f64 restatement oracle/stacked.py at the recurrent tests' bars — gradients 5e-6 of
max |g| (GRAD_RTOL), Fisher-vector products 2e-5 — and against the lane-per-thread kernels (engine kernel variant 1).
Output counts by where the last live row falls in the head's 16-row tile: 3 (the smallest in range), 5 (off the
accumulator's four-row groups), 10 (the bandit experiment's), 12 (the last live row), 1 (the critic: a single live row).
Helpers and shapes are those of tests/test_gpu_seq_wide_tile.py.  Every test but the neighbours' fails on a library
without the path.

Measured on an MI355X over the twelve f64 cases: see DESIGN section 53."""
import numpy as np
import pytest

import relearn_amd as ra
import seq_multi_ref as R
from oracle import stacked as S
from test_gpu_partition import module
from test_gpu_seq_wide_tile import FVP_RTOL, biased, history, passes
from test_gpu_stacked import GRAD_RTOL, rel_err

pytestmark = pytest.mark.gpu


def lin(D, A, cell="gru", H=128):
    return R.Net(cell, D, H, 1, 0, True, A)


@pytest.mark.parametrize("n,T,all_end", [(32, 1, False), (32, 2, True), (96, 7, False)])
@pytest.mark.parametrize("D,A", [(6, 3), (14, 10), (19, 5), (24, 12)])
def test_passes_against_f64(engine, D, A, n, T, all_end):
    pnet, cnet = lin(D, A), lin(D, 1)
    pol, cri = biased(engine, pnet, 41), biased(engine, cnet, 42)  # (the Linear's bias is drawn Uniform: not zero)
    traj, h = history(engine, pnet, n, T, all_end)
    spec, full = R.spec_of(pnet), R.to_oracle(pnet, pol.get_params())
    logits, _, _ = S.forward(spec, full, h, want_succ=False)
    dz, loss64, ent64 = R.surrogate_dlogits(logits, h["action"], h["adv"])
    g64 = R.restrict(pnet, S.backward(spec, full, h, dz))
    g_d, loss_d, ent_d = ra.policy_gradient(pol, traj)
    assert traj.last_pass_path() == ra.PASS_PATH_RECURRENT_TILE
    v = np.random.default_rng(3).normal(size=pol.P).astype(np.float32)
    h64 = R.restrict(pnet, S.policy_fvp(spec, full, R.to_oracle(pnet, v, tangent=True), h, 1e-5))
    h_d = ra.policy_fvp(pol, traj, v, 1e-5)
    assert traj.last_pass_path() == ra.PASS_PATH_RECURRENT_TILE
    cspec, cfull = R.spec_of(cnet), R.to_oracle(cnet, cri.get_params())
    values, _, _ = S.forward(cspec, cfull, h, want_succ=False)
    d = values[0] - h["rtg"].astype(np.float64)
    c64 = R.restrict(cnet, S.backward(cspec, cfull, h, (2.0 * d / d.size)[None]))
    c_d, closs_d = ra.critic_gradient(cri, traj)
    assert traj.last_pass_path() == ra.PASS_PATH_RECURRENT_TILE
    e_g, e_h, e_c = rel_err(g_d, g64), rel_err(h_d, h64), rel_err(c_d, c64)
    print("D%d A%d %dx%d: gradient %.3g, critic gradient %.3g (bar %.3g), fvp %.3g (bar %.3g)"
          % (D, A, n, T, e_g, e_c, GRAD_RTOL, e_h, FVP_RTOL))
    assert e_g < GRAD_RTOL and e_c < GRAD_RTOL and e_h < FVP_RTOL
    assert abs(loss_d - loss64) <= 2e-5 * abs(loss64) + 1e-7 and abs(ent_d - ent64) <= 2e-5 * abs(ent64) + 1e-7
    assert abs(closs_d - (d * d).mean()) <= 1e-5 * (d * d).mean()
    head = 3 * 128 * (D + 128) + 6 * 128  # kernel [a][128], then bias [a]
    for g, a in ((g_d, A), (c_d, 1)):  # every row of the head's kernel and every bias entry carries gradient
        assert np.all(np.abs(g[head:head + a * 128].reshape(a, 128)).max(1) > 0) and np.all(g[head + a * 128:] != 0)


def test_block_walks_at_a_second_iteration():
    """1,280 blocks — more than the head backward's 512 workgroups, two per weight-gradient chunk: the f64 restatement is
    too slow here; the two kernel families are each within the bars of f64, so their distance is held to twice the bars"""
    g0, h0, c0, path0 = passes(0, lin(14, 10), lin(14, 1), 2048, 20)
    g1, h1, c1, path1 = passes(1, lin(14, 10), lin(14, 1), 2048, 20)
    assert (path0, path1) == (ra.PASS_PATH_RECURRENT_TILE, ra.PASS_PATH_RECURRENT)
    e_g, e_h, e_c = rel_err(g0, g1), rel_err(h0, h1), rel_err(c0, c1)
    print("2048x20: variants apart by gradient %.3g, critic gradient %.3g, fvp %.3g" % (e_g, e_c, e_h))
    assert e_g < 2 * GRAD_RTOL and e_c < 2 * GRAD_RTOL and e_h < 2 * FVP_RTOL


@pytest.mark.parametrize("what,net,n,variant", [
    ("70 lanes", lin(24, 3), 70, 0), ("lstm", lin(24, 3, cell="lstm"), 64, 0), ("hidden 64", lin(24, 3, H=64), 64, 0),
    ("variant 1", lin(24, 3), 64, 1), ("in_dim 5", lin(5, 3), 64, 0)], ids=lambda x: x if isinstance(x, str) else None)
def test_neighbours_keep_their_path(engine, what, net, n, variant):
    try:
        engine.set_kernel_variant(variant)
        traj, _ = history(engine, net, n, 3)
        ra.policy_gradient(module(engine, net, 41), traj)
        assert traj.last_pass_path() == ra.PASS_PATH_RECURRENT
    finally:
        engine.set_kernel_variant(0)


def test_one_update_on_meta_bandit_lanes():
    """TRPO + critic on 64 ten-arm meta-bandit lanes x 10 steps under both variants: what was collected, and the values and
    advantages rl_gae left, are byte-equal (rollout and values did not move); each update descends"""
    runs = []
    for variant in (0, 1):
        eng = ra.Engine(0)
        eng.set_kernel_variant(variant)
        env = ra.MetaBanditEnvWide(eng, 64, 10, 3, seed_env=3, seed_actor=4)
        pol, cri = module(eng, lin(env.D, 10), 31), module(eng, lin(env.D, 1), 32)
        traj = ra.Trajectory(eng, 64, 10, env.D)
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.3)
        planes = traj.read_all()
        planes.update(values=traj.read(ra.TRAJ_VALUES), adv=traj.read(ra.TRAJ_ADVANTAGES))
        p0 = pol.get_params()
        ccfg = ra.values_opt_config_default()
        ccfg.opt_steps_per_update = 3
        st, cst = ra.actor_critic_update(pol, cri, ra.Adam(cri), traj, None, ccfg)
        assert st.status == ra.OPT_OK and st.loss_final < st.loss_initial and cst.loss_last < cst.loss_first
        assert traj.last_pass_path() == (ra.PASS_PATH_RECURRENT, ra.PASS_PATH_RECURRENT_TILE)[variant == 0]
        runs.append((planes, pol.get_params() - p0, cst.loss_first))
        eng.close()
    assert all(np.array_equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0])
    print("policy step: variants apart by %.3g of max |step|; first critic loss %.9g, %.9g"
          % (rel_err(runs[0][1], runs[1][1]), runs[0][2], runs[1][2]))
    assert abs(runs[0][2] - runs[1][2]) <= 1e-5 * runs[1][2]
