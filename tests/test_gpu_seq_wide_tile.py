"""GRU-MLP chains of 6 to 24 inputs at the partition-game experiment's widths (GRU 128, MLP [128], one or two outputs):
their training passes on the tile-resident bf16-pipe kernels with the input side in kernels_seq_in.hip
(PASS_PATH_RECURRENT_TILE), against the f64 restatement oracle/stacked.py at the recurrent tests' bars — gradients 5e-6
of max |g| (GRAD_RTOL), Fisher-vector products 2e-5 — and against the lane-per-thread kernels (engine kernel variant 1),
which share no code with them.  Input widths by where the bias row and the first zero row fall in the 32-row k-block
(6, 8, 23, 24); shapes as in tests/test_gpu_seq_bits.py.  Rollouts, values and GAE stay on the lane-per-thread kernels:
the collected trajectory is byte-equal between the variants.  Every test but the neighbours' fails on a library
without the path."""
import numpy as np
import pytest

import relearn_amd as ra
import seq_multi_ref as R
from oracle import stacked as S
from test_gpu_partition import module, written
from test_gpu_stacked import GRAD_RTOL, rel_err

pytestmark = pytest.mark.gpu
FVP_RTOL = 2e-5


def wide(D, A, cell="gru", H=128, H2=128):
    return R.Net(cell, D, H, 1, H2, True, A)


def biased(engine, net, seed):
    """the module with recurrent bias vectors that are not the default's zeros: the constant row of the k-block counts"""
    m = module(engine, net)
    m.init_with(seed, bias=R.BIAS_INIT)
    return m


def history(engine, net, n, T, all_end=False):
    """a host-written trajectory of T steps (R.history needs two): episode ends staggered across lanes, or everywhere"""
    traj, h = written(engine, net, n, 6, max(T, 2))
    if all_end:
        h["flag"][:] = 1
    if T < 2:
        h = {k: (v[:, :T + 1] if k == "obs" else v[:, :T] if k == "term_obs" else v[:T]) for k, v in h.items()}
        traj = ra.TrajectoryWide24(engine, n, T, net.D)
    traj.write_all(h)
    traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
    traj.write(ra.TRAJ_RETURNS, h["rtg"])
    return traj, h


@pytest.mark.parametrize("n,T,all_end", [(32, 1, False), (32, 2, True), (96, 7, False)])
@pytest.mark.parametrize("D", [6, 8, 23, 24])
def test_passes_against_f64(engine, D, n, T, all_end):
    pnet, cnet = wide(D, 2), wide(D, 1)
    pol, cri = biased(engine, pnet, 41), biased(engine, cnet, 42)
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
    print("D%d %dx%d: gradient %.3g, critic gradient %.3g (bar %.3g), fvp %.3g (bar %.3g)"
          % (D, n, T, e_g, e_c, GRAD_RTOL, e_h, FVP_RTOL))
    assert e_g < GRAD_RTOL and e_c < GRAD_RTOL and e_h < FVP_RTOL
    assert abs(loss_d - loss64) <= 2e-5 * abs(loss64) + 1e-7 and abs(ent_d - ent64) <= 2e-5 * abs(ent64) + 1e-7
    assert abs(closs_d - (d * d).mean()) <= 1e-5 * (d * d).mean()
    for g in (g_d, c_d):  # every input column carries gradient
        assert np.all(np.abs(g[:3 * 128 * D].reshape(-1, D)).max(0) > 0)


def passes(variant, net_p, net_c, n, T):
    eng = ra.Engine(0)
    eng.set_kernel_variant(variant)
    pol, cri = biased(eng, net_p, 41), biased(eng, net_c, 42)
    traj, _ = history(eng, net_p, n, T)
    g = ra.policy_gradient(pol, traj)[0]
    path = traj.last_pass_path()
    v = np.linspace(-1.0, 1.0, pol.P).astype(np.float32)
    out = g, ra.policy_fvp(pol, traj, v, 1e-5), ra.critic_gradient(cri, traj)[0], path
    eng.close()
    return out


def test_block_walks_at_a_second_iteration():
    """1,280 blocks, two per chunk: the f64 restatement is too slow here; the two kernel families are each within the
    bars of f64, so their distance is held to twice the bars"""
    g0, h0, c0, path0 = passes(0, wide(24, 2), wide(24, 1), 2048, 20)
    g1, h1, c1, path1 = passes(1, wide(24, 2), wide(24, 1), 2048, 20)
    assert (path0, path1) == (ra.PASS_PATH_RECURRENT_TILE, ra.PASS_PATH_RECURRENT)
    e_g, e_h, e_c = rel_err(g0, g1), rel_err(h0, h1), rel_err(c0, c1)
    print("2048x20: variants apart by gradient %.3g, critic gradient %.3g, fvp %.3g" % (e_g, e_c, e_h))
    assert e_g < 2 * GRAD_RTOL and e_c < 2 * GRAD_RTOL and e_h < 2 * FVP_RTOL


@pytest.mark.parametrize("what,net,n,variant", [
    ("70 lanes", wide(24, 2), 70, 0), ("lstm", wide(24, 2, cell="lstm"), 64, 0), ("hidden 64", wide(24, 2, H=64), 64, 0),
    ("linear tail", wide(24, 2, H2=0), 64, 0), ("variant 1", wide(24, 2), 64, 1), ("in_dim 5", wide(5, 2), 64, 0)],
    ids=lambda x: x if isinstance(x, str) else None)
def test_neighbours_keep_their_path(engine, what, net, n, variant):
    try:
        engine.set_kernel_variant(variant)
        traj, _ = history(engine, net, n, 3)
        ra.policy_gradient(module(engine, net, 41), traj)
        assert traj.last_pass_path() == ra.PASS_PATH_RECURRENT
    finally:
        engine.set_kernel_variant(0)


def test_one_update_on_partition_lanes():
    """TRPO + critic on 64 PartitionGame lanes x 8 steps at 24 features under both variants: what was collected, and the
    values and advantages rl_gae left, are byte-equal (rollout and values did not move); each update descends"""
    runs = []
    for variant in (0, 1):
        eng = ra.Engine(0)
        eng.set_kernel_variant(variant)
        env = ra.PartitionEnv(eng, 64, max_steps=3, limit=ra.LIMIT_VISIBLE, seed_env=3, seed_actor=4)
        pol, cri = module(eng, wide(24, 2), 31), module(eng, wide(24, 1), 32)
        traj = ra.TrajectoryWide24(eng, 64, 8, 24)
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.999, 0.95)
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
