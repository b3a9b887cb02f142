"""GRU-MLP chains of 6 to 24 inputs with 3 to 12 outputs (GRU 128, MLP [128]: the RL² experiments' default chain as a
categorical policy): their update passes on the tile-resident bf16-pipe kernels with the head in kernels_seq_head_n.hip
(PASS_PATH_RECURRENT_TILE) — gradient, Fisher-vector product and the record-less evaluation against the f64 restatement
oracle/stacked.py at the bars of tests/test_gpu_seq_wide_tile.py and tests/test_gpu_seq_eval_tile.py, against the
lane-per-thread kernels (engine kernel variant 1), and inside one TRPO + critic update.  Output counts: 3 and 12 (the ends
of the head tile's guarded rows), 5 and 10 (the experiments' own).  Every test but the neighbours' fails on a library
without the path, at its path assertion.

Measured on an MI355X: see DESIGN section 55."""
import numpy as np
import pytest

import relearn_amd as ra
import seq_multi_ref as R
from oracle import stacked as S
from test_gpu_partition import module
from test_gpu_seq_eval_tile import bars, evaluated
from test_gpu_seq_wide_tile import FVP_RTOL, biased, history, passes, wide
from test_gpu_stacked import GRAD_RTOL, rel_err

pytestmark = pytest.mark.gpu
SHAPES = [(6, 3), (14, 10), (19, 5), (24, 12)]
RUNS = [(32, 1, False), (32, 2, True), (96, 7, False)]
TILE, LANE = ra.PASS_PATH_RECURRENT_TILE, ra.PASS_PATH_RECURRENT


@pytest.mark.parametrize("n,T,all_end", RUNS)
@pytest.mark.parametrize("D,A", SHAPES)
def test_passes_against_f64(engine, D, A, n, T, all_end):
    pnet, cnet = wide(D, A), wide(D, 1)
    pol, cri = biased(engine, pnet, 41), biased(engine, cnet, 42)
    traj, h = history(engine, pnet, n, T, all_end)
    spec, full = R.spec_of(pnet), R.to_oracle(pnet, pol.get_params())
    logits, _, _ = S.forward(spec, full, h, want_succ=False)
    dz, loss64, ent64 = R.surrogate_dlogits(logits, h["action"], h["adv"])
    g64 = R.restrict(pnet, S.backward(spec, full, h, dz))
    g_d, loss_d, ent_d = ra.policy_gradient(pol, traj)
    assert traj.last_pass_path() == TILE
    v = np.random.default_rng(3).normal(size=pol.P).astype(np.float32)
    h64 = R.restrict(pnet, S.policy_fvp(spec, full, R.to_oracle(pnet, v, tangent=True), h, 1e-5))
    h_d = ra.policy_fvp(pol, traj, v, 1e-5)
    assert traj.last_pass_path() == TILE
    cspec, cfull = R.spec_of(cnet), R.to_oracle(cnet, cri.get_params())
    values, _, _ = S.forward(cspec, cfull, h, want_succ=False)
    d = values[0] - h["rtg"].astype(np.float64)
    c64 = R.restrict(cnet, S.backward(cspec, cfull, h, (2.0 * d / d.size)[None]))
    c_d, closs_d = ra.critic_gradient(cri, traj)
    assert traj.last_pass_path() == TILE
    e_g, e_h, e_c = rel_err(g_d, g64), rel_err(h_d, h64), rel_err(c_d, c64)
    print("D%d A%d %dx%d: gradient %.3g, critic gradient %.3g (bar %.3g), fvp %.3g (bar %.3g)"
          % (D, A, n, T, e_g, e_c, GRAD_RTOL, e_h, FVP_RTOL))
    assert e_g < GRAD_RTOL and e_c < GRAD_RTOL and e_h < FVP_RTOL
    assert abs(loss_d - loss64) <= 2e-5 * abs(loss64) + 1e-7 and abs(ent_d - ent64) <= 2e-5 * abs(ent64) + 1e-7
    assert abs(closs_d - (d * d).mean()) <= 1e-5 * (d * d).mean()
    b1 = 3 * 128 * (D + 128) + 6 * 128 + 128 * 128  # [.., W1, b1 [128], W2 [A][128], b2 [A]]
    w2, b2 = b1 + 128, b1 + 128 + A * 128
    # every row of W2 and every entry of b2 carries gradient, and every entry of b1 whose unit is live on some sample (a
    # unit that is dead on all of them has a gradient of exactly zero in f64 as well)
    assert np.all(np.abs(g_d[w2:b2].reshape(A, 128)).max(1) > 0) and np.all(g_d[b2:] != 0)
    print("  units of u dead on all %d samples: %d of 128" % (n * T, 128 - np.count_nonzero(g64[b1:w2])))
    assert np.array_equal(g_d[b1:w2] != 0, g64[b1:w2] != 0) and np.count_nonzero(g_d[b1:w2]) > 64


@pytest.mark.parametrize("n,T,all_end", RUNS)
@pytest.mark.parametrize("D,A", SHAPES)
def test_evaluation_against_f64_and_the_training_forward(engine, D, A, n, T, all_end):
    net = wide(D, A)
    m = biased(engine, net, 41)
    traj, h = history(engine, net, n, T, all_end)
    spec, p = R.spec_of(net), m.get_params()
    v = np.random.default_rng(3).normal(size=m.P).astype(np.float32)
    moved = (p + 0.01 * v).astype(np.float32)
    logits, _, _ = S.forward(spec, R.to_oracle(net, p), h, want_succ=False)
    z1, _, _ = S.forward(spec, R.to_oracle(net, moved), h, want_succ=False)
    l64, k64 = R.loss_and_kl(z1, logits, h["action"], h["adv"])
    m.set_params(moved)
    loss1, kl1 = ra.policy_loss_kl(m, traj, p)
    assert traj.last_pass_path() == TILE
    bl, bk = bars(l64, k64, logits)
    print("D%d A%d %dx%d: loss off by %.3g (bar %.3g), KL %.6g off by %.3g (bar %.3g)"
          % (D, A, n, T, abs(loss1 - l64), bl, k64, abs(kl1 - k64), bk))
    assert abs(loss1 - l64) <= bl and abs(kl1 - k64) <= bk
    m.set_params(p)  # the record-less forward is the recording forward's arithmetic: ratios of exactly 1
    assert ra.policy_loss_kl(m, traj, p)[1] == 0.0


@pytest.mark.parametrize("T", [20, 33])
def test_block_walks_at_a_second_iteration(T):
    """2048 x 20: 1,280 blocks — more than the head backward's and the tangent's 512 workgroups, two per weight-gradient
    chunk; the head forward's 2,048 workgroups take one block each there.  2048 x 33: 2,112 blocks — the first 64
    workgroups of the head forward, with and without a record, come round a second time on a prefetched operand.  The f64
    restatement is too slow here; the two kernel families are each within the bars of f64, so their distance is held to
    twice the bars"""
    pnet, cnet = wide(24, 12), wide(24, 1)
    g0, h0, c0, path0 = passes(0, pnet, cnet, 2048, T)
    g1, h1, c1, path1 = passes(1, pnet, cnet, 2048, T)
    assert (path0, path1) == (TILE, LANE)
    e_g, e_h, e_c = rel_err(g0, g1), rel_err(h0, h1), rel_err(c0, c1)
    print("2048x%d: variants apart by gradient %.3g, critic gradient %.3g, fvp %.3g" % (T, e_g, e_c, e_h))
    assert e_g < 2 * GRAD_RTOL and e_c < 2 * GRAD_RTOL and e_h < 2 * FVP_RTOL
    (l0, k0), path0, _ = evaluated(0, pnet, 2048, T)
    (l1, k1), path1, logits = evaluated(1, pnet, 2048, T)
    assert (path0, path1) == (TILE, LANE)
    bl, bk = bars(l1, k1, logits)
    print("2048x%d: variants apart by loss %.3g (bar %.3g), KL %.3g (bar %.3g)" % (T, abs(l0 - l1), 2 * bl, abs(k0 - k1), 2 * bk))
    assert abs(l0 - l1) <= 2 * bl and abs(k0 - k1) <= 2 * bk


@pytest.mark.parametrize("what,net,n,variant", [
    ("70 lanes", wide(24, 3), 70, 0), ("lstm", wide(24, 3, cell="lstm"), 64, 0), ("hidden 64", wide(24, 3, H=64), 64, 0),
    ("mlp 64", wide(24, 3, H2=64), 64, 0), ("variant 1", wide(24, 3), 64, 1), ("in_dim 5", wide(5, 3), 64, 0)],
    ids=lambda x: x if isinstance(x, str) else None)
def test_neighbours_keep_their_path(engine, what, net, n, variant):
    try:
        engine.set_kernel_variant(variant)
        traj, _ = history(engine, net, n, 3)
        ra.policy_gradient(module(engine, net, 41), traj)
        assert traj.last_pass_path() == LANE
    finally:
        engine.set_kernel_variant(0)


def test_one_update_on_random_mdp_lanes():
    """TRPO + critic on 64 random-MDP lanes (10 states x 5 actions: 19 features) x 8 steps under both variants: what was
    collected, and the values and advantages rl_gae left, are byte-equal (rollout and values did not move); each update
    descends inside the KL bound, and the accepted candidate's loss and KL equal, bit for bit, an independent evaluation
    at the accepted parameters — a candidate that went through another forward would be about 1e-8 away"""
    runs = []
    for variant in (0, 1):
        eng = ra.Engine(0)
        eng.set_kernel_variant(variant)
        env = ra.MetaMdpEnvWide(eng, 64, 10, 5, 2, 2, seed_env=3, seed_actor=4)
        pol, cri = module(eng, wide(env.D, 5), 31), module(eng, wide(env.D, 1), 32)
        traj = ra.TrajectoryWide(eng, 64, 8, env.D)
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.3)
        planes = traj.read_all()
        planes.update(values=traj.read(ra.TRAJ_VALUES), adv=traj.read(ra.TRAJ_ADVANTAGES))
        p0 = pol.get_params()
        cfg, ccfg = ra.trpo_config_default(), ra.values_opt_config_default()
        ccfg.opt_steps_per_update = 3
        st, cst = ra.actor_critic_update(pol, cri, ra.Adam(cri), traj, cfg, ccfg)
        assert traj.last_pass_path() == (LANE, TILE)[variant == 0]
        assert st.status == ra.OPT_OK and st.loss_final < st.loss_initial and cst.loss_last < cst.loss_first
        assert st.constraint_val_final <= cfg.max_policy_step_kl
        loss, kl = ra.policy_loss_kl(pol, traj, p0)
        assert traj.last_pass_path() == (LANE, TILE)[variant == 0]
        print("variant %d: %d backtracks, loss %.9g / %.9g, KL %.9g / %.9g"
              % (variant, st.num_backtracks, st.loss_final, loss, st.constraint_val_final, kl))
        # the accepted candidate went through the forward pair (record at theta_0, then no record) that this call runs
        assert st.loss_final == loss and st.constraint_val_final == kl
        runs.append((planes, pol.get_params() - p0))
        eng.close()
    assert all(np.array_equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0])
    print("accepted steps: variants apart by %.3g of max |step|" % rel_err(runs[0][1], runs[1][1]))
