"""The line search's evaluation pass (the second half of rl_policy_loss_kl, the candidates of rl_trpo_update) of GRU chains
of 6 to 24 inputs, MLP and linear tail, on the record-less tile forward (PASS_PATH_RECURRENT_TILE): against the f64
restatement at the bars tests/test_gpu_wide_meta.py holds loss and KL to, against the training forward it must share
its arithmetic with (KL exactly 0 at unmoved parameters), against the lane-per-thread kernels (variant 1), and inside
one TRPO update.  Helpers and shapes are those of tests/test_gpu_seq_wide_tile.py.  Every test but the neighbours'
fails on a library without the path.

Measured on an MI355X: see DESIGN section 54."""
import numpy as np
import pytest

import relearn_amd as ra
import seq_multi_ref as R
from oracle import stacked as S
from test_gpu_partition import module
from test_gpu_seq_wide_tile import biased, history, wide
from test_gpu_stacked import rel_err

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -24
TAILS = [(6, 2, 128), (24, 2, 128), (6, 3, 0), (14, 10, 0), (24, 12, 0)]  # (D, A, MLP width; 0: a linear tail)


def bars(l_ref, k_ref, logits0):
    """tests/test_gpu_wide_meta.py's: loss 2e-5 |l| + 1e-7, KL 2e-4 |k| + the f32 floor of a log-probability difference"""
    floor = 4 * ULP * np.abs(R.log_softmax(np.asarray(logits0, dtype=np.float64))).max(0).mean()
    return 2e-5 * abs(l_ref) + 1e-7, 2e-4 * abs(k_ref) + floor


@pytest.mark.parametrize("n,T,all_end", [(32, 1, False), (32, 2, True), (96, 7, False)])
@pytest.mark.parametrize("D,A,H2", TAILS)
def test_evaluation_against_f64_and_the_training_forward(engine, D, A, H2, n, T, all_end):
    net = wide(D, A, H2=H2)
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
    assert traj.last_pass_path() == ra.PASS_PATH_RECURRENT_TILE
    bl, bk = bars(l64, k64, logits)
    print("D%d A%d H2 %d %dx%d: loss off by %.3g (bar %.3g), KL %.6g off by %.3g (bar %.3g)"
          % (D, A, H2, n, T, abs(loss1 - l64), bl, k64, abs(kl1 - k64), bk))
    assert abs(loss1 - l64) <= bl and abs(kl1 - k64) <= bk
    # the same arithmetic as the forward that left log pi_0: ratios of exactly 1
    m.set_params(p)
    loss0, kl0 = ra.policy_loss_kl(m, traj, p)
    print("  at unmoved parameters: KL %.9g" % kl0)
    assert kl0 == 0.0


def evaluated(variant, net, n, T):
    eng = ra.Engine(0)
    eng.set_kernel_variant(variant)
    m = biased(eng, net, 41)
    traj, _ = history(eng, net, n, T)
    p = m.get_params()
    logits = m.seq_forward(traj, want_succ=False)[0]  # (the f32 lane forward under both variants)
    m.set_params((p + 0.01 * np.linspace(-1.0, 1.0, m.P)).astype(np.float32))
    out = ra.policy_loss_kl(m, traj, p), traj.last_pass_path(), logits
    eng.close()
    return out


@pytest.mark.parametrize("A,H2", [(2, 128), (12, 0)])
def test_block_walk_at_a_second_iteration(A, H2):
    """1,280 blocks: the head kernels' walk comes round a second time; the f64 restatement is too slow here, and the two
    kernel families are each within the bars of f64, so their distance is held to twice the bars"""
    (l0, k0), path0, _ = evaluated(0, wide(24, A, H2=H2), 2048, 20)
    (l1, k1), path1, logits = evaluated(1, wide(24, A, H2=H2), 2048, 20)
    assert (path0, path1) == (ra.PASS_PATH_RECURRENT_TILE, ra.PASS_PATH_RECURRENT)
    bl, bk = bars(l1, k1, logits)
    print("2048x20 A%d: variants apart by loss %.3g (bar %.3g), KL %.3g (bar %.3g)" % (A, abs(l0 - l1), 2 * bl, abs(k0 - k1), 2 * bk))
    assert abs(l0 - l1) <= 2 * bl and abs(k0 - k1) <= 2 * bk


@pytest.mark.parametrize("what,net,n,variant", [
    ("70 lanes", wide(24, 2), 70, 0), ("lstm", wide(24, 2, cell="lstm"), 64, 0), ("hidden 64", wide(24, 2, H=64), 64, 0),
    ("linear tail", wide(24, 2, H2=0), 64, 0), ("variant 1", wide(24, 2), 64, 1), ("in_dim 5", wide(5, 2), 64, 0),
    ("lin 70 lanes", wide(24, 3, H2=0), 70, 0), ("lin lstm", wide(24, 3, cell="lstm", H2=0), 64, 0),
    ("lin hidden 64", wide(24, 3, H=64, H2=0), 64, 0), ("lin variant 1", wide(24, 3, H2=0), 64, 1),
    ("lin in_dim 5", wide(5, 3, H2=0), 64, 0)], ids=lambda x: x if isinstance(x, str) else None)
def test_neighbours_keep_their_path(engine, what, net, n, variant):
    try:
        engine.set_kernel_variant(variant)
        traj, _ = history(engine, net, n, 3)
        m = module(engine, net, 41)
        ra.policy_loss_kl(m, traj, m.get_params())
        assert traj.last_pass_path() == ra.PASS_PATH_RECURRENT
    finally:
        engine.set_kernel_variant(0)


@pytest.mark.parametrize("game", ["partition", "ten arms"])
def test_one_trpo_update(game):
    """64 PartitionGame lanes x 8 steps (MLP tail) / 64 ten-arm meta-bandit lanes x 10 steps (linear tail), default
    max_backtracks, both variants: the accepted candidate's loss and KL are those of an independent evaluation of the
    updated parameters against theta_0 — a candidate launch that ignored the skip flag would have overwritten them"""
    steps = []
    for variant in (0, 1):
        eng = ra.Engine(0)
        eng.set_kernel_variant(variant)
        if game == "partition":
            env = ra.PartitionEnv(eng, 64, max_steps=3, limit=ra.LIMIT_VISIBLE, seed_env=3, seed_actor=4)
            pnet, cnet, traj, lam = wide(24, 2), wide(24, 1), ra.TrajectoryWide24(eng, 64, 8, 24), (0.999, 0.95)
        else:
            env = ra.MetaBanditEnvWide(eng, 64, 10, 3, seed_env=3, seed_actor=4)
            pnet, cnet, traj, lam = wide(env.D, 10, H2=0), wide(env.D, 1, H2=0), ra.Trajectory(eng, 64, 10, env.D), (0.99, 0.3)
        pol, cri = module(eng, pnet, 31), module(eng, cnet, 32)
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, *lam)
        p0 = pol.get_params()
        logits0 = pol.seq_forward(traj, want_succ=False)[0]
        cfg = ra.trpo_config_default()
        st = ra.trpo_update(pol, traj, cfg)
        assert st.status == ra.OPT_OK and st.loss_final < st.loss_initial
        assert st.constraint_val_final <= cfg.max_policy_step_kl
        loss, kl = ra.policy_loss_kl(pol, traj, p0)
        assert traj.last_pass_path() == (ra.PASS_PATH_RECURRENT, ra.PASS_PATH_RECURRENT_TILE)[variant == 0]
        bl, bk = bars(loss, kl, logits0)
        print("%s variant %d: %d backtracks, loss %.8g / %.8g, KL %.6g / %.6g"
              % (game, variant, st.num_backtracks, st.loss_final, loss, st.constraint_val_final, kl))
        assert abs(st.loss_final - loss) <= bl and abs(st.constraint_val_final - kl) <= bk
        steps.append(pol.get_params() - p0)
        eng.close()
    print("accepted steps: variants apart by %.3g of max |step|" % rel_err(steps[0], steps[1]))
