"""Wide feed-forward modules (9 to 24 inputs) with one hidden layer of 65 to 128 units: the fused passes of
relearn_amd/csrc/kernels_wide_split.hip — a 32-sample tile shared by a team of waves, each owning part of the hidden layer —
against torch float64 autograd, with the helpers and the bars of tests/test_gpu_wide_mlp.py, and Trajectory.last_pass_path()
(rl_traj_last_pass_path) as the witness of which kernel family ran.  Every test here fails on a library without that entry point;
with it but without the kernel the three test_split_* tests fail at their path assertion."""
import numpy as np
import pytest

import relearn_amd as ra
from test_gpu_wide_mlp import CLIP, LR, close, critic64, history, logit_bound, policy64, setup, sgd_ppo

pytestmark = pytest.mark.gpu

# (in_dim, hidden, activation, bias, n, T): 99 samples are four tiles, the last with three live samples (the base); a third
# unit tile with one live unit and an empty fourth; a width on a tile edge and one past it; the bias row in the first k-step
# of layer 0, as first row of the second, and inside it; one ragged tile (every other team of the workgroup walks on zeros)
CASES = [(24, [128], "Relu", True, 33, 3), (24, [65], "Relu", True, 33, 3), (24, [96], "Relu", True, 33, 3),
         (24, [97], "Tanh", True, 33, 3), (9, [128], "Relu", True, 33, 3), (16, [128], "Relu", True, 33, 3),
         (17, [128], "Tanh", True, 33, 3), (24, [128], "Relu", True, 8, 3)]
IDS = ["%d-%d-%s-%dx%d" % (c[0], c[1][0], c[2], c[4], c[5]) for c in CASES]
GM_FLUSH, TEAMS_PER_WG = 64, 2  # gen_mfma_common.hpp, kernels_wide_split.hip


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_split_passes_against_f64(engine, c):
    pol, cri, traj, x, a, adv, rtg = setup(engine, c)
    p0 = pol.get_params()
    vec = np.random.default_rng(5).normal(size=p0.size).astype(np.float32)
    moved = (p0 + 0.01 * vec).astype(np.float32)
    r0, r1 = policy64(c, p0, p0, x, a, adv, vec), policy64(c, moved, p0, x, a, adv)
    assert close("logits", pol.forward(x), r0["z"], 0.0, logit_bound(c, p0, x))
    g, loss, ent = ra.policy_gradient(pol, traj)
    assert traj.last_pass_path() == ra.PASS_PATH_WIDE_SPLIT
    assert close("gradient", g, r0["grad"], 2e-5, 1e-9)
    assert abs(loss - r0["loss"]) <= 2e-5 * abs(r0["loss"]) + 1e-7 and abs(ent - r0["entropy"]) <= 2e-5 * r0["entropy"] + 1e-7
    assert close("fvp", ra.policy_fvp(pol, traj, vec, 0.0), r0["fvp"], 5e-5, 0.0)
    assert close("fvp + damping", ra.policy_fvp(pol, traj, vec, 1e-5), r0["fvp"] + 1e-5 * vec.astype(np.float64), 5e-5, 0.0)
    pol.set_params(moved)
    loss1, kl1 = ra.policy_loss_kl(pol, traj, p0)
    assert abs(loss1 - r1["loss"]) <= 2e-5 * abs(r1["loss"]) + 1e-7 and abs(kl1 - r1["kl"]) <= 2e-4 * r1["kl"] + 1e-8
    # the clipped PPO gradient read back from one and two SGD steps, as in test_passes_against_f64
    p1, p2 = sgd_ppo(engine, pol, traj, p0, 1), sgd_ppo(engine, pol, traj, p0, 2)
    gp = policy64(c, p1.astype(np.float32), p0, x, a, adv, clip=CLIP)["grad"]
    diff = np.abs((p1 - p2) / LR - gp) - 2.0 ** -24 * (np.abs(p2) + LR * np.abs(gp)) / LR
    print("ppo gradient: max error beyond the readback %.3e, bound %.3e" % (diff.max(), 2e-5 * np.abs(gp).max() + 1e-9))
    assert diff.max() <= 2e-5 * np.abs(gp).max() + 1e-9
    closs, cgrad = critic64(c, cri.get_params(), x, rtg)
    cg, cl = ra.critic_gradient(cri, traj)
    assert traj.last_pass_path() == ra.PASS_PATH_WIDE_SPLIT
    assert close("critic gradient", cg, cgrad, 5e-6, 0.0) and abs(cl - closs) <= 1e-5 * closs


def test_split_flushes_and_adds(engine):
    """enough tiles that every team flushes after GM_FLUSH of them and one team adds a tile's gradient to its slab row
    behind that; the f64 gradient (a mean) is summed over slices of the samples"""
    T = 33
    B_min = 32 * (GM_FLUSH * engine.info()[2] * TEAMS_PER_WG + 1)
    c = (24, [65], "Relu", True, -(-B_min // T), T)
    pol, cri, traj, x, a, adv, rtg = setup(engine, c)
    p0, c0, B = pol.get_params(), cri.get_params(), len(a)
    want, cwant = np.zeros(p0.size), np.zeros(c0.size)
    for s in range(0, B, 1 << 17):
        e = min(B, s + (1 << 17))
        want += policy64(c, p0, p0, x[s:e], a[s:e], adv[s:e])["grad"] * ((e - s) / B)
        cwant += critic64(c, c0, x[s:e], rtg[s:e])[1] * ((e - s) / B)
    g = ra.policy_gradient(pol, traj)[0]
    assert traj.last_pass_path() == ra.PASS_PATH_WIDE_SPLIT
    assert close("gradient", g, want, 2e-5, 1e-9)
    assert close("critic gradient", ra.critic_gradient(cri, traj)[0], cwant, 5e-6, 0.0)


@pytest.mark.parametrize("hidden, bias, variant, path", [([64], True, 0, "WIDE_MFMA"), ([33, 64], True, 0, "PER_LAYER"),
                                                         ([128], False, 0, "PER_LAYER"), ([128], True, 1, "PER_LAYER")])
def test_paths_elsewhere_are_what_they_were(engine, hidden, bias, variant, path):
    engine.set_kernel_variant(variant)
    try:
        pol, _, traj = setup(engine, (24, hidden, "Relu", bias, 33, 3))[:3]
        assert traj.last_pass_path() == ra.PASS_PATH_NONE
        ra.policy_gradient(pol, traj)
        assert traj.last_pass_path() == getattr(ra, "PASS_PATH_" + path)
    finally:
        engine.set_kernel_variant(0)


def test_split_update_agrees_with_per_layer(engine):
    """one TRPO step with 2 CG iterations and 2 Adam critic steps: the split kernel against the per-layer kernels, at the
    bars of test_update_steps_agree_between_the_variants"""
    got = []
    for variant in (0, 1):
        engine.set_kernel_variant(variant)
        try:
            pol, cri, traj = setup(engine, CASES[0])[:3]
            p0, c0 = pol.get_params(), cri.get_params()
            cfg = ra.trpo_config_default()
            cfg.iterations = 2
            st = ra.trpo_update(pol, traj, cfg)
            cst = ra.critic_update(cri, ra.Adam(cri), traj, 2)
            assert traj.last_pass_path() == (ra.PASS_PATH_PER_LAYER if variant else ra.PASS_PATH_WIDE_SPLIT)
            got.append((st, pol.get_params(), cst, cri.get_params()))
        finally:
            engine.set_kernel_variant(0)
    (s0, p_0, c_0, q_0), (s1, p_1, c_1, q_1) = got
    assert s0.status == s1.status == ra.OPT_OK and s0.num_backtracks == s1.num_backtracks
    assert s0.cg_iterations == s1.cg_iterations == 2
    assert np.abs(p_0 - p_1).max() <= 2e-3 * np.abs(p_1 - p0).max() + 1e-7
    assert abs(c_0.loss_first - c_1.loss_first) <= 1e-5 * c_1.loss_first and c_0.loss_last < c_0.loss_first
    assert np.abs(q_0 - q_1).max() <= 2e-3 * np.abs(q_1 - c0).max() + 1e-7
