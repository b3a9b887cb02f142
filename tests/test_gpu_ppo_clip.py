"""The clipped PPO gradient at ratios off 1, on every policy path, against the f64 reference of tests/ppo_clip_cases.py.

Under plain SGD at rate lr from p0, rl_ppo_update with one step gives p1 and, from p0 again with a fresh optimiser, with
two steps gives p2.  Both steps of the second run share log pi_0 of p0, so g_dev = (p1 - p2) / lr in f64 is the clipped
gradient AT p1 — where the first step, a large one, has moved the ratios both ways for both signs of the drawn advantages,
and where the mask, the side it clips and the min matter (at the first step every ratio is exactly 1).  The readback costs
element j at most 2^-24 (|p2_j| + lr |g_j|) / lr — the rounding of lr g_j and of p2_j — and exactly that is added to the
bar.  The reference is evaluated at the device's own p1.

The bar, relative to max |g|, is the one the same path's existing test applies to rl_policy_gradient:
  "single"     1e-6 + 2 e32 (tests/narrow_cases.py grad_check; e32 the f32 oracle's own distance from f64 on the row's data)
  "general"    2e-5 of max |g| + 1e-9 (tests/test_gpu_general_mlp.py)
  "multi"      close(): 2e-5 of max |g| + 1e-9 (tests/test_gpu_multi_action.py)
  "recurrent"  5e-6 (GRAD_RTOL of tests/test_gpu_gru.py, test_gpu_stacked.py and test_gpu_chain_linear.py)
and every parameter block is held to 50 times it relative to the block's own maximum."""
import numpy as np
import pytest

import ppo_clip_cases as pc
import relearn_amd as ra

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
BLOCK_FACTOR = 50.0
_runs = {}


def build_module(engine, row):
    if row.kind == "mlp":
        D, hidden, A, act = row.spec
        return ra.Mlp(engine, D, hidden, A, act)
    if row.kind == "rnn":
        cell, D, H, NL, H2, A = row.spec
        return (ra.GruMlp if cell == "gru" else ra.LstmMlp)(engine, D, A, H, H2, num_layers=NL)
    cell, D, H, NL, A = row.spec
    return (ra.GruLinear if cell == "gru" else ra.LstmLinear)(engine, D, A, H, num_layers=NL)


def sgd_steps(pol, traj, p0, lr, steps, clip):
    """`steps` PPO steps under plain SGD (no momentum, no weight decay) from p0 with a fresh optimiser"""
    cfg = ra.optimizer_config_default(ra.OPTIMIZER_SGD)
    assert (cfg.momentum, cfg.weight_decay, cfg.dampening, cfg.nesterov) == (0.0, 0.0, 0.0, 0)
    cfg.learning_rate = lr
    step = ra.ppo_config_default()
    step.opt_steps_per_update, step.clip_distance = steps, clip
    pol.set_params(p0)
    opt = ra.Optimizer(pol, cfg)
    try:
        _, losses = ra.ppo_update(pol, opt, traj, step, want_losses=True)
        return pol.get_params(), losses.astype(np.float64)
    finally:
        opt.close()


def device_runs(engine, case):
    """every device run of a case, once: one and two steps at each clip distance, and rl_policy_gradient at p0"""
    if case in _runs:
        return _runs[case]
    name, variant = case
    row = pc.BY_NAME[name]
    h = pc.history(name)
    p0 = pc.initial_params(name)
    engine.set_kernel_variant(variant)
    try:
        pol = build_module(engine, row)
        assert pol.P == len(p0)
        traj = ra.Trajectory(engine, row.n, row.T, pc.in_dim_of(row))
        traj.write_all(h)
        traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
        r = dict(row=row, p0=p0)
        pol.set_params(p0)
        r["g0"] = ra.policy_gradient(pol, traj)[0]
        r["again"] = sgd_steps(pol, traj, p0, row.lr, 1, 0.2)[0]
        for clip in pc.CLIPS:
            r[clip] = dict(p1=sgd_steps(pol, traj, p0, row.lr, 1, clip)[0])
            r[clip]["p2"], r[clip]["losses"] = sgd_steps(pol, traj, p0, row.lr, 2, clip)
        traj.close()
        pol.close()
    finally:
        engine.set_kernel_variant(0)
    _runs[case] = r
    return r


def bar_of(row, p1):
    """(relative bar, absolute floor)"""
    if row.bar == "single":
        return 1e-6 + 2.0 * pc.f32_oracle_distance(row, p1), 0.0
    return {"general": (2e-5, 1e-9), "multi": (2e-5, 1e-9), "recurrent": (5e-6, 0.0)}[row.bar]


def check_gradient(case, what, row, p_before, p_after, ref_grad, rel, floor):
    """(p_before - p_after) / lr against ref_grad: whole vector and per block; prints the measured error beside its bar"""
    g_dev = (p_before.astype(np.float64) - p_after.astype(np.float64)) / row.lr
    readback = ULP * (np.abs(p_after.astype(np.float64)) + row.lr * np.abs(ref_grad)) / row.lr
    diff = np.abs(g_dev - ref_grad)
    gmax = np.abs(ref_grad).max()
    beyond = np.maximum(diff - readback, 0.0).max() / gmax
    print("%s %s: device error %.3g of max|g|, %.3g beyond the readback term (bar %.3g); readback term at most %.3g" % (
        pc.case_id(case), what, diff.max() / gmax, beyond, rel + floor / gmax, readback.max() / gmax))
    failures = []
    if not np.all(diff <= rel * gmax + floor + readback):
        failures.append(("whole", beyond, rel))
    for blk, s in pc.blocks(row):
        bmax = np.abs(ref_grad[s]).max()
        assert bmax > 0.0, (blk, "the reference gradient of this block is zero")
        if not np.all(diff[s] <= BLOCK_FACTOR * (rel * bmax + floor) + readback[s]):
            failures.append((blk, np.maximum(diff[s] - readback[s], 0.0).max() / bmax, BLOCK_FACTOR * rel))
    assert not failures, failures


def check_second_step(case, clip, r):
    """the gradient and the loss of the second step at clip distance `clip` against the reference at the device's p1"""
    row, p1, p2 = r["row"], r[clip]["p1"], r[clip]["p2"]
    B = row.n * row.T
    ref = pc.reference(row, r["p0"], p1, clip)
    c = ref["census"]
    print("%s clip %.1f: census %s, nearest ratio to a bound %.3g" % (pc.case_id(case), clip, c, ref["margin"]))
    # the conditions of tests/test_ppo_clip_cases_cpu.py, at the device's p1
    assert ref["margin"] > pc.MARGIN, ref["margin"]
    if clip == 0.2:
        assert min(c[1:]) >= 0.05 * B and c[0] >= 0.15 * B, c
    elif clip == 0.0:
        assert c[0] == 0 and min(c[1:]) >= 0.05 * B, c
    else:
        assert c == (B, 0, 0, 0, 0), c  # the unclipped surrogate
    rel, floor = bar_of(row, p1)
    check_gradient(case, "clip %.1f" % clip, row, p1, p2, ref["grad"], rel, floor)
    loss = r[clip]["losses"][1]
    print("%s clip %.1f: loss %.8g, reference %.8g" % (pc.case_id(case), clip, loss, ref["loss"]))
    assert abs(loss - ref["loss"]) <= 2e-5 * max(1.0, abs(ref["loss"]))  # tests/test_gpu_ppo.py's bar for a step's loss


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_clipped_gradient_against_f64(engine, case):
    r = device_runs(engine, case)
    # precondition of the method: two one-step runs from p0 return the same bits
    assert np.array_equal(r["again"], r[0.2]["p1"])
    assert not np.array_equal(r[0.2]["p1"], r["p0"]) and np.all(np.isfinite(r[0.2]["p2"]))
    check_second_step(case, 0.2, r)


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_clip_zero_and_clip_wide(engine, case):
    """clip 0.0: lo = hi = 1, and step one is a tie inside the bounds — the bits of the 0.2 run's p1; its second step clips
    every sample of two regions.  clip 4.0: a negative lower bound, nothing clipped — the unclipped surrogate's gradient."""
    r = device_runs(engine, case)
    assert np.array_equal(r[0.0]["p1"], r[0.2]["p1"])
    assert np.array_equal(r[4.0]["p1"], r[0.2]["p1"])
    check_second_step(case, 0.0, r)
    check_second_step(case, 4.0, r)


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_first_step_is_the_unclipped_gradient(engine, case):
    """(p0 - p1) / lr is rl_policy_gradient's vector within the readback term alone: a failure of step two (above) can be
    told from a failure of step one"""
    r = device_runs(engine, case)
    row, p0, p1 = r["row"], r["p0"].astype(np.float64), r[0.2]["p1"].astype(np.float64)
    g0 = r["g0"].astype(np.float64)
    assert np.abs(g0).max() > 0.0
    readback = ULP * (np.abs(p1) + row.lr * np.abs(g0)) / row.lr
    diff = np.abs((p0 - p1) / row.lr - g0)
    print("%s: first step, worst excess over the readback term %.3g of max|g|" % (
        pc.case_id(case), np.maximum(diff - readback, 0.0).max() / np.abs(g0).max()))
    assert np.all(diff <= readback)
    # and that vector is the reference's gradient at ratio 1 (the existing check of rl_policy_gradient, at this row's bar)
    rel, floor = bar_of(row, r["p0"])
    ref = pc.unclipped_gradient(row, r["p0"])
    assert np.abs(g0 - ref).max() <= rel * np.abs(ref).max() + floor
