"""Narrow and 4-input single-hidden-layer modules on every device path, against the oracle.

rl_mlp_create takes hidden 1..128 and in_dim 4 or 5, and every shape but 5-128 runs the hand-written f32 kernels at both
kernel variants: the persistent rollouts through the packed LDS records (mlp_pack_lds / mlp_forward_group_lds, with G
threads per lane), mlp_forward_lane inside the row forward, the advantage scan and the TD targets, k_policy_pass,
k_critic_fwd and k_mlp_backward, and the reduction, CG, line-search and optimiser kernels at P between 7 and 1026.  The
rest of the suite runs that family at H = 128, D = 5 almost everywhere; here it runs at the shapes of
tests/narrow_cases.py — tails of the 16-unit blocks dealt to G threads, the `j < H` mask and the H-dependent parameter
offsets of the backward pass, the empty fifth slot of a D = 4 record — and tests/test_narrow_cases_cpu.py shows on the
CPU that these comparisons fail when a tail unit is lost.

Bars.  Everything on the rollout and value paths is bit for bit (array_equal), as in tests/test_gpu_parity.py.  Losses,
KL, entropy, Adam parameters and PPO losses take tests/test_gpu_parity.py's, tests/test_gpu_ppo.py's and
tests/test_gpu_values_opt.py's bars unchanged.  A gradient or a Fisher-vector product takes narrow_cases.grad_check: no
farther from the f64 oracle than GRAD_RTOL + 2 e32, e32 being the f32 oracle's own distance from it (two correct f32
sums differ by more than GRAD_RTOL at these shapes: e32 reaches 7.4e-7 at 5-1), every parameter block within 50 times
that.  Each case prints e32 and the device's error.

Observed on an MI355X (256 CUs), relative to max |g|, over the 18 trajectories (the two kernel variants give the same
figures):
  check                   e32                 device vs f64       bar                 closest to its bar
  policy gradient         3.9e-8 .. 7.4e-7    3.8e-8 .. 7.4e-7    1.1e-6 .. 2.5e-6    5-1 ragged, 0.30 of it
  Fisher-vector product   1.6e-8 .. 2.5e-7    1.6e-8 .. 3.0e-7    1.0e-6 .. 1.5e-6    4-128 tiny, 0.21 of it
  critic gradient         1.5e-8 .. 9.3e-8    1.5e-8 .. 1.3e-7    1.0e-6 .. 1.2e-6    4-128 tiny, 0.12 of it
"""
import ctypes as C

import numpy as np
import pytest

import narrow_cases as nc
import oracle as O

pytestmark = pytest.mark.gpu

ra = pytest.importorskip("relearn_amd")

from test_gpu_dqn import check_store, make as make_dqn  # noqa: E402
from test_gpu_parity import GRAD_RTOL, PARAM_ATOL, _oracle_cfg  # noqa: E402

L = O.lib()
assert GRAD_RTOL == nc.GRAD_RTOL and (ra.LIMIT_NONE, ra.LIMIT_LATENT, ra.LIMIT_VISIBLE) == (
    O.LIMIT_NONE, O.LIMIT_LATENT, O.LIMIT_VISIBLE)

SHAPE_IDS = [nc.shape_id(s) for s in nc.SHAPES]
UPDATE_CASES = [(s, k) for s in nc.SHAPES for k in nc.UPDATE_KINDS]
UPDATE_IDS = ["%s-%s" % (nc.shape_id(s), k) for s, k in UPDATE_CASES]
on_update_cases = pytest.mark.parametrize("shape,kind", UPDATE_CASES, ids=UPDATE_IDS)


@pytest.fixture(params=[0, 1], ids=["kernels-best", "kernels-v1"])
def variant(engine, request):
    """both kernel variants: off the fused shape they take the same kernels (test_both_variants_take_the_same_kernels)"""
    engine.set_kernel_variant(request.param)
    yield request.param
    engine.set_kernel_variant(0)


def modules(engine, shape):
    D, H = shape
    pol, cri = ra.Mlp(engine, D, H, 2), ra.Mlp(engine, D, H, 1)
    pol.init(nc.MODULE_SEEDS[shape][0])
    cri.init(nc.MODULE_SEEDS[shape][1])
    return pol, cri


def assert_rollout_equal(got, want):
    for k in ("action", "flag", "reward", "obs"):
        assert np.array_equal(got[k], want[k]), k
    m = want["flag"] == O.INTERRUPT
    assert np.array_equal(got["term_obs"][:, m], want["term_obs"][:, m])


# ------------------------------------------------------------------------------------------- rollout, forward, values
ROLLOUTS = [(s, l, g) for s, l, gs in nc.ROLLOUT_CASES for g in gs]


@pytest.mark.parametrize("shape,limit,G", ROLLOUTS, ids=["%s-limit%d-G%d" % (nc.shape_id(s), l, g) for s, l, g in ROLLOUTS])
def test_rollout_bit_exact_in_every_group_class(engine, shape, limit, G):
    """k_rollout_cartpole<D, 64, G> with one lane count inside each class of launch_rollout's rule (narrow_cases.py cites
    it), none a multiple of 64: the last wave's `live` clamp.  Two periods of nine steps under a nine-step limit: every
    lane resets, the second period crosses the 16-word block of the actor stream and continues the lanes."""
    n = nc.rollout_lanes(engine.info()[2])[G]
    D, H = shape
    env = ra.CartPoleEnv(engine, n, max_steps=nc.ROLLOUT_MAX_STEPS, limit=limit, **nc.ROLLOUT_SEEDS)
    pol, _ = modules(engine, shape)
    traj = ra.Trajectory(engine, n, nc.ROLLOUT_T, D)
    for want, state in nc.oracle_rollout(shape, limit, n):
        ra.rollout(env, pol, traj)
        assert_rollout_equal(traj.read_all(), want)
        for a, b in zip(env.get_state(), state):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("shape", nc.SHAPES, ids=SHAPE_IDS)
def test_forward_rows_bit_exact(engine, shape):
    """rl_mlp_forward (k_mlp_forward_rows<D, A, false>, mlp_forward_lane's own tail) at one row, one short of a block of
    256 and one past it, both output widths"""
    D, H = shape
    rng = np.random.default_rng(H)
    for A, seed in ((2, 11), (1, 12)):
        m = ra.Mlp(engine, D, H, A)
        m.init(seed)
        p = m.get_params()
        assert np.array_equal(p, O.mlp_init(O.MlpShape(D, H, A), seed))
        for rows in (1, 255, 257):
            x = (2.0 * rng.standard_normal((rows, D))).astype(np.float32)
            want = O.mlp_forward_batch(O.MlpShape(D, H, A), p, x)
            assert np.array_equal(m.forward(x), want), (A, rows)
            assert np.abs(want).max() > 0


def device_case(engine, shape, kind):
    """the device side of narrow_cases.oracle_update_case: the lanes after the warm-up periods, one more rollout, the
    advantage pass — and the premise of every comparison below, that its trajectory and advantages are the oracle's"""
    r = nc.oracle_update_case(shape, kind)
    c = r["case"]
    env = ra.CartPoleEnv(engine, c["n"], max_steps=c["max_steps"], limit=c["limit"], seed_env=c["seed_env"],
                         seed_actor=c["seed_actor"])
    pol, cri = modules(engine, shape)
    traj = ra.Trajectory(engine, c["n"], c["T"], shape[0])
    for _ in range(c["warmup"] + 1):
        ra.rollout(env, pol, traj)
    assert_rollout_equal(traj.read_all(), r["want"])
    ra.gae(traj, cri, nc.GAMMA, nc.LAMBDA)
    assert np.array_equal(traj.read(ra.TRAJ_ADVANTAGES), r["adv2d"])
    assert np.array_equal(pol.get_params(), r["pp"]) and np.array_equal(cri.get_params(), r["cp"])
    return r, env, pol, cri, traj


@on_update_cases
def test_values_advantages_returns_and_td_targets_bit_exact(engine, shape, kind):
    """k_mlp_forward_rows<D, 1>, k_gae_scan<D> and k_value_targets_td<D> (mlp_forward_lane on the Interrupt successors)"""
    r, env, pol, cri, traj = device_case(engine, shape, kind)
    assert np.array_equal(traj.read(ra.TRAJ_VALUES), r["values"])
    assert np.array_equal(traj.read(ra.TRAJ_RETURNS), r["rtg2d"])
    ra.reward_to_go(traj, nc.GAMMA)
    assert np.array_equal(traj.read(ra.TRAJ_RETURNS), r["rtg2d"])
    assert np.array_equal(traj.read(ra.TRAJ_ADVANTAGES), r["rtg2d"])
    cfg = ra.values_opt_config_default()
    cfg.opt_steps_per_update, cfg.target, cfg.discount_factor = 1, ra.VALUE_TARGET_ONE_STEP_TD, nc.GAMMA
    ra.values_opt_update(cri, ra.Adam(cri), traj, cfg)
    assert np.array_equal(traj.read(ra.TRAJ_TARGETS), r["td2d"])


@pytest.mark.parametrize("hidden", [37, 100])
def test_chain_lanes_bit_exact(engine, hidden):
    """k_rollout_chain_mlp<5, 64>: one thread per lane through the LDS records, over two trajectories"""
    n, T = 70, 20
    env = ra.ChainEnv(engine, n, max_steps=9, seed_env=3, seed_actor=4)
    sim = O.ChainLaneSim(n, max_steps=9, seed_env=3, seed_actor=4)
    pol = ra.Mlp(engine, 5, hidden, 2)
    pol.init(41)
    traj = ra.Trajectory(engine, n, T, 5)
    for period in range(2):
        ra.rollout(env, pol, traj)
        want = sim.rollout_mlp(O.MlpShape(5, hidden, 2), pol.get_params(), T)
        got = traj.read_all()
        for k in ("obs", "action", "reward", "flag"):
            assert np.array_equal(got[k], want[k]), (period, k)
        m = want["flag"] == O.INTERRUPT
        assert m.any() and np.array_equal(got["term_obs"][:, m], want["term_obs"][:, m])
        for a, b in zip(env.get_state(), sim.get_state()):
            assert np.array_equal(a, b)
    assert set(np.unique(want["action"])) == {0, 1}


@pytest.mark.parametrize("lanes", ["200", "G8"])
@pytest.mark.parametrize("hidden,limit,seed", nc.DQN_CASES)
def test_dqn_collection_bit_exact(engine, hidden, limit, seed, lanes):
    """k_rollout_cartpole_dqn<D, 64, G> at G = 16 (200 lanes) and with a lane count of launch_rollout_dqn's G = 8 class
    (narrow_cases.py cites that rule), against the oracle's per-lane ReplayBuffers; the second collection evicts"""
    n = 200 if lanes == "200" else nc.dqn_lanes_g8(engine.info()[2])
    k = nc.DQN_COLLECT
    dqn, osim = make_dqn(engine, n=n, hidden=hidden, capacity=k["capacity"], limit=limit, max_steps=k["max_steps"],
                         eps=("const", k["eps"]))
    q = O.mlp_init(osim.qshape, seed)
    dqn.qnet.set_params(q)
    osim.qparams[:] = q
    for rep in range(k["reps"]):
        st = dqn.collect(k["T"])
        flags_o, full = osim.collect(k["T"], k["eps"])
        assert not full
        assert np.array_equal(dqn.replay_read(ra.REPLAY_LAST_FLAGS), flags_o)
        assert st.steps == k["T"] * n and st.episodes_ended == int((flags_o != 0).sum())
        check_store(dqn, osim)
    for a, b in zip(dqn.env.get_state(), osim.sim.get_state()):
        assert np.array_equal(a, b)
    dqn.close()


# ------------------------------------------------------------------------------------------- the update passes
def assert_grad(name, shape, A, got, f32, f64):
    err, e32, bar, failures = nc.grad_check(name, shape, A, got, f32, f64)
    assert not failures, failures


@on_update_cases
def test_policy_passes_match_the_oracles(engine, variant, shape, kind):
    """k_policy_pass<D, MODE> and k_mlp_backward<D, 2>: gradient, loss and entropy; Fisher-vector product, its symmetry
    and positivity; loss and KL at moved parameters, and KL == 0 at the parameters themselves"""
    r, env, pol, cri, traj = device_case(engine, shape, kind)
    ps, x, a, adv, p0 = r["ps"], r["x"], r["a"], r["adv"], r["pp"]
    g_d, loss_d, ent_d = ra.policy_gradient(pol, traj)
    assert_grad("policy gradient %s v%d" % (kind, variant), shape, 2, g_d, r["g32"], r["g64"])
    assert abs(loss_d - r["loss32"]) <= 1e-5 * max(1.0, abs(r["loss32"]))
    assert 0.0 < ent_d <= np.log(2.0) + 1e-6
    hv_d = ra.policy_fvp(pol, traj, r["v"], nc.FVP_REG)
    assert_grad("fisher-vector product %s v%d" % (kind, variant), shape, 2, hv_d, r["hv32"], r["hv64"])
    hu_d = ra.policy_fvp(pol, traj, r["u"], nc.FVP_REG)
    lhs = float(np.dot(r["u"].astype(np.float64), hv_d))
    rhs = float(np.dot(r["v"].astype(np.float64), hu_d))
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs), 1e-6)
    assert float(np.dot(r["v"].astype(np.float64), hv_d)) > 0.0
    p1 = (p0 + 0.01 * np.random.default_rng(2).standard_normal(len(p0))).astype(np.float32)
    pol.set_params(p1)
    loss_d, kl_d = ra.policy_loss_kl(pol, traj, p0)
    lo, ko = C.c_float(), C.c_float()
    L.oracle_policy_loss_kl_f32(ps, O.f32p(p1), O.f32p(p0), O.f32p(x), O.i64p(a), O.f32p(adv), len(a), C.byref(lo),
                                C.byref(ko))
    assert abs(loss_d - lo.value) <= 1e-5 * max(1.0, abs(lo.value))
    assert abs(kl_d - ko.value) <= 1e-5 * max(1e-3, abs(ko.value))
    pol.set_params(p0)
    loss0, kl0 = ra.policy_loss_kl(pol, traj, p0)
    assert kl0 == 0.0
    assert abs(loss0 + adv.astype(np.float64).mean()) < 1e-5 * max(1.0, abs(adv.mean()))


@on_update_cases
def test_critic_gradient_and_adam_steps_match_the_oracle(engine, variant, shape, kind):
    """k_critic_fwd<D> and k_mlp_backward<D, 1>, then 20 Adam steps (tests/test_gpu_parity.py's bars)"""
    r, env, pol, cri, traj = device_case(engine, shape, kind)
    g_d, loss_d = ra.critic_gradient(cri, traj)
    assert_grad("critic gradient %s v%d" % (kind, variant), shape, 1, g_d, r["c32"], r["c64"])
    assert abs(loss_d - r["closs32"]) <= 1e-5 * r["closs32"]
    steps = 20
    st, losses_d = ra.critic_update(cri, ra.Adam(cri), traj, steps, want_losses=True)
    c_o, losses_o = nc.oracle_critic_steps(shape, kind, "rtg", steps)
    assert np.allclose(losses_d, losses_o, rtol=1e-4)
    assert np.abs(cri.get_params() - c_o).max() < PARAM_ATOL + 1e-3 * steps * 1e-3
    assert losses_d[-1] < losses_d[0] and st.steps == steps


@on_update_cases
def test_values_opt_update_with_td_targets(engine, variant, shape, kind):
    """tests/test_gpu_values_opt.py's check: the targets of the critic as it stood before the first step, then 12 steps"""
    r, env, pol, cri, traj = device_case(engine, shape, kind)
    steps = 12
    cfg = ra.values_opt_config_default()
    cfg.opt_steps_per_update, cfg.target, cfg.discount_factor = steps, ra.VALUE_TARGET_ONE_STEP_TD, nc.GAMMA
    st, losses_d = ra.values_opt_update(cri, ra.Adam(cri), traj, cfg, want_losses=True)
    assert np.array_equal(traj.read(ra.TRAJ_TARGETS), r["td2d"])
    c_o, losses_o = nc.oracle_critic_steps(shape, kind, "td", steps)
    assert np.allclose(losses_d, losses_o, rtol=1e-4)
    assert np.abs(cri.get_params() - c_o).max() < 2e-5 + 1e-3 * steps * 1e-3
    assert st.steps == steps and losses_d[-1] < losses_d[0]


@pytest.mark.parametrize("run", list(nc.PPO_RUNS))
@on_update_cases
def test_ppo_update(engine, variant, shape, kind, run):
    """tests/test_gpu_ppo.py's check at its two learning rates.  Whether the larger rate clips, and whether eight steps
    at it lower the loss, depends on the trajectory (tests/test_narrow_cases_cpu.py: it clips on at least one of every
    shape's two): the device's answer to both is the oracle's."""
    r, env, pol, cri, traj = device_case(engine, shape, kind)
    lr, steps = nc.PPO_RUNS[run]
    acfg = ra.adam_config_default()
    acfg.learning_rate = lr
    cfg = ra.ppo_config_default()
    assert (cfg.opt_steps_per_update, cfg.clip_distance) == (10, 0.2)
    cfg.opt_steps_per_update = steps
    st, losses_d = ra.ppo_update(pol, ra.Adam(pol, acfg), traj, cfg, want_losses=True)
    p_o, losses_o, ent_o, clipped_o = nc.oracle_ppo(shape, kind, run)
    p_d = pol.get_params()
    assert abs(st.entropy - ent_o) < 1e-5
    assert st.steps == steps and st.loss_first == losses_d[0] and st.loss_last == losses_d[-1]
    scale = max(1.0, np.abs(losses_o).max())
    assert np.max(np.abs(losses_d - losses_o)) < 2e-5 * scale, (losses_d, losses_o)
    # Adam normalises by sqrt(v): where |g| is at rounding level a parameter can move by lr either way
    assert np.abs(p_d - p_o).max() < (2e-5 if lr < 1e-2 else 5e-3)
    assert np.mean(np.abs(p_d - p_o) < 2e-5) > 0.97
    ratio = np.exp(nc.policy_logp32(r["ps"], p_d, r["x"], r["a"]) - nc.policy_logp32(r["ps"], r["pp"], r["x"], r["a"]))
    clipped_d = float(((ratio < 0.8) | (ratio > 1.2)).mean())
    print("%s %s %s: share of ratios outside [0.8, 1.2] device %.3f oracle %.3f" % (nc.shape_id(shape), kind, run,
                                                                                     clipped_d, clipped_o))
    assert (clipped_d > 0.02) == (clipped_o > 0.02)
    assert (losses_d[-1] < losses_d[0]) == (losses_o[-1] < losses_o[0])


@on_update_cases
def test_reinforce_update(engine, variant, shape, kind):
    r, env, pol, cri, traj = device_case(engine, shape, kind)
    p = r["pp"].copy()
    st = ra.reinforce_update(pol, ra.Adam(pol), traj)
    ost, ocfg = L.oracle_adam_new(len(p)), nc.adam_cfg()
    loss, ent = C.c_float(), C.c_float()
    L.oracle_reinforce_update_f32(r["ps"], O.f32p(p), ost, C.byref(ocfg), O.f32p(r["x"]), O.i64p(r["a"]),
                                  O.f32p(r["adv"]), len(r["a"]), C.byref(loss), C.byref(ent))
    L.oracle_adam_free(ost)
    assert abs(st.loss_first - loss.value) <= 1e-5 * max(1.0, abs(loss.value))
    assert abs(st.entropy - ent.value) < 1e-5
    # first Adam step: every parameter moves by lr * sign(g) (up to eps): identical unless g is at rounding level
    assert np.mean(np.abs(pol.get_params() - p) < 1e-6) > 0.99


def test_both_variants_take_the_same_kernels(engine):
    """off the fused shape the kernel variant chooses nothing: the same launch classes, the same counts, the f32 family's
    forward and backward classes and no fused one"""
    r, env, pol, cri, traj = device_case(engine, (5, 100), "ragged")
    counts = {}
    engine.profile_enable(True)
    try:
        for variant in (0, 1):
            engine.set_kernel_variant(variant)
            engine.profile_read(reset=True)
            ra.policy_gradient(pol, traj)
            ra.policy_fvp(pol, traj, r["v"], nc.FVP_REG)
            ra.critic_gradient(cri, traj)
            counts[variant] = {k: int(c) for k, (_, c) in engine.profile_read(reset=True).items() if c}
    finally:
        engine.set_kernel_variant(0)
        engine.profile_enable(False)
    assert counts[0] == counts[1], counts
    assert set(counts[0]) == {"policy_pass", "backward", "critic_fwd", "reduce"}, counts


# ------------------------------------------------------------------------------------------- whole updates
def with_advantages(engine, shape, n, T, max_steps):
    D, H = shape
    limit = nc.update_case(shape, "ragged")["limit"]
    env = ra.CartPoleEnv(engine, n, max_steps=max_steps, limit=limit, **nc.ROLLOUT_SEEDS)
    pol, cri = modules(engine, shape)
    traj = ra.Trajectory(engine, n, T, D)
    ra.rollout(env, pol, traj)
    want = nc.oracle_rollout(shape, limit, n, T, max_steps, 1)[0][0]
    assert_rollout_equal(traj.read_all(), want)
    ra.gae(traj, cri, nc.GAMMA, nc.LAMBDA)
    x, a = O.flat_samples(want)
    return pol, traj, x, a, np.ascontiguousarray(traj.read(ra.TRAJ_ADVANTAGES).reshape(-1))


# (5, 1) stays: on these 512 x 16 steps the oracle's own f32 and f64 runs agree on status and backtrack count at one and
# at two CG iterations (status OK; 1 and 1 backtracks at 5-1, 0 or 1 at the other shapes), checked on the CPU
@pytest.mark.parametrize("shape", [(5, 17), (5, 100), (4, 37), (5, 1)], ids=nc.shape_id)
@pytest.mark.parametrize("iterations,tol", [(1, 3e-4), (2, 2e-3)])
def test_trpo_update_few_cg_iterations_tight(engine, variant, shape, iterations, tol):
    """tests/test_gpu_parity.py's test of the same name, its tolerances, on 512 lanes x 16 steps under a nine-step limit"""
    pol, traj, x, a, adv = with_advantages(engine, shape, 512, 16, 9)
    ps, p0 = nc.shapes_of(shape)[0], pol.get_params()
    dcfg = ra.trpo_config_default()
    dcfg.iterations = iterations
    st_d = ra.trpo_update(pol, traj, dcfg)
    p_d = pol.get_params()
    p_o, st_o, sd_o = O.trpo_update(ps, p0, x, a, adv, _oracle_cfg(dcfg))
    assert st_d.status == st_o.status == ra.OPT_OK
    assert st_d.num_backtracks == st_o.num_backtracks
    assert st_d.cg_iterations == st_o.cg_iterations == iterations
    assert abs(st_d.entropy - st_o.entropy) < 1e-5
    assert abs(st_d.loss_initial - st_o.loss_initial) <= 1e-5 * max(1.0, abs(st_o.loss_initial))
    assert abs(st_d.step_size - st_o.step_size) <= tol * st_o.step_size
    assert abs(st_d.loss_final - st_o.loss_final) <= 1e-5 * max(1.0, abs(st_o.loss_final))
    assert abs(st_d.constraint_val_final - st_o.constraint_val_final) <= 10 * tol * st_o.constraint_val_final + 1e-7
    assert np.abs(p_d - p_o).max() <= tol * np.abs(p_o - p0).max() + 1e-7


def test_trpo_rollback_on_failure(engine, variant):
    """tests/test_gpu_parity.py's test of the same name at 5-17 (256 lanes x 32 steps, 30-step limit: the oracle needs
    more than three backtracks there, in f32 and in f64)"""
    shape = (5, 17)
    pol, traj, x, a, adv = with_advantages(engine, shape, 256, 32, 30)
    ps, p0 = nc.shapes_of(shape)[0], pol.get_params()
    cfg = ra.trpo_config_default()
    cfg.max_backtracks = 3
    st = ra.trpo_update(pol, traj, cfg)
    p_o, st_o, _ = O.trpo_update(ps, p0, x, a, adv, _oracle_cfg(cfg))
    assert st.status == st_o.status
    assert st.status in (ra.OPT_CONSTRAINT_VIOLATED, ra.OPT_LOSS_NOT_IMPROVING)
    assert st.num_backtracks == -1 and st_o.num_backtracks == -1
    assert np.array_equal(pol.get_params(), p0) and np.array_equal(p_o, p0)
    cfg = ra.trpo_config_default()
    cfg.iterations = 0
    st = ra.trpo_update(pol, traj, cfg)
    assert st.status == ra.OPT_LOSS_NOT_IMPROVING and st.cg_iterations == 0
    assert np.array_equal(pol.get_params(), p0)
    traj.write(ra.TRAJ_ADVANTAGES, np.zeros((32, 256), np.float32))
    st = ra.trpo_update(pol, traj)
    p_o, st_o, _ = O.trpo_update(ps, p0, x, a, np.zeros_like(adv))
    assert st.status == st_o.status == ra.OPT_LOSS_NOT_IMPROVING
    assert np.array_equal(pol.get_params(), p0)


def test_actor_critic_update_equals_the_two_updates_in_turn(engine):
    """rl_actor_critic_update with a 5-100 policy and a 5-64 critic (the critic reads the trajectory's five features) is
    not on the two-stream pairing, which needs both modules on the fused 5-128 kernels: it runs rl_trpo_update, then
    rl_values_opt_update, and every number equals theirs bit for bit (tests/test_gpu_stacked.py's check of the other
    families)"""
    n, T = 64, 20
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = 5

    def run(joint):
        env = ra.CartPoleEnv(engine, n, max_steps=9, seed_env=5, seed_actor=6)
        pol, cri = ra.Mlp(engine, 5, 100, 2), ra.Mlp(engine, 5, 64, 1)
        pol.init(2)
        cri.init(3)
        opt = ra.Adam(cri)
        traj = ra.Trajectory(engine, n, T, 5)
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.95)
        if joint:
            pst, cst, losses = ra.actor_critic_update(pol, cri, opt, traj, None, ccfg, want_losses=True)
        else:
            pst = ra.trpo_update(pol, traj)
            cst, losses = ra.values_opt_update(cri, opt, traj, ccfg, want_losses=True)
        return pol.get_params(), cri.get_params(), pst.as_dict(), losses.copy()

    a, b = run(False), run(True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])
    assert a[2]["status"] == ra.OPT_OK and a[3][-1] < a[3][0]


@pytest.mark.parametrize("shape,other", [((5, 37), 36), ((4, 64), 63)], ids=["5-37", "4-64"])
def test_actor_document_round_trip(engine, shape, other):
    """actor_to_cbor / module_from_cbor: the parameters come back bit for bit; a module of another width refuses them"""
    D, H = shape
    env = ra.CartPoleEnv(engine, 64, max_steps=9, limit=ra.LIMIT_VISIBLE if D == 5 else ra.LIMIT_NONE)
    pol = ra.Mlp(engine, D, H, 2)
    pol.init(19)
    doc = ra.actor_to_cbor(env, pol)
    twin = ra.Mlp(engine, D, H, 2)
    twin.init(20)
    ra.module_from_cbor(twin, doc)
    assert np.array_equal(twin.get_params(), pol.get_params())
    narrower = ra.Mlp(engine, D, other, 2)
    narrower.init(21)
    before = narrower.get_params()
    with pytest.raises(ra.RelearnError):
        ra.module_from_cbor(narrower, doc)
    assert np.array_equal(narrower.get_params(), before)
