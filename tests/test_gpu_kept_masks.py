"""The relu' masks and Fisher weights a keeping gradient pass of the fused 5-128-2 policy kernel leaves for the
Fisher-vector passes of the same call (k_policy_bf16, mask_plane.hpp).

(a) Fixed masks.  B = 33 samples (3 lanes x 11 steps): one full tile and a tail of one sample.  The policy's hidden biases
    are +-10 and its W1 is small (0.01 N(0, 1) against observations N(0, 1): |W1 x| stays below 0.3), so relu' of a unit is
    its bias's sign whatever the observation — a mask bit that lands in another unit's or another sample's place changes
    the product by a whole unit's term.  Signs from a seeded random bit per unit, all units on, all units off.
    rl_policy_fvp against the f64 oracle product by the comparison and the bars tests/test_gpu_tile_walk.py applies to its
    `fvp` pass (Checker.vector: no farther from f64 than max(4 x the f32-sample oracle's distance, 1e-6) of the largest
    entry).

(b) Nothing stale.  The kept planes are valid for one C-ABI call.  Every comparison is bitwise, against a fresh engine
    that does only the last operation on the same parameters and planes, at B = 33 and B = 517 (47 lanes x 11 steps: the
    uneven 5 : 3 dealing plus a tail):
      rl_policy_fvp, new parameters through rl_params_set, rl_policy_fvp;
      two trajectories with different observations and one policy, products on A, B, A;
      rl_policy_gradient (a gradient pass that does not keep), then rl_trpo_update;
      rl_trpo_update, a PPO update, rl_trpo_update;
      rl_trpo_update, a new rollout into the same trajectory, rl_trpo_update.
"""
import collections

import numpy as np
import pytest

import oracle as O
import test_gpu_tile_walk as TW

pytestmark = pytest.mark.gpu

ra = pytest.importorskip("relearn_amd")

H = 128
PS = O.MlpShape(5, H, 2)
B1 = slice(5 * H, 6 * H)
SHAPES = {"B33": (3, 11), "B517": (47, 11)}
Case = collections.namedtuple("Case", "name passes")


def biased_policy(engine, signs):
    """W1 = 0.01 N(0, 1), b1 = +-10 by `signs` [H] (True: the unit is on for every sample)"""
    pol = ra.Mlp(engine, 5, H, 2)
    pol.init(2)
    p = pol.get_params()
    p[:5 * H] = (0.01 * np.random.default_rng(11).standard_normal(5 * H)).astype(np.float32)
    p[B1] = np.where(signs, 10.0, -10.0).astype(np.float32)
    pol.set_params(p)
    return pol


@pytest.mark.parametrize("pattern", ["random", "all-on", "all-off"])
def test_fixed_masks_against_f64(engine, pattern):
    n, T = SHAPES["B33"]
    signs = {"random": np.random.default_rng(5).integers(0, 2, size=H).astype(bool),
             "all-on": np.ones(H, dtype=bool), "all-off": np.zeros(H, dtype=bool)}[pattern]
    pol = biased_policy(engine, signs)
    traj = ra.Trajectory(engine, n, T, 5)
    case = Case("fixed-masks-" + pattern, ("fvp",))
    try:
        with TW.Profiled(engine, case):
            h = TW.history(n, T)
            x, a, adv, rtg = TW.flat(h)
            pp = pol.get_params()
            assert np.abs(x @ pp[:5 * H].reshape(H, 5).T).max() < 0.3  # the bias decides every relu'
            TW.write(traj, h)
            v = TW.tangent()
            got = ra.policy_fvp(pol, traj, v, 0.0)
            h64, _ = O.grad_f64_mt("fvp", PS, pp, x, v=v)
            h32, _ = O.grad_f64_mt("fvp", PS, pp, x, v=v, f32_samples=True)
            TW.Checker(case.name, samples=n * T).vector("fisher-vector", got, h64, h32)
            # the rows of the units that are off are exactly zero (W1, b1 and both W2 rows): their masked sums are empty
            off = ~signs
            rows = np.concatenate([np.repeat(off, 5), off, off, off, [False, False]])
            assert not got[rows].any(), np.abs(got[rows]).max()
    finally:
        traj.close()
        pol.close()


# ---------------------------------------------------------------- nothing stale
def fresh(n, T, params, planes, op):
    """op(policy, trajectory) on a new engine that has seen nothing else"""
    eng = ra.Engine(0)
    eng.set_kernel_variant(0)
    pol = ra.Mlp(eng, 5, H, 2)
    pol.init(2)
    pol.set_params(params)
    traj = ra.Trajectory(eng, n, T, 5)
    write_planes(traj, planes)
    try:
        return op(pol, traj)
    finally:
        traj.close()
        pol.close()
        eng.close()


def write_planes(traj, planes):
    traj.write(ra.TRAJ_OBS, planes["obs"])
    traj.write(ra.TRAJ_ACTION, planes["action"])
    traj.write(ra.TRAJ_ADVANTAGES, planes["adv"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def trpo(pol, traj):
    """the parameters a TRPO update leaves, and its statistics"""
    st = ra.trpo_update(pol, traj)
    return pol.get_params(), st.as_dict()


def assert_same_update(got, want, what):
    assert same_bits(got[0], want[0]), what + ": parameters differ from a fresh engine's"
    assert got[1] == want[1] or all(same_bits(np.float64(got[1][k]), np.float64(want[1][k])) for k in want[1]), \
        (what, got[1], want[1])
    assert want[1]["cg_iterations"] > 0, want[1]


@pytest.fixture
def setup(engine, request):
    n, T = SHAPES[request.param]
    engine.set_kernel_variant(0)
    pol = ra.Mlp(engine, 5, H, 2)
    pol.init(2)
    traj = ra.Trajectory(engine, n, T, 5)
    planes = TW.history(n, T, seed=3)
    write_planes(traj, planes)
    yield n, T, pol, traj, planes
    traj.close()
    pol.close()


both_shapes = pytest.mark.parametrize("setup", list(SHAPES), indirect=True)


@both_shapes
def test_product_after_new_parameters(engine, setup):
    n, T, pol, traj, planes = setup
    v = TW.tangent()
    first = ra.policy_fvp(pol, traj, v, 0.0)
    p2 = (pol.get_params() + np.float32(0.05) * np.random.default_rng(1).standard_normal(pol.P).astype(np.float32))
    p2[B1] = -p2[B1] + np.float32(0.1)  # (moves many units across their relu edge)
    pol.set_params(p2.astype(np.float32))
    got = ra.policy_fvp(pol, traj, v, 0.0)
    want = fresh(n, T, p2.astype(np.float32), planes, lambda p, t: ra.policy_fvp(p, t, v, 0.0))
    assert same_bits(got, want) and not same_bits(got, first)


@both_shapes
def test_products_on_two_trajectories(engine, setup):
    n, T, pol, traj_a, planes_a = setup
    planes_b = TW.history(n, T, seed=4)
    traj_b = ra.Trajectory(engine, n, T, 5)
    try:
        write_planes(traj_b, planes_b)
        v = TW.tangent()
        pp = pol.get_params()
        a1 = ra.policy_fvp(pol, traj_a, v, 0.0)
        b1 = ra.policy_fvp(pol, traj_b, v, 0.0)
        a2 = ra.policy_fvp(pol, traj_a, v, 0.0)
        want_a = fresh(n, T, pp, planes_a, lambda p, t: ra.policy_fvp(p, t, v, 0.0))
        want_b = fresh(n, T, pp, planes_b, lambda p, t: ra.policy_fvp(p, t, v, 0.0))
        assert same_bits(a1, want_a) and same_bits(a2, want_a) and same_bits(b1, want_b)
        assert not same_bits(want_a, want_b)
    finally:
        traj_b.close()


@both_shapes
def test_update_after_a_gradient_that_does_not_keep(engine, setup):
    n, T, pol, traj, planes = setup
    pp = pol.get_params()
    ra.policy_gradient(pol, traj)
    got = trpo(pol, traj)
    assert_same_update(got, fresh(n, T, pp, planes, trpo), "gradient, update")


@both_shapes
def test_update_ppo_update(engine, setup):
    n, T, pol, traj, planes = setup
    trpo(pol, traj)
    step = ra.ppo_config_default()
    step.opt_steps_per_update = 2
    opt = ra.Optimizer(pol, ra.optimizer_config_default(ra.OPTIMIZER_ADAM))
    try:
        ra.ppo_update(pol, opt, traj, step)
    finally:
        opt.close()
    before = pol.get_params()
    got = trpo(pol, traj)
    assert_same_update(got, fresh(n, T, before, planes, trpo), "update, ppo, update")


@both_shapes
def test_update_rollout_update(engine, setup):
    n, T, pol, traj, planes = setup
    trpo(pol, traj)
    env = ra.CartPoleEnv(engine, n, max_steps=9, seed_env=5, seed_actor=6)
    cri = ra.Mlp(engine, 5, H, 1)
    cri.init(3)
    try:
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.95)
        rolled = dict(obs=traj.read(ra.TRAJ_OBS), action=traj.read(ra.TRAJ_ACTION), adv=traj.read(ra.TRAJ_ADVANTAGES))
        assert not same_bits(rolled["obs"], planes["obs"])
        before = pol.get_params()
        got = trpo(pol, traj)
        assert_same_update(got, fresh(n, T, before, rolled, trpo), "update, rollout, update")
    finally:
        cri.close()
        env.close()
