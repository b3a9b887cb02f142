"""relu' and the |pre| forward of the fused 5-128 kernels AT the edges the other tests stay away from (bt::mask_tile,
bt::range_guard, bt::masked_sum_tile, mask_plane.hpp; include/relearn_hip.h, "Numeric range of the fused kernels").

The designs are the table of tests/relu_edge_cases.py: pre-activations whose exact value — and so whose mask relu'(pre) =
[pre > 0], relu'(0) = 0 — is known from exact arithmetic, checked on the CPU by tests/test_relu_edge_cases_cpu.py.  Kernel
variant 0 under test_gpu_tile_walk.Profiled: the fused kernels ran, and no per-layer pass did.

(a) test_designed_sets.  One tile of 32 samples (n = 32, T = 1).  A set whose biases are all <= 0 runs as ONE live sample
    (the designed observation) on a tile of dead ones (observation 0, advantage 0, return = the critic's b2: pre = b1 <=
    0, no unit on, the output b2 exactly), the live sample at each of the 32 positions of the tile in turn — element 0 of
    every accumulator tile goes through v_med3 before the clamped conversion, and a mask bit that lands on another sample
    of the same unit moves the live sample's whole term.  A set with a bias > 0 in its design runs as 32 copies of the
    sample.  The sets `ordinary` and `margin` also run with two more tiles (n = 23, T = 3: B = 69), the live sample in
    the second tile and in the ragged third.  Every entry of the observation planes is a designed value or 0, row T
    included: the guard's range words see them all.
    Passes: rl_policy_gradient, rl_policy_fvp (reg 0, a tangent with equal b2 entries), rl_policy_loss_kl at parameters
    moved in W1 and W2, one rl_ppo_update under SGD at rate 1, rl_critic_gradient; at two positions rl_trpo_update
    against a fresh engine's result on the same planes, bit for bit (the kept mask planes at a per-sample pattern).
    Asserted: for a unit whose exact mask is 0, its W1 row, its b1 and its W2 column are EXACTLY 0.0 in the gradients,
    the PPO step and the Fisher-vector product — a fractional mask of any size fails that; everything else against
    O.grad_f64_mt over all 32 samples by TW.Checker.vector (no farther from f64 than max(4 x the f32-sample oracle's
    distance, 1e-6) of the largest entry) and TW's scalar bars (tests/test_gpu_parity.py's).  The `worst` design's units
    may come out 0 or 1 (their rows are all zero, or they meet the bar as rows of a unit that is on); the observed mask
    is printed and recorded in DESIGN 43.

(b) test_guard_boundary.  upper = 2^31 is refused by rl_critic_gradient, rl_policy_gradient and rl_policy_fvp with
    RL_ERR_UNSUPPORTED / "numeric range", 2^31 - 2^7 is accepted and correct; largest = 2^-46 is accepted (by a bias, and
    by max|w| min_nz|x|) and correct, the next f32 below is refused; every other unit is identically zero.

(c) test_forward_with_strongly_off_units.  b1 = -1000 on three quarters of the units, Glorot output weights (not on a
    grid): the two halves of relu(x) = (x + |x|) / 2 must cancel where plain f32 returns an exact 0.  One sample per call
    (B = 1), so that the critic's value y = dL/db2 / 2 + return and the policy's loss and KL are per-sample figures.

(d) test_convention_on_variant_1, test_convention_on_the_general_fused_kernels.  The order-free zeros and smallest
    values through kernel variant 1 at 5-128 and through the general fused kernels at [8, 8] (layer 1 designed, layer 2
    held off its edges by biases of +-1).

Measured distances, the observed mask of the worst case, the forward figures and wall times: DESIGN 43.
"""
import numpy as np
import pytest

import oracle as O
import relu_edge_cases as R
import test_gpu_gen_tile_walk as GW
import test_gpu_kept_masks as KM
import test_gpu_tile_walk as TW

pytestmark = pytest.mark.gpu

ra = pytest.importorskip("relearn_amd")

H = R.H
PS, CS = O.MlpShape(5, H, 2), O.MlpShape(5, H, 1)
W2P, W2C, B1 = TW.W2P, TW.W2C, TW.B1
POLICY_B2 = np.array([0.125, -0.25], dtype=np.float32)
CRITIC_B2 = TW.CRITIC_B2
ONE_TILE, THREE_TILES = (32, 1), (23, 3)
TRPO_AT = (0, 21)


def unit_rows(units, out_dim):
    """the entries of a flat 5-128-out_dim parameter vector that belong to hidden units `units` (boolean [H]): their W1
    rows, b1 and W2 columns"""
    units = np.asarray(units, dtype=bool)
    return np.concatenate([np.repeat(units, 5), units] + [units] * out_dim + [np.zeros(out_dim, dtype=bool)])


def modules_of(engine, s):
    pol, cri = ra.Mlp(engine, 5, H, 2), ra.Mlp(engine, 5, H, 1)
    pol.init(2)
    cri.init(3)
    pol.set_params(R.params(s, 2, 2, POLICY_B2))
    cri.set_params(R.params(s, 1, 3, [CRITIC_B2]))
    return pol, cri


def tangent_and_candidate(s, pp, masks):
    """a tangent of the parameters' own magnitudes with equal b2 entries (and nothing on the W1 rows and b1 of units
    whose mask is open: the tangent logits then do not depend on it), and candidate parameters moved in W1 and W2"""
    v0 = TW.tangent()
    v = v0.copy()
    v[:5 * H] *= np.float32(64.0) * s.w1_move
    v[W2P] *= R.p2(s.w2_log2)
    v[8 * H:] = 0.5
    open_units = masks < 0
    v[np.concatenate([np.repeat(open_units, 5), open_units, np.zeros(2 * H + 2, dtype=bool)])] = 0.0
    p_new = pp.copy()
    p_new[:5 * H] = np.float32(s.w1_keep) * pp[:5 * H] + s.w1_move * v0[:5 * H]
    p_new[W2P] = R.w2_grid(s, 2, 2, moved=True).reshape(-1)
    return v, p_new


def planes_with(s, n, T, live, rng):
    """(planes, flat samples) with the designed observation at the flat sample indices `live` (b = t n + lane) and dead
    samples elsewhere"""
    planes = TW.dead_batch(n, T)
    obs_flat = planes["obs"].reshape(5, (T + 1) * n)
    k = len(live)
    obs_flat[:, live] = np.asarray(s.x, dtype=np.float32)[:, None]
    # Copies of one observation have one policy output, so a sample's gradient term is (1[a = 0] - p0) A times a vector they
    # all share: with advantages of random sign the 32 terms cancel (measured on the f64 oracle for `lower-bias`: sum of
    # the terms' magnitudes 76 x the largest entry of their sum), the kernels add a tile's terms in f32 before the f64
    # level while the f32-sample oracle of the yardstick adds samples in f64, and the first run missed the bar at
    # 1.3e-6 against 1e-6 — a third of ONE f32 rounding of such a sum.  So the sign of the advantage goes with the action
    # (A > 0 for action 0, A < 0 for action 1): both actions, both signs, and every term on the same side.
    action = rng.integers(0, 2, size=k) if k == 1 else np.arange(k) % 2
    sign = rng.choice([-1.0, 1.0], size=k) if k == 1 else np.where(action == 0, 1.0, -1.0)
    planes["action"].reshape(-1)[live] = action.astype(np.uint8)
    planes["adv"].reshape(-1)[live] = (sign * (0.5 + rng.random(k))).astype(np.float32)
    planes["rtg"].reshape(-1)[live] = (-3.0 + rng.random(k)).astype(np.float32)
    assert not planes["obs"][:, T].any()
    return planes


class EdgeChecker(TW.Checker):
    """TW.Checker's comparisons with the unit rows of this file: exact zeros where the exact mask is 0, the open units
    (mask 0 or 1, never a fraction) apart"""

    def __init__(self, tag, masks, out_dim_of, samples):
        super().__init__(tag, samples=samples)
        self.masks, self.out_dim_of, self.observed = masks, out_dim_of, {}

    def unit_vector(self, name, got, want64, want32, extra_abs=0.0):
        out_dim = self.out_dim_of[name]
        got = np.asarray(got, dtype=np.float64)
        off = unit_rows(self.masks == 0, out_dim)
        assert not want64[off].any() and not want32[off].any(), (self.tag, name, "the oracle's own zeros")
        nz = np.flatnonzero(got[off])
        assert nz.size == 0, (self.tag, name, "non-zero entries of units whose exact mask is 0", nz[:8], got[off][nz[:8]])
        top = np.abs(want64).max()
        bar = max(4 * TW.rel_err(want32, want64), 1e-6) * top + extra_abs
        got, want64, want32 = got.copy(), want64.copy(), want32.copy()
        seen = []
        for j in np.flatnonzero(self.masks < 0):
            rows = unit_rows(np.arange(H) == j, out_dim)
            on = bool(got[rows].any())
            seen.append(int(on))
            if on:
                assert np.abs(got[rows] - want64[rows]).max() < bar, (self.tag, name, "a fractional mask on unit", j)
            got[rows] = want64[rows] = want32[rows] = 0.0
        if seen:
            assert len(set(seen)) == 1, (self.tag, name, "the open units differ among themselves", seen)
            self.observed[name] = seen[0]
        self.vector(name, got, want64, want32, extra_abs)


def run_edge_passes(chk, s, pol, cri, traj, planes, v, p_new, trpo=False):
    n, T = planes["action"].shape[1], planes["action"].shape[0]
    B = n * T
    x, a, adv, rtg = TW.flat(planes)
    pp, cp = pol.get_params(), cri.get_params()
    ent64, loss_new64, kl64 = TW.policy_scalars64(p_new, pp, x, a, adv)
    g_d, loss_d, ent_d = ra.policy_gradient(pol, traj)
    g64, l64 = O.grad_f64_mt("policy", PS, pp, x, a, adv)
    g32, _ = O.grad_f64_mt("policy", PS, pp, x, a, adv, f32_samples=True)
    chk.unit_vector("policy gradient", g_d, g64, g32)
    chk.scalar("policy loss", loss_d, l64, 1e-5 * max(1.0, abs(l64)))
    print("%s entropy          got %.9g  f64 %.9g" % (chk.tag, ent_d, ent64 / B))
    assert abs(ent_d - ent64 / B) < 1e-5
    h_d = ra.policy_fvp(pol, traj, v, 0.0)
    h64, _ = O.grad_f64_mt("fvp", PS, pp, x, v=v)
    h32, _ = O.grad_f64_mt("fvp", PS, pp, x, v=v, f32_samples=True)
    chk.unit_vector("fisher-vector", h_d, h64, h32)
    loss_m, kl_m = GW.moved_loss_kl(pol, traj, p_new)
    chk.scalar("moved loss", loss_m, loss_new64 / B, 1e-5 * max(1.0, abs(loss_new64 / B)))
    chk.scalar("moved kl", kl_m, kl64 / B, 1e-5 * max(1e-3, abs(kl64 / B)) + chk.floor)
    assert kl64 > 0.0, "the candidate parameters must move the policy"
    step = GW.sgd_ppo_step(pol, traj)
    p1_top = np.abs(pp.astype(np.float64) - step).max()
    chk.unit_vector("ppo step", step, g64, g32, extra_abs=2.0 ** -24 * max(np.abs(pp).max(), p1_top))
    gc_d, lc_d = ra.critic_gradient(cri, traj)
    gc64, lc64 = O.grad_f64_mt("critic", CS, cp, x, aux=rtg)
    gc32, _ = O.grad_f64_mt("critic", CS, cp, x, aux=rtg, f32_samples=True)
    chk.unit_vector("critic gradient", gc_d, gc64, gc32)
    chk.scalar("critic loss", lc_d, lc64, 1e-5 * lc64)
    if trpo:
        got = KM.trpo(pol, traj)
        pol.set_params(pp)
        KM.assert_same_update(got, KM.fresh(n, T, pp, planes, KM.trpo), chk.tag + " trpo")
    return chk.observed


OUT_DIMS = {"policy gradient": 2, "fisher-vector": 2, "ppo step": 2, "critic gradient": 1}


@pytest.mark.parametrize("name", list(R.SETS))
def test_designed_sets(engine, name):
    s = R.SETS[name]
    masks = R.expected_masks(s)
    pol, cri = modules_of(engine, s)
    v, p_new = tangent_and_candidate(s, pol.get_params(), masks)
    layouts = [(ONE_TILE, [b]) for b in range(32)] if not s.copies else [(ONE_TILE, list(range(32)))]
    if name in ("ordinary", "margin"):
        layouts += [(THREE_TILES, [32 + 17]), (THREE_TILES, [64 + 3])]
    case = KM.Case("relu-edges-" + name, ("policy", "eval", "fvp", "critic"))
    observed = []
    trajs = {shape: ra.Trajectory(engine, shape[0], shape[1], 5) for shape in (ONE_TILE, THREE_TILES)}
    try:
        with TW.Profiled(engine, case):
            for (n, T), live in layouts:
                rng = np.random.default_rng([len(observed), n])
                planes = planes_with(s, n, T, live, rng)
                traj = trajs[(n, T)]
                TW.write(traj, planes)
                tag = "%s B=%d live %s" % (name, n * T, live[0] if len(live) == 1 else "all")
                chk = EdgeChecker(tag, masks, OUT_DIMS, samples=n * T)
                trpo = s.copies or (n == 32 and live[0] in TRPO_AT) or n != 32
                observed.append(run_edge_passes(chk, s, pol, cri, traj, planes, v, p_new, trpo=trpo))
        if (masks < 0).any():
            print("%s: observed masks of the open units per layout: %s" % (name, observed))
            flat = {m for o in observed for m in o.values()}
            assert len(flat) == 1, ("the open units' mask depends on the sample's position or the pass", observed)
    finally:
        for t in trajs.values():
            t.close()
        pol.close()
        cri.close()


@pytest.mark.parametrize("name", list(R.GUARD_CASES))
def test_guard_boundary(engine, name):
    g = R.GUARD_CASES[name]
    s = R.guard_set(g)
    masks = R.expected_masks(s)
    pol, cri = modules_of(engine, s)
    v, p_new = tangent_and_candidate(s, pol.get_params(), masks)
    n, T = ONE_TILE
    traj = ra.Trajectory(engine, n, T, 5)
    case = KM.Case("guard-" + name, () if g.refused else ("policy", "fvp", "critic"))
    try:
        with TW.Profiled(engine, case):
            planes = planes_with(s, n, T, list(range(32)), np.random.default_rng(5))
            TW.write(traj, planes)
            x, a, adv, rtg = TW.flat(planes)
            pp, cp = pol.get_params(), cri.get_params()
            calls = {"critic gradient": lambda: ra.critic_gradient(cri, traj)[0],
                     "policy gradient": lambda: ra.policy_gradient(pol, traj)[0],
                     "fisher-vector": lambda: ra.policy_fvp(pol, traj, v, 0.0)}
            if g.refused:
                for what, call in calls.items():
                    with pytest.raises(ra.RelearnError) as err:
                        call()
                    assert err.value.code == ra.ERR_UNSUPPORTED and "numeric range" in str(err.value), (name, what)
            else:
                chk = EdgeChecker("guard " + name, masks, OUT_DIMS, samples=n * T)
                want = {"critic gradient": ("critic", CS, cp, dict(aux=rtg)),
                        "policy gradient": ("policy", PS, pp, dict(actions=a, aux=adv)),
                        "fisher-vector": ("fvp", PS, pp, dict(v=v))}
                for what, call in calls.items():
                    kind, shape, p, kw = want[what]
                    w64, _ = O.grad_f64_mt(kind, shape, p, x, **kw)
                    w32, _ = O.grad_f64_mt(kind, shape, p, x, f32_samples=True, **kw)
                    chk.unit_vector(what, call(), w64, w32)
    finally:
        traj.close()
        pol.close()
        cri.close()


# ---------------------------------------------------------------- (c) the forward with strongly-off units
FORWARD_SAMPLES = 24
# What the form costs.  Both halves of sum_j w2_j (pre_j + |pre_j|) / 2 are f32 sums of 128 terms of size |w2_j pre_j|,
# the units that are off included, so the result carries roundings of 2^-24 of S = sum_j |w2_j pre_j| where a plain f32
# forward (relu by comparison: exact zeros for the units that are off) carries them of the ACTIVE units' sum only.  The
# bar for a logit or a value is c 2^-24 S per sample.  c counts the roundings a correct f32 summation of such a sum makes
# and is not taken from the fused kernel: it is 4 x what kernel variant 1 (plain f32) measures on the same inputs in
# units of 2^-24 x ITS conditioning, the active units' sum_j |w2_j pre_j| + |b2| — measured per run, printed, and
# floored at 1 (half an ulp of the result itself, which no f32 evaluation can be held under).


def strongly_off_modules(engine):
    pol, cri = ra.Mlp(engine, 5, H, 2), ra.Mlp(engine, 5, H, 1)
    pol.init(2)
    cri.init(3)
    off = np.arange(H) % 4 != 1
    for m in (pol, cri):
        p = m.get_params()
        p[B1][off] = -1000.0
        m.set_params(p)
    return pol, cri, off


def forward64(p, out_dim, x):
    """(outputs, S = sum_j |w2_j pre_j| per output, the same over the active units + |b2|) of one sample in f64"""
    p = p.astype(np.float64)
    pre = p[:5 * H].reshape(H, 5) @ x.astype(np.float64) + p[B1]
    W2, b2 = p[6 * H:6 * H + out_dim * H].reshape(out_dim, H), p[6 * H + out_dim * H:]
    terms = np.abs(W2 * pre)
    return W2 @ np.maximum(pre, 0.0) + b2, terms.sum(axis=1), (terms * (pre > 0)).sum(axis=1) + np.abs(b2)


def kl_and_loss64(z0, z1, a, adv):
    lp0, lp1 = (z - z.max() - np.log(np.exp(z - z.max()).sum()) for z in (z0, z1))
    return -np.exp(lp1[a] - lp0[a]) * adv, (np.exp(lp0) * (lp0 - lp1)).sum(), lp0, lp1


def test_forward_with_strongly_off_units(engine):
    pol, cri, off = strongly_off_modules(engine)
    pp, cp = pol.get_params(), cri.get_params()
    p_new = (pp + np.float32(0.01) * TW.tangent()).astype(np.float32)
    p_new[B1] = pp[B1]
    traj = ra.Trajectory(engine, 1, 1, 5)
    rng = np.random.default_rng(9)
    xs = (3.0 * rng.standard_normal((FORWARD_SAMPLES, 5))).astype(np.float32)
    # (off the relu edges, by RELU_EDGE of tests/test_gpu_tile_walk.py: this test is about the forward, not the mask)
    def on_an_edge(x):
        for p in (pp, cp, p_new):
            W1, b1 = p[:5 * H].reshape(H, 5).astype(np.float64), p[B1].astype(np.float64)
            if (np.abs(W1 @ x + b1) < TW.RELU_EDGE * (np.abs(W1) @ np.abs(x) + np.abs(b1))).any():
                return True
        return False

    for i in range(FORWARD_SAMPLES):
        while on_an_edge(xs[i].astype(np.float64)):
            xs[i] = (3.0 * rng.standard_normal(5)).astype(np.float32)
    rows = []
    try:
        for variant in (1, 0):
            engine.set_kernel_variant(variant)
            for i, x in enumerate(xs):
                a, adv = np.uint8(i & 1), np.float32(1.0 if i & 2 else -1.0)
                planes = dict(obs=np.zeros((5, 2, 1), dtype=np.float32), action=np.full((1, 1), a),
                              adv=np.full((1, 1), adv), rtg=np.zeros((1, 1), dtype=np.float32))
                planes["obs"][:, 0, 0] = x
                TW.write(traj, planes)
                gc, _ = ra.critic_gradient(cri, traj)
                y = float(gc[7 * H]) / 2.0  # dL/db2 = 2 (y - 0) / B, B = 1
                loss, kl = GW.moved_loss_kl(pol, traj, p_new)
                rows.append((variant, i, y, loss, kl))
    finally:
        engine.set_kernel_variant(0)
        traj.close()
        pol.close()
        cri.close()
    eps = 2.0 ** -24
    ref = []
    for i, x in enumerate(xs):
        a, adv = i & 1, 1.0 if i & 2 else -1.0
        y64, S_c, A_c = forward64(cp, 1, x)
        g32, _ = O.grad_f64_mt("critic", CS, cp, x[None, :], aux=np.zeros(1, dtype=np.float32), f32_samples=True)
        z0, S_0, A_0 = forward64(pp, 2, x)
        z1, S_1, A_1 = forward64(p_new, 2, x)
        loss64, kl64, lp0, lp1 = kl_and_loss64(z0, z1, a, adv)
        ref.append(dict(y=y64[0], y32=g32[7 * H] / 2.0, S=S_c[0], A=A_c[0], loss=loss64, kl=kl64, S0=S_0.max(), S1=S_1.max(), A0=A_0.max(),
                        A1=A_1.max(), ratio=np.exp(lp1[a] - lp0[a]), dlp=np.abs(lp0 - lp1).max(),
                        dp=np.abs(np.exp(lp1) - np.exp(lp0)).sum()))
    # c from kernel variant 1, in units of 2^-24 x its own conditioning
    c1 = max(abs(y - ref[i]["y"]) / (eps * ref[i]["A"]) for variant, i, y, _, _ in rows if variant == 1)
    c = 4.0 * max(c1, 1.0)
    o1 = max(abs(r["y32"] - r["y"]) / (eps * r["A"]) for r in ref)
    print("f32-sample oracle: max |y - f64| = %.3f x 2^-24 x (active sum |w2 pre| + |b2|)" % o1)
    print("variant 1: max |y - f64| = %.3f x 2^-24 x (active sum |w2 pre| + |b2|); c = %.3f" % (c1, c))
    worst = dict(y=0.0, loss=0.0, kl=0.0, y_plain=0.0)
    failures = []
    for variant, i, y, loss, kl in rows:
        r = ref[i]
        # a logit off by dz moves log pi by at most 2 dz: the loss -ratio A by 2 dz ratio |A| (first order; 4: both
        # policies), and KL = sum_a p0_a (lp0_a - lp1_a) by dz1 sum|p1 - p0| + 2 dz0 max|lp0 - lp1| + the floor of
        # tests/test_gpu_tile_walk.py for the rounding of the log-sum-exp itself
        dz0, dz1 = c * eps * r["S0"], c * eps * r["S1"]
        bar_y, bar_loss = c * eps * r["S"], 2.0 * (dz0 + dz1) * r["ratio"] + 1e-6
        bar_kl = dz1 * r["dp"] + 2.0 * dz0 * r["dlp"] + TW.KL_FLOOR
        e_y, e_loss, e_kl = abs(y - r["y"]), abs(loss - r["loss"]), abs(kl - r["kl"])
        if variant == 0:
            worst["y"] = max(worst["y"], e_y / (eps * r["S"]))
            worst["y_plain"] = max(worst["y_plain"], e_y / (eps * r["A"]))
            worst["loss"] = max(worst["loss"], e_loss / bar_loss)
            worst["kl"] = max(worst["kl"], e_kl / bar_kl)
            print("sample %2d: y %.9g f64 %.9g  |diff| %.3e = %.3f x 2^-24 S (S %.1f, active %.3f)  loss diff %.3e (bar %.3e)"
                  "  kl diff %.3e (bar %.3e)" % (i, y, r["y"], e_y, e_y / (eps * r["S"]), r["S"], r["A"], e_loss, bar_loss,
                                                  e_kl, bar_kl))
        if not (e_y <= bar_y and e_loss <= bar_loss and e_kl <= bar_kl):
            failures.append((variant, i, e_y, bar_y, e_loss, bar_loss, e_kl, bar_kl))
    print("variant 0: max |y - f64| = %.3f x 2^-24 S = %.1f x 2^-24 x the plain-f32 conditioning; loss %.3f, kl %.3f of "
          "their bars" % (worst["y"], worst["y_plain"], worst["loss"], worst["kl"]))
    assert not failures, failures
    assert off.sum() == 96 and min(r["S"] / r["A"] for r in ref) > 50.0  # the units that are off dominate S


# ---------------------------------------------------------------- (d) the convention on the other paths
EXACT_SETS = ("ordinary", "lower-weight", "lower-bias")


@pytest.mark.parametrize("name", EXACT_SETS)
def test_convention_on_variant_1(engine, name):
    s = R.SETS[name]
    masks = R.expected_masks(s)
    pol, cri = modules_of(engine, s)
    v, p_new = tangent_and_candidate(s, pol.get_params(), masks)
    n, T = ONE_TILE
    traj = ra.Trajectory(engine, n, T, 5)
    engine.set_kernel_variant(1)
    try:
        for live in ([0], [13]) if not s.copies else (list(range(32)),):
            planes = planes_with(s, n, T, live, np.random.default_rng(3))
            TW.write(traj, planes)
            chk = EdgeChecker("variant 1 %s live %s" % (name, live[0] if len(live) == 1 else "all"), masks, OUT_DIMS,
                              samples=n * T)
            run_edge_passes(chk, s, pol, cri, traj, planes, v, p_new)
    finally:
        engine.set_kernel_variant(0)
        traj.close()
        pol.close()
        cri.close()


def test_convention_on_the_general_fused_kernels(engine):
    """[8, 8] over 5 inputs (tests/test_gpu_gen_tile_walk.py's smallest): layer 1 carries eight designs of the
    `ordinary` set, layer 2 has biases of +-1 and weights on the 2^-10 grid (its pre-activations are b + O(2^-22): off
    every edge), 32 copies of the sample.  Units of layer 1 with exact mask 0: their W1 rows, b1 and layer-2 columns are
    exactly 0 in every gradient and in the Fisher-vector product."""
    s = R.SETS["ordinary"]
    spec = GW.SPECS[0]
    assert spec.hidden == [8, 8] and spec.in_dim == 5
    designs = [s.designs[i] for i in (0, 1, 3, 4, 6, 7, 8, 9)]
    masks = np.array([R.exact_mask(s.x, d) for d in designs])
    assert (masks == 1).sum() >= 2 and (masks == 0).sum() >= 4
    pol, cri = GW.modules(engine, spec)
    n, T = ONE_TILE
    traj = ra.Trajectory(engine, n, T, 5)
    rng = np.random.default_rng(12)
    try:
        nets = {}
        for m, out_dim in ((pol, 2), (cri, 1)):
            p = m.get_params()
            k = 0
            p[k:k + 40] = np.array([d.w for d in designs], dtype=np.float32).reshape(-1)
            p[k + 40:k + 48] = [d.b for d in designs]
            k += 48
            p[k:k + 64] = rng.integers(64, 128, size=64) * rng.choice([-1, 1], size=64) / 1024.0
            p[k + 64:k + 72] = [1, -1, 1, 1, -1, 1, -1, 1]
            k += 72
            p[k:k + 8 * out_dim] = rng.integers(64, 128, size=8 * out_dim) * rng.choice([-1, 1], size=8 * out_dim) / 1024.0
            m.set_params(p)
            nets[out_dim] = p
        pp, cp = nets[2], nets[1]
        planes = TW.dead_batch(n, T)
        planes["obs"][:, 0, :] = np.asarray(s.x, dtype=np.float32)[:, None]
        planes["action"][:] = rng.integers(0, 2, size=(T, n)).astype(np.uint8)
        planes["adv"][:] = (rng.choice([-1.0, 1.0], size=(T, n)) * (0.5 + rng.random((T, n)))).astype(np.float32)
        planes["rtg"][:] = (-3.0 + rng.random((T, n))).astype(np.float32)
        v = np.random.default_rng(7).standard_normal(pol.P).astype(np.float32)
        v[-2:] = 0.5
        p_new = pp.copy()
        p_new[:40] += np.float32(2.0 ** -6) * v[:40]
        p_new[120:128] += np.float32(2.0 ** -6) * v[120:128]
        with GW.Profiled(engine, "relu-edges-general"):
            TW.write(traj, planes)
            x, a, adv, rtg = TW.flat(planes)
            want = GW.reference(spec, pp, cp, v, p_new, x, a, adv, rtg)
            chk = GW.Checker("general [8, 8]", samples=n * T)
            GW.run_passes(chk, spec, pol, cri, traj, want, v, p_new, ppo=True)
            off = masks == 0

            def rows(out_dim):  # W1 rows and b1 of layer 1, the columns of layer 2's weights
                r = np.zeros(48 + 72 + 9 * out_dim, dtype=bool)
                r[:40] = np.repeat(off, 5)
                r[40:48] = off
                r[48:112] = np.tile(off, 8)
                return r

            for what, got, out_dim in (("policy gradient", ra.policy_gradient(pol, traj)[0], 2),
                                       ("fisher-vector", ra.policy_fvp(pol, traj, v, 0.0), 2),
                                       ("ppo step", GW.sgd_ppo_step(pol, traj), 2),
                                       ("critic gradient", ra.critic_gradient(cri, traj)[0], 1)):
                got = np.asarray(got)
                assert not got[rows(out_dim)].any(), (what, got[rows(out_dim)])
                assert got[~rows(out_dim)].any(), what
    finally:
        traj.close()
        pol.close()
        cri.close()
