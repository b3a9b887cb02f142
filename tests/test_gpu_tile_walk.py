"""The tile walk of the fused 5-128 update kernels (bt::deal_tiles, bt::walk_tiles, bt::flush: bf16_tile.hpp)
at the sample counts where it changes behaviour, against f64 — whole-batch sums, and one live tile at a time.

k_policy_bf16 (gradient, PPO, Fisher-vector and evaluation mode) and k_critic_step_mfma<1> deal 32-sample tiles to
"virtual waves", 5 : 3 between the older and the younger wave of a SIMD, walk a ragged last tile on the virtual wave
whose turn it is, and fold f32 partial sums into an f64 image every 16 (policy) or 64 (critic) tiles of a real wave — the
first flush stores, later ones add, a remainder flush follows the walk.  The other oracle tests run sample counts that are
multiples of 32 with at most one tile per virtual wave, or 65,536 x 128 where every wave walks a whole number of flush
periods.  Here the counts come from tests/tile_walk_model.py — a restatement of the walk, checked on the CPU by
tests/test_tile_walk_model.py — computed from the device's compute-unit count: below one workgroup, either side of the
grid's cap, the second round of the virtual waves (eight-wave form and the sixteen-wave evaluation pass), and one tile
either side of each flush period on an older and on a younger wave.  Kernel variant 0; the profile classes show that
the fused kernels, and no per-layer pass, ran.

(a) Whole-batch sums on the random histories of tests/test_gpu_numeric_range.py::history at the case's (n, T):
    policy gradient, loss and entropy, the Fisher-vector product (reg = 0), the critic gradient and loss, loss and KL of
    parameters moved by 0.01 v, and — below the second round — one PPO step under SGD at rate 1 (p0 - p1 is the gradient
    at ratio 1).  Vectors by the criterion of tests/test_gpu_fullsize.py / test_gpu_numeric_range.py: no farther from
    f64 than max(4 x the f32-sample oracle's distance on the same samples, 1e-6) of the largest entry; scalars as in
    tests/test_gpu_parity.py.  (KL below 32,768 samples — parity's smallest count — gets a per-sample floor, see KL_FLOOR;
    the few samples with a pre-activation that f32 cannot tell from 0 are redrawn first, see RELU_EDGE: the first run
    missed five bars by exactly one such (sample, unit) term each.)

(b) One live tile on a dead batch.  A whole-batch sum over 10^5 tiles dilutes a lost tile to 10^-5; here a tile that is
    dropped, walked twice, walked under the wrong validity mask or flushed over costs the whole expected result.  Both
    modules get b1 = -1 on every hidden unit, output weights on the 2^-10 grid and the critic b2 = 0.25.  A DEAD sample —
    observation 0, advantage 0, action 0, return 0.25 — has every pre-activation -1: no active unit, and its output is
    b2 exactly in any summation order (all products dyadic).  With a tangent whose two b2 entries are equal and
    candidate parameters that differ from the old ones in W1 and W2 only (W2 again on the grid: off it, the two halves
    of relu(x) = (x + |x|) / 2 no longer cancel exactly on a dead sample and its KL is ~1e-16, not 0) a dead sample adds
    exactly zero to every sum of every pass but the entropy, which is H(softmax(b2)) per dead sample.  That is asserted
    on an all-dead batch first.  Then the samples of ONE tile are made live — observations N(0, 3^2), random actions,
    advantages N(0, 1), returns 10 N(0, 1) — and every pass must equal m / B times the f64 result over those m samples,
    by the yardstick of (a) relative to the probe's own largest entry.  The tiles: tile_walk_model.probes_for.

Measured distances and wall times: DESIGN 24, "who tests what".
"""
import time

import numpy as np
import pytest

import oracle as O
import tile_walk_model as M

pytestmark = pytest.mark.gpu

ra = pytest.importorskip("relearn_amd")

H = 128
PS, CS = O.MlpShape(5, H, 2), O.MlpShape(5, H, 1)
P_POL = 5 * H + H + 2 * H + 2
W2P, W2C = slice(6 * H, 8 * H), slice(6 * H, 7 * H)
B1 = slice(5 * H, 6 * H)
CRITIC_B2 = np.float32(0.25)
CHUNK = 1 << 16
PARITY_SMALLEST = 32768
# tests/test_gpu_parity.py holds KL to 1e-5 max(1e-3, KL) at 32,768 samples and more, where the per-sample rounding of
# log pi averages out.  It does not on a handful of samples: KL = sum_a p0_a (lp0_a - lp_a), and lp_a = z_a - lse carries
# the rounding of lse (one v_log_f32, two additions of values up to |z| + 0.7 < 8: half an ulp of 4 .. 8, 2.4e-7, each)
# into BOTH terms with weights that sum to one — first order, ~3 roundings for each of lp0 and lp: 1.5e-6 per sample at
# the worst.  Batches below parity's smallest count and the m-sample probes get that much more, as 2e-6 per sample.
KL_FLOOR = 2e-6
# The derivative of relu at a pre-activation that f32 cannot tell from 0 is not a question the f64 oracle can answer for
# an f32 kernel.  pre = b + sum of five products carries ~6 roundings of 2^-24 of its terms' size in any f32 evaluation
# (the oracle's fma chain, the kernels' exact piece products under f32 accumulation alike); with 128 units and 10^5 .. 10^6
# samples a batch holds about one (sample, unit) pair with |pre| below that, the device and the f64 oracle take relu' on
# different sides, and the gradient moves by that ONE pair's term — which the random returns 10 N(0, 1) make 1e-5 .. 1e-4
# of the critic gradient's largest entry.  Measured on the unmoved histories, kernel variant 0, 256 compute units:
#   second-round-NV-tail    critic gradient 4.833e-06 off = the term of sample 261853, unit 102 (pre = 5.1e-10): 4.832e-06
#   second-round-NV+1-tail  critic gradient 7.522e-06 off = sample 25208, unit 21 (pre = 1.5e-10): 7.522e-06
#   eval-2NVE+1-tail        critic gradient 3.918e-05 off = sample 204012, unit 53 (pre = -3.9e-09): 3.918e-05
#   eval-NVE-1-tail         policy gradient 5.844e-08 off = sample 23337, unit 68 (pre = 2.0e-08): 5.841e-08
# against bars of 3.5e-07 and 2.4e-09: no tile lost, no tolerance problem.  So the samples with a pre-activation within
# 2^-20 of its terms' size (16 roundings) are redrawn before the batch is used: 0.02 % of them, none otherwise special.
RELU_EDGE = 2.0 ** -20
EDGE_CHUNK = 1 << 13


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def history(n, T, seed=0):
    """tests/test_gpu_numeric_range.py::history at unit feature scales and (n, T): the same draws in the same order"""
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((5, T + 1, n)).astype(np.float32)
    return dict(obs=obs, action=rng.integers(0, 2, size=(T, n)).astype(np.uint8),
                adv=rng.standard_normal((T, n)).astype(np.float32),
                rtg=(10.0 * rng.standard_normal((T, n))).astype(np.float32))


def on_a_relu_edge(modules, x):
    """the samples of x [m][5] with a pre-activation of one of `modules` (parameter vectors) inside RELU_EDGE: a coarse f32
    pass keeps the samples with some |pre| < 1e-3, f64 decides among them"""
    bad = np.zeros(len(x), dtype=bool)
    xmax = float(np.abs(x).max()) if len(x) else 0.0
    for p in modules:
        W1, b1 = p[:5 * H].reshape(H, 5), p[B1]
        # (the coarse pass must not lose an edge: the edge's width and the f32 pass's own error stay far below 1e-3)
        assert 2.0 ** -18 * (np.abs(W1).sum(axis=1).max() * xmax + np.abs(b1).max()) < 5e-4
        W1d, b1d = W1.astype(np.float64), b1.astype(np.float64)
        for lo in range(0, len(x), EDGE_CHUNK):
            xs = x[lo:lo + EDGE_CHUNK]
            near = np.flatnonzero((np.abs(xs @ W1.T + b1) < 1e-3).any(axis=1))
            xn = xs[near].astype(np.float64)
            pre, size = xn @ W1d.T + b1d, np.abs(xn) @ np.abs(W1d).T + np.abs(b1d)
            bad[lo + near] |= (np.abs(pre) < RELU_EDGE * size).any(axis=1)
    return bad


def off_the_relu_edges(modules, x, draw):
    """redraw (draw(count) -> [count][5]) the samples of x that sit on a relu edge of `modules`, in place; their indices"""
    moved = np.flatnonzero(on_a_relu_edge(modules, x))
    bad = moved
    while len(bad):
        x[bad] = draw(len(bad))
        bad = bad[on_a_relu_edge(modules, x[bad])]
    return moved


def write(traj, h):
    traj.write(ra.TRAJ_OBS, h["obs"])
    traj.write(ra.TRAJ_ACTION, h["action"])
    traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
    traj.write(ra.TRAJ_RETURNS, h["rtg"])


def flat(h):
    x, a = O.flat_samples(h)
    return x, a.astype(np.uint8), h["adv"].reshape(-1), h["rtg"].reshape(-1)


def policy_scalars64(p_new, p_old, x, a, adv):
    """f64, in chunks: SUMS over the samples of the entropy of pi_old, of -ratio A and of KL(pi_old || pi_new)"""
    def log_pi(p, xs):
        p = p.astype(np.float64)
        hid = np.maximum(xs @ p[:5 * H].reshape(H, 5).T + p[B1], 0.0)
        z = hid @ p[W2P].reshape(2, H).T + p[8 * H:]
        zmax = z.max(axis=1, keepdims=True)
        return z - zmax - np.log(np.exp(z - zmax).sum(axis=1, keepdims=True))

    ent = loss = kl = 0.0
    for lo in range(0, len(x), CHUNK):
        xs = x[lo:lo + CHUNK].astype(np.float64)
        rows = np.arange(len(xs))
        act = a[lo:lo + CHUNK].astype(np.int64)
        lp0 = log_pi(p_old, xs)
        ent -= (np.exp(lp0) * lp0).sum()
        if p_new is not None:
            lp1 = log_pi(p_new, xs)
            loss -= (np.exp(lp1[rows, act] - lp0[rows, act]) * adv[lo:lo + CHUNK].astype(np.float64)).sum()
            kl += (np.exp(lp0) * (lp0 - lp1)).sum()
    return ent, loss, kl


class Checker:
    """the comparisons of one case, printed before they are asserted; `scale` = m / B turns the references — means over
    the m samples they were computed on — into what a batch of B samples of which only those m count must give"""

    def __init__(self, tag, scale=1.0, samples=None):
        self.tag, self.scale, self.floor = tag, scale, 0.0
        if samples is not None and samples < PARITY_SMALLEST:
            self.floor = KL_FLOOR

    def vector(self, name, got, want64, want32, extra_abs=0.0):
        want64, want32 = self.scale * want64, self.scale * want32
        top = np.abs(want64).max()
        err, bar = np.abs(np.asarray(got, dtype=np.float64) - want64).max(), max(4 * rel_err(want32, want64), 1e-6) * top
        print("%s %-16s |got - f64| %.3e  bar %.3e (+ %.1e)  of max %.3e: %.3e, f32 oracle %.3e"
              % (self.tag, name, err, bar, extra_abs, top, err / max(top, 1e-300), rel_err(want32, want64)))
        assert np.all(np.isfinite(got)) and top > 0.0, (self.tag, name)
        assert err < bar + extra_abs, (self.tag, name, err, bar, extra_abs)

    def scalar(self, name, got, want, bar):
        want, bar = self.scale * want, self.scale * bar
        print("%s %-16s got %.9g  f64 %.9g  |diff| %.3e  bar %.3e" % (self.tag, name, got, want, abs(got - want), bar))
        assert np.isfinite(got) and abs(got - want) <= bar, (self.tag, name, got, want, bar)


def run_passes(chk, case, cus, pol, cri, traj, x, a, adv, rtg, v, p_new, ent_extra=0.0, ppo=True):
    """every pass the case runs, on whatever the planes hold, against the f64 results over the samples (x, a, adv, rtg)"""
    m = len(x)
    if "policy" in case.passes or "eval" in case.passes:
        ent64, loss_new64, kl64 = policy_scalars64(p_new, pol.get_params(), x, a, adv)
    if "policy" in case.passes:
        pp = pol.get_params()
        g_d, loss_d, ent_d = ra.policy_gradient(pol, traj)
        g64, l64 = O.grad_f64_mt("policy", PS, pp, x, a, adv)
        g32, _ = O.grad_f64_mt("policy", PS, pp, x, a, adv, f32_samples=True)
        chk.vector("policy gradient", g_d, g64, g32)
        chk.scalar("policy loss", loss_d, l64, 1e-5 * max(1.0, abs(l64)))
        # (the entropy is the one sum a dead sample takes part in: ent_extra is its share, not scaled)
        print("%s entropy          got %.9g  f64 %.9g" % (chk.tag, ent_d, chk.scale * ent64 / m + ent_extra))
        assert abs(ent_d - (chk.scale * ent64 / m + ent_extra)) < 1e-5
        if ppo and M.below_second_round(case, cus):
            cfg = ra.optimizer_config_default(ra.OPTIMIZER_SGD)
            cfg.learning_rate = 1.0
            step = ra.ppo_config_default()
            step.opt_steps_per_update = 1
            opt = ra.Optimizer(pol, cfg)
            ra.ppo_update(pol, opt, traj, step)
            p1 = pol.get_params()
            opt.close()
            pol.set_params(pp)
            chk.vector("ppo step", pp.astype(np.float64) - p1.astype(np.float64), g64, g32,
                       extra_abs=2.0 ** -24 * np.abs(pp).max())
    if "fvp" in case.passes:
        pp = pol.get_params()
        h_d = ra.policy_fvp(pol, traj, v, 0.0)
        h64, _ = O.grad_f64_mt("fvp", PS, pp, x, v=v)
        h32, _ = O.grad_f64_mt("fvp", PS, pp, x, v=v, f32_samples=True)
        chk.vector("fisher-vector", h_d, h64, h32)
    if "eval" in case.passes:
        pp = pol.get_params()
        pol.set_params(p_new)
        try:
            loss_d, kl_d = ra.policy_loss_kl(pol, traj, pp)
        finally:
            pol.set_params(pp)
        chk.scalar("moved loss", loss_d, loss_new64 / m, 1e-5 * max(1.0, abs(loss_new64 / m)))
        chk.scalar("moved kl", kl_d, kl64 / m, 1e-5 * max(1e-3, abs(kl64 / m)) + chk.floor)
        assert kl64 > 0.0, "the candidate parameters must move the policy"
    if "critic" in case.passes:
        cp = cri.get_params()
        gc_d, lc_d = ra.critic_gradient(cri, traj)
        gc64, lc64 = O.grad_f64_mt("critic", CS, cp, x, aux=rtg)
        gc32, _ = O.grad_f64_mt("critic", CS, cp, x, aux=rtg, f32_samples=True)
        chk.vector("critic gradient", gc_d, gc64, gc32)
        chk.scalar("critic loss", lc_d, lc64, 1e-5 * lc64)


class Profiled:
    """launch counts per kernel class over the block: the fused kernels ran, and no per-layer pass did"""

    def __init__(self, engine, case):
        self.engine, self.case = engine, case

    def __enter__(self):
        self.engine.set_kernel_variant(0)
        self.engine.profile_enable(True)
        self.engine.profile_read(reset=True)
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, kind, *rest):
        counts = {k: int(c) for k, (_, c) in self.engine.profile_read(reset=True).items()}
        self.engine.profile_enable(False)
        print("%s wall %.2f s, launches %s" % (self.case.name, time.perf_counter() - self.t0,
                                               {k: c for k, c in counts.items() if c}))
        if kind is None:
            want = {"policy": "policy_fused", "eval": "policy_fused", "fvp": "policy_fvp", "critic": "critic_fused"}
            for p in self.case.passes:
                assert counts[want[p]] > 0, (self.case.name, want[p], counts)
            assert counts["policy_pass"] == 0 and counts["backward"] == 0 and counts["critic_fwd"] == 0, counts


@pytest.fixture(scope="module")
def table(engine):
    cus = int(engine.info()[2])
    return cus, {c.name: c for c in M.cases(cus)}


def tangent(seed=7):
    return np.random.default_rng(seed).standard_normal(P_POL).astype(np.float32)


@pytest.mark.parametrize("name", M.case_names())
def test_whole_batch_sums_at_the_walks_edges(engine, table, name):
    cus, cases = table
    case = cases[name]
    print("%s: B = %d = %d x %d on %d compute units, %d full tiles + %d" % (name, case.B, case.n, case.T, cus,
                                                                            case.B // 32, case.B % 32))
    pol, cri = ra.Mlp(engine, 5, H, 2), ra.Mlp(engine, 5, H, 1)
    pol.init(2)
    cri.init(3)
    traj = ra.Trajectory(engine, case.n, case.T, 5)
    try:
        with Profiled(engine, case):
            h = history(case.n, case.T)
            x, a, adv, rtg = flat(h)
            edge_of = ([pol.get_params()] if "policy" in case.passes else []) + \
                      ([cri.get_params()] if "critic" in case.passes else [])
            rng = np.random.default_rng([1, case.B])
            moved = off_the_relu_edges(edge_of, x, lambda k: rng.standard_normal((k, 5)).astype(np.float32))
            h["obs"].reshape(5, (case.T + 1) * case.n)[:, moved] = x[moved].T  # (flat sample b = t n + lane, b < T n)
            print("%s: %d of %d samples redrawn off the relu edges" % (name, len(moved), case.B))
            write(traj, h)
            v = tangent()
            p_new = (pol.get_params() + np.float32(0.01) * v).astype(np.float32)
            run_passes(Checker(name, samples=case.B), case, cus, pol, cri, traj, x, a, adv, rtg, v, p_new)
    finally:
        traj.close()
        pol.close()
        cri.close()


def dyadic_modules(engine):
    """b1 = -1 on every hidden unit, the output weights on the 2^-10 grid, the critic's b2 = 0.25"""
    pol, cri = ra.Mlp(engine, 5, H, 2), ra.Mlp(engine, 5, H, 1)
    pol.init(2)
    cri.init(3)
    for m, w2 in ((pol, W2P), (cri, W2C)):
        p = m.get_params()
        p[B1] = -1.0
        p[w2] = np.round(p[w2] * 1024.0) / 1024.0
        if m is cri:
            p[7 * H] = CRITIC_B2
        assert np.abs(p[w2]).max() > 0.05
        m.set_params(p)
    return pol, cri


def dead_batch(n, T):
    return dict(obs=np.zeros((5, T + 1, n), dtype=np.float32), action=np.zeros((T, n), dtype=np.uint8),
                adv=np.zeros((T, n), dtype=np.float32), rtg=np.full((T, n), CRITIC_B2, dtype=np.float32))


def assert_dead_batch_is_silent(case, cus, pol, cri, traj, v, p_new, h_dead):
    """a dead sample adds exactly nothing to any sum but the entropy"""
    pp = pol.get_params()
    if "policy" in case.passes:
        g, loss, ent = ra.policy_gradient(pol, traj)
        assert not g.any() and loss == 0.0, ("policy gradient", np.abs(g).max(), loss)
        assert abs(ent - h_dead) < 1e-6, (ent, h_dead)
        if M.below_second_round(case, cus):
            cfg = ra.optimizer_config_default(ra.OPTIMIZER_SGD)
            cfg.learning_rate = 1.0
            step = ra.ppo_config_default()
            step.opt_steps_per_update = 1
            opt = ra.Optimizer(pol, cfg)
            ra.ppo_update(pol, opt, traj, step)
            opt.close()
            assert np.array_equal(pol.get_params(), pp), "ppo step"
    if "fvp" in case.passes:
        hv = ra.policy_fvp(pol, traj, v, 0.0)
        assert not hv.any(), ("fisher-vector product", np.abs(hv).max())
    if "eval" in case.passes:
        pol.set_params(p_new)
        try:
            loss, kl = ra.policy_loss_kl(pol, traj, pp)
        finally:
            pol.set_params(pp)
        assert loss == 0.0 and kl == 0.0, ("moved loss / kl", loss, kl)
    if "critic" in case.passes:
        g, loss = ra.critic_gradient(cri, traj)
        assert not g.any() and loss == 0.0, ("critic gradient", np.abs(g).max(), loss)


@pytest.mark.parametrize("name", M.case_names())
def test_one_live_tile_on_a_dead_batch(engine, table, name):
    cus, cases = table
    case = cases[name]
    B, n, T = case.B, case.n, case.T
    pol, cri = dyadic_modules(engine)
    traj = ra.Trajectory(engine, n, T, 5)
    try:
        with Profiled(engine, case):
            pp = pol.get_params()
            v = tangent()
            v[8 * H:] = 0.5  # equal b2 entries: the tangent logits of a dead sample do not differ
            p_new = pp.copy()
            p_new[:5 * H] += np.float32(0.01) * v[:5 * H]
            p_new[W2P] = np.round((pp[W2P] + np.float32(0.01) * v[W2P]) * 1024.0) / 1024.0
            assert np.mean(p_new[W2P] != pp[W2P]) > 0.9
            z = pp[8 * H:].astype(np.float64)
            lp = z - z.max() - np.log(np.exp(z - z.max()).sum())
            h_dead = float(-(np.exp(lp) * lp).sum())
            planes = dead_batch(n, T)
            write(traj, planes)
            assert_dead_batch_is_silent(case, cus, pol, cri, traj, v, p_new, h_dead)
            # views of the planes in the flat sample order b = t n + lane
            obs_flat = planes["obs"].reshape(5, (T + 1) * n)
            act_flat, adv_flat, rtg_flat = (planes[k].reshape(-1) for k in ("action", "adv", "rtg"))
            probes = M.probes_for(case, cus)
            for g in probes:
                lo, hi = 32 * g, min(32 * g + 32, B)
                m = hi - lo
                assert m == (32 if g < B // 32 else B % 32)
                rng = np.random.default_rng([g, B])
                x = (3.0 * rng.standard_normal((m, 5))).astype(np.float32)
                off_the_relu_edges([pp, cri.get_params()], x, lambda k: (3.0 * rng.standard_normal((k, 5))).astype(np.float32))
                obs_flat[:, lo:hi] = x.T
                act_flat[lo:hi] = rng.integers(0, 2, size=m).astype(np.uint8)
                adv_flat[lo:hi] = rng.standard_normal(m).astype(np.float32)
                rtg_flat[lo:hi] = (10.0 * rng.standard_normal(m)).astype(np.float32)
                write(traj, planes)
                chk = Checker("%s tile %d (%d live of %d)" % (name, g, m, B), scale=m / B, samples=m)
                run_passes(chk, case, cus, pol, cri, traj, x, act_flat[lo:hi].copy(), adv_flat[lo:hi].copy(),
                           rtg_flat[lo:hi].copy(), v, p_new, ent_extra=(B - m) / B * h_dead)
                obs_flat[:, lo:hi], act_flat[lo:hi], adv_flat[lo:hi], rtg_flat[lo:hi] = 0.0, 0, 0.0, CRITIC_B2
            print("%s: probed tiles %s" % (name, probes))
    finally:
        traj.close()
        pol.close()
        cri.close()
