"""The tile walk of the general-MLP fused kernels (k_gen_mfma, k_gen_pair, launch_gen_mfma: kernels_gen_mfma.hip,
DESIGN 27) at the sample counts where it changes behaviour, against f64 — whole-batch sums, and one live tile at a time.

Both kernels deal 32-sample tiles round-robin to the walkers of a grid of one workgroup per four tiles, capped at the
compute-unit count: a wave is a walker in k_gen_mfma, a PAIR of waves in k_gen_pair, where every pair runs as many
iterations as the busiest one — idle ones on zeros.  A walker fetches one tile ahead (past the end: sample B - 1 under
an all-false mask), and folds its f32 partial sums into its f64 slab row after every 64 tiles and after its last: the
row's first flush stores, later ones add.  The other tests of these kernels stop at 197 tiles (no walker has a second
one) or run 65,536 tiles on 1,024 walkers, 64 each: one storing flush, no idle iteration after a live one, no uneven
round.  Here the counts come from tests/gen_walk_model.py — a restatement of the walk, checked on the CPU by
tests/test_gen_walk_model.py — computed from the device's compute-unit count.  Kernel variant 0; the profile classes
show that no per-layer pass ran.

Modules, the narrowest that reach the kernels (the walk does not depend on the width: layers are padded to 64 or 128
units), Relu hidden layers because Relu permits exactly dead samples:
  pair-8-8       [8, 8] Relu / Identity over 5 inputs: k_gen_pair<., 2, 4> for the gradient, PPO, Fisher-vector and
                 critic passes, k_gen_mfma<PASS_EVAL, 2, 2> for loss / KL
  wave-72        [72] Relu / Identity over 7 inputs (over 4 or 5 it would be the non-general fused module; with 7 the
                 bias input sits in the last slot of the input fragment): k_gen_mfma<., 1, 4> in all five modes
  pair-33-tanh   [33] Relu / Tanh (pair, NL = 1) and
  pair-8-8-8     [8, 8, 8] Relu / Identity (pair, NL = 3; its Fisher-vector pass takes the per-layer kernels by design
                 and is left out), both at the four cases from 64 W tiles up only.

(a) Whole-batch sums on host-made planes: policy gradient with loss and entropy, the Fisher-vector product (reg = 0),
    loss and KL of parameters moved by 0.01 v, the critic gradient and loss, and one PPO step under SGD at rate 1
    (p0 - p1 is the gradient at ratio 1), against the f64 restatement of tests/test_gpu_general_mlp.py (forward64,
    backward64, jvp64).  Vector bars are that file's for these kernels — 2e-5 of the largest entry for gradients, 5e-5
    for the Fisher-vector product; scalar bars are tests/test_gpu_tile_walk.py's (its Checker and KL_FLOOR).  Batches
    above 2^17 samples are the cyclic repetition of BASE = 8,191 distinct samples (prime: no two tiles of a walker
    hold the same samples, and a tile lost, doubled or flushed over shifts the sum by the samples of THAT tile); the
    reference is then the multiplicity-weighted sum over the base.  Samples with a hidden pre-activation that f32
    cannot tell from 0 are redrawn first (RELU_EDGE of test_gpu_tile_walk.py, every layer); at most 0.1 % may be.

(b) One live tile on a dead batch, the recipe of test_gpu_tile_walk.py: every hidden bias -1, every weight after the
    first layer on the 2^-10 grid, the critic's output bias 0.25 (Tanh output: output biases 0, dead return 0).  A DEAD
    sample — observation 0, advantage 0, action 0, return = the critic's dead output — has no active unit and its
    outputs are the output biases exactly; with a tangent whose output-bias entries are equal and candidate parameters
    that differ from the old ones in weights only it adds exactly zero to every sum of every pass but the entropy.
    Asserted on an all-dead batch first (an idle iteration of a pair, which runs on zeros WITHOUT the bias input, is
    then silent only through its validity mask).  Then the samples of ONE tile of gen_walk_model.probe_tiles are made
    live and every pass must equal m / B times the f64 result over those m samples, by the bars of (a) relative to the
    probe's own largest entry.  A live sample is drawn until it reaches the output: with biases of -1 a random
    observation often leaves a whole hidden layer of 8 units inactive (62 % of them for [8, 8], 93 % for [8, 8, 8]), and
    the first run's ragged tiles of one or two such samples probed nothing (reference and device both 0 up to 1e-19).
    The PPO step runs in probes only below the second round: above it m / B of a gradient is under the f32 resolution
    of the parameters.

Measured distances and wall times: DESIGN 27, "who tests what".
"""
import time

import numpy as np
import pytest

import gen_walk_model as M
import test_gpu_general_mlp as G
import test_gpu_tile_walk as TW

pytestmark = pytest.mark.gpu

ra = pytest.importorskip("relearn_amd")

GRAD_BAR, FVP_BAR = 2e-5, 5e-5  # tests/test_gpu_general_mlp.py: test_gradients_and_fisher_vector_products
BASE = 8191
DISTINCT_LIMIT = 1 << 17
CHUNK = 1 << 15
MAX_REDRAWN = 1e-3

Spec = type("Spec", (), {})


def spec(name, in_dim, hidden, out_act, form, fvp, only=None):
    s = Spec()
    s.name, s.in_dim, s.hidden, s.act, s.out_act, s.form, s.fvp, s.only = name, in_dim, hidden, "Relu", out_act, form, fvp, only
    return s


SPECS = [spec("pair-8-8", 5, [8, 8], "Identity", M.PAIR, True),
         spec("wave-72", 7, [72], "Identity", M.WAVE, True),
         spec("pair-33-tanh", 5, [33], "Tanh", M.PAIR, True, only=M.FLUSH_CASES),
         spec("pair-8-8-8", 5, [8, 8, 8], "Identity", M.PAIR, False, only=M.FLUSH_CASES)]
PARAMS = [pytest.param(s, name, id="%s@%s" % (s.name, name)) for s in SPECS for name in M.case_names()
          if s.only is None or name in s.only]


def net_of(s, p, out_dim):
    return G.unflatten(np.asarray(p), s.in_dim, s.hidden, out_dim)


def log_softmax(z):
    zmax = z.max(axis=1, keepdims=True)
    return z - zmax - np.log(np.exp(z - zmax).sum(axis=1, keepdims=True))


def reference(s, pp, cp, v, p_new, x, a, adv, rtg, wgt=None):
    """f64, in chunks: every result the passes return, as the weighted MEAN over the samples (x, a, adv, rtg) with
    multiplicities wgt (default 1): the restatement of tests/test_gpu_general_mlp.py"""
    m = len(x)
    wgt = np.ones(m) if wgt is None else wgt.astype(np.float64)
    B = wgt.sum()
    pnet, tnet, nnet, cnet = net_of(s, pp, 2), net_of(s, v, 2), net_of(s, p_new, 2), net_of(s, cp, 1)
    r = dict(g=0.0, loss=0.0, ent=0.0, fvp=0.0, loss_new=0.0, kl=0.0, cg=0.0, closs=0.0)
    for lo in range(0, m, CHUNK):
        xs, w = x[lo:lo + CHUNK].astype(np.float64), wgt[lo:lo + CHUNK]
        rows, act = np.arange(len(xs)), a[lo:lo + CHUNK].astype(np.int64)
        ad, rt = adv[lo:lo + CHUNK].astype(np.float64), rtg[lo:lo + CHUNK].astype(np.float64)
        z, acts = G.forward64(pnet, xs, s.act, s.out_act)
        lp = log_softmax(z)
        p = np.exp(lp)
        r["g"] += G.backward64(pnet, xs, acts, -(w * ad)[:, None] * (np.eye(2)[act] - p) / B)
        r["loss"] -= (w * ad).sum() / B
        r["ent"] -= (w[:, None] * p * lp).sum() / B
        _, tz = G.jvp64(pnet, tnet, xs, s.act, s.out_act)
        r["fvp"] += G.backward64(pnet, xs, acts, w[:, None] * p * (tz - (p * tz).sum(axis=1, keepdims=True)) / B)
        lp1 = log_softmax(G.forward64(nnet, xs, s.act, s.out_act)[0])
        r["loss_new"] -= (w * np.exp(lp1[rows, act] - lp[rows, act]) * ad).sum() / B
        r["kl"] += (w[:, None] * p * (lp - lp1)).sum() / B
        val, cacts = G.forward64(cnet, xs, s.act, s.out_act)
        d = val[:, 0] - rt
        r["cg"] += G.backward64(cnet, xs, cacts, (2.0 * w * d / B)[:, None])
        r["closs"] += (w * d * d).sum() / B
    return r


def on_a_relu_edge(s, modules, x):
    """the samples of x with a hidden pre-activation, of any layer of one of `modules` (parameter vectors with their
    output widths), within TW.RELU_EDGE of its terms' size: the idea of test_gpu_tile_walk.off_the_relu_edges for any depth"""
    bad = np.zeros(len(x), dtype=bool)
    for p, out_dim in modules:
        net = net_of(s, p, out_dim)
        for lo in range(0, len(x), CHUNK):
            h = x[lo:lo + CHUNK].astype(np.float64)
            for W, b in net[:-1]:
                pre, size = h @ W.T + b, np.abs(h) @ np.abs(W).T + np.abs(b)
                bad[lo:lo + CHUNK] |= (np.abs(pre) < TW.RELU_EDGE * size).any(axis=1)
                h = np.maximum(pre, 0.0)
    return bad


def cut_off_from_the_output(s, modules, x):
    """the samples of x that leave no unit of the last hidden layer of one of `modules` active: such a sample is dead to
    every weight (only the output biases see it), and a probe tile made of one or two of them probes nothing"""
    bad = np.zeros(len(x), dtype=bool)
    for p, out_dim in modules:
        net = net_of(s, p, out_dim)
        h = x.astype(np.float64)
        for W, b in net[:-1]:
            h = np.maximum(h @ W.T + b, 0.0)
        bad |= ~(h > 0.0).any(axis=1)
    return bad


def off_the_relu_edges(s, modules, x, draw, reach_the_output=False):
    """redraw (draw(count) -> [count][in_dim]) the samples of x on a relu edge of `modules` — and, for the few samples of
    a probe tile, those cut off from the output — in place; their indices"""
    def unusable(xs):
        bad = on_a_relu_edge(s, modules, xs)
        return bad | cut_off_from_the_output(s, modules, xs) if reach_the_output else bad

    moved = np.flatnonzero(unusable(x))
    bad = moved
    while len(bad):
        x[bad] = draw(len(bad))
        bad = bad[unusable(x[bad])]
    return moved


class Checker(TW.Checker):
    """test_gpu_tile_walk's scalars, and vectors by the bars of tests/test_gpu_general_mlp.py: `rel` of the reference's
    largest entry"""

    def vector(self, name, got, want64, rel, extra_abs=0.0):
        want64 = self.scale * np.asarray(want64, dtype=np.float64)
        top = np.abs(want64).max()
        err, bar = np.abs(np.asarray(got, dtype=np.float64) - want64).max(), rel * top
        print("%s %-16s |got - f64| %.3e  bar %.3e (+ %.1e)  of max %.3e: %.3e" % (self.tag, name, err, bar, extra_abs, top,
                                                                                  err / max(top, 1e-300)))
        assert np.all(np.isfinite(got)) and top > 0.0, (self.tag, name)
        assert err <= bar + extra_abs, (self.tag, name, err, bar, extra_abs)


def sgd_ppo_step(pol, traj):
    """p0 - p1 of one PPO step under SGD at rate 1: the gradient at ratio 1; the parameters are put back"""
    pp = pol.get_params()
    cfg = ra.optimizer_config_default(ra.OPTIMIZER_SGD)
    cfg.learning_rate = 1.0
    step = ra.ppo_config_default()
    step.opt_steps_per_update = 1
    opt = ra.Optimizer(pol, cfg)
    try:
        ra.ppo_update(pol, opt, traj, step)
        p1 = pol.get_params()
    finally:
        opt.close()
        pol.set_params(pp)
    return pp.astype(np.float64) - p1.astype(np.float64)


def moved_loss_kl(pol, traj, p_new):
    pp = pol.get_params()
    pol.set_params(p_new)
    try:
        return ra.policy_loss_kl(pol, traj, pp)
    finally:
        pol.set_params(pp)


def run_passes(chk, s, pol, cri, traj, want, v, p_new, ppo, ent_extra=0.0):
    """every pass on whatever the planes hold, against `want` (reference(): means over the samples that count)"""
    pp = pol.get_params()
    g_d, loss_d, ent_d = ra.policy_gradient(pol, traj)
    chk.vector("policy gradient", g_d, want["g"], GRAD_BAR)
    chk.scalar("policy loss", loss_d, want["loss"], 1e-5 * max(1.0, abs(want["loss"])))
    # (the entropy is the one sum a dead sample takes part in: ent_extra is its share, not scaled)
    ent_want = chk.scale * want["ent"] + ent_extra
    print("%s entropy          got %.9g  f64 %.9g" % (chk.tag, ent_d, ent_want))
    assert abs(ent_d - ent_want) < 1e-5
    if ppo:
        chk.vector("ppo step", sgd_ppo_step(pol, traj), want["g"], GRAD_BAR, extra_abs=2.0 ** -24 * np.abs(pp).max())
    if s.fvp:
        chk.vector("fisher-vector", ra.policy_fvp(pol, traj, v, 0.0), want["fvp"], FVP_BAR)
    loss_d, kl_d = moved_loss_kl(pol, traj, p_new)
    chk.scalar("moved loss", loss_d, want["loss_new"], 1e-5 * max(1.0, abs(want["loss_new"])))
    chk.scalar("moved kl", kl_d, want["kl"], 1e-5 * max(1e-3, abs(want["kl"])) + chk.floor)
    assert want["kl"] > 0.0, "the candidate parameters must move the policy"
    gc_d, lc_d = ra.critic_gradient(cri, traj)
    chk.vector("critic gradient", gc_d, want["cg"], GRAD_BAR)
    chk.scalar("critic loss", lc_d, want["closs"], 1e-5 * want["closs"])


class Profiled:
    """launch counts per kernel class over the block: no per-layer pass ran"""

    def __init__(self, engine, tag):
        self.engine, self.tag = engine, tag

    def __enter__(self):
        self.engine.set_kernel_variant(0)
        self.engine.profile_enable(True)
        self.engine.profile_read(reset=True)
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, kind, *rest):
        counts = {k: int(c) for k, (_, c) in self.engine.profile_read(reset=True).items()}
        self.engine.profile_enable(False)
        print("%s wall %.2f s, launches %s" % (self.tag, time.perf_counter() - self.t0, {k: c for k, c in counts.items() if c}))
        if kind is None:
            assert counts["policy_pass"] == 0 and counts["backward"] == 0 and counts["critic_fwd"] == 0, counts


@pytest.fixture(scope="module")
def table(engine):
    cus = int(engine.info()[2])
    return cus, {c.name: c for c in M.cases(cus)}


def modules(engine, s):
    pol = ra.Mlp(engine, s.in_dim, s.hidden, 2, s.act, s.out_act)
    cri = ra.Mlp(engine, s.in_dim, s.hidden, 1, s.act, s.out_act)
    pol.init(2)
    cri.init(3)
    return pol, cri


def planes_of(s, case, x, a, adv, rtg):
    """the trajectory planes whose flat sample b = t n + lane (b < B) is sample b mod len(x) of (x, a, adv, rtg)"""
    idx = np.arange(case.B) % len(x)
    obs = np.zeros((s.in_dim, (case.T + 1) * case.n), dtype=np.float32)
    obs[:, :case.B] = x[idx].T
    shape = (case.T, case.n)
    return dict(obs=obs.reshape(s.in_dim, case.T + 1, case.n), action=a[idx].reshape(shape), adv=adv[idx].reshape(shape),
                rtg=rtg[idx].reshape(shape)), np.bincount(idx, minlength=len(x))


def describe(s, case, cus):
    tiles = {w: sum(t is not None for t in v) for w, v in M.walk(case.B, cus, s.form).items()}
    iters = {w: len(v) for w, v in M.walk(case.B, cus, s.form).items()}
    k = min(tiles.values())
    adds = sum(1 for w in iters if iters[w] and len(M.flush_pattern(iters[w])) > 1)
    print("%s@%s: B = %d = %d x %d on %d compute units, %d full tiles + %d; %s form, %d walkers: %d with %d tiles, %d with %d;"
          " rows %d; walkers with an adding flush %d" % (s.name, case.name, case.B, case.n, case.T, cus, case.B // 32, case.B % 32,
                                                        s.form, len(tiles), sum(1 for c in tiles.values() if c == k), k,
                                                        sum(1 for c in tiles.values() if c == k + 1), k + 1,
                                                        M.rows(case.B, cus, s.form), adds))


@pytest.mark.parametrize("s,name", PARAMS)
def test_whole_batch_sums_at_the_walks_edges(engine, table, s, name):
    cus, cases = table
    case = cases[name]
    describe(s, case, cus)
    pol, cri = modules(engine, s)
    traj = ra.Trajectory(engine, case.n, case.T, s.in_dim)
    try:
        with Profiled(engine, "%s@%s" % (s.name, name)):
            pp, cp = pol.get_params(), cri.get_params()
            m = case.B if case.B <= DISTINCT_LIMIT else BASE
            rng = np.random.default_rng([0, case.B])
            x = rng.standard_normal((m, s.in_dim)).astype(np.float32)
            a = rng.integers(0, 2, size=m).astype(np.uint8)
            adv = rng.standard_normal(m).astype(np.float32)
            rtg = (10.0 * rng.standard_normal(m)).astype(np.float32)
            moved = off_the_relu_edges(s, [(pp, 2), (cp, 1)], x, lambda k: rng.standard_normal((k, s.in_dim)).astype(np.float32))
            print("%s@%s: %d of %d distinct samples redrawn off the relu edges" % (s.name, name, len(moved), m))
            assert len(moved) <= MAX_REDRAWN * m
            planes, wgt = planes_of(s, case, x, a, adv, rtg)
            TW.write(traj, planes)
            v = np.random.default_rng(7).standard_normal(pol.P).astype(np.float32)
            p_new = (pp + np.float32(0.01) * v).astype(np.float32)
            want = reference(s, pp, cp, v, p_new, x, a, adv, rtg, wgt)
            run_passes(Checker("%s@%s" % (s.name, name), samples=case.B), s, pol, cri, traj, want, v, p_new, ppo=True)
    finally:
        traj.close()
        pol.close()
        cri.close()


def dyadic_modules(engine, s):
    """every hidden bias -1, every weight after the first layer on the 2^-10 grid; output biases: the critic's 0.25 and
    the policy's as initialised, or all 0 under a Tanh output"""
    pol, cri = modules(engine, s)
    dead_value = np.float32(0.25 if s.out_act == "Identity" else 0.0)
    for mod, out_dim in ((pol, 2), (cri, 1)):
        p, k = mod.get_params(), 0
        for l, (fi, fo) in enumerate(G.layers(s.in_dim, s.hidden, out_dim)):
            W, b = slice(k, k + fi * fo), slice(k + fi * fo, k + fi * fo + fo)
            k += fi * fo + fo
            if l > 0:
                p[W] = np.round(p[W] * 1024.0) / 1024.0
                assert np.abs(p[W]).max() > 0.05
            if l < len(s.hidden):
                p[b] = -1.0
            elif s.out_act != "Identity":
                p[b] = 0.0
            elif mod is cri:
                p[b] = dead_value
        mod.set_params(p)
    return pol, cri, dead_value


def weight_slices(s, out_dim):
    out, k = [], 0
    for fi, fo in G.layers(s.in_dim, s.hidden, out_dim):
        out.append((slice(k, k + fi * fo), slice(k + fi * fo, k + fi * fo + fo)))
        k += fi * fo + fo
    return out


def assert_dead_batch_is_silent(s, pol, cri, traj, v, p_new, h_dead, ppo):
    """a dead sample adds exactly nothing to any sum but the entropy"""
    pp = pol.get_params()
    g, loss, ent = ra.policy_gradient(pol, traj)
    assert not g.any() and loss == 0.0, ("policy gradient", np.abs(g).max(), loss)
    assert abs(ent - h_dead) < 1e-6, (ent, h_dead)
    if ppo:
        step = sgd_ppo_step(pol, traj)
        assert not step.any(), ("ppo step", np.abs(step).max())
    if s.fvp:
        hv = ra.policy_fvp(pol, traj, v, 0.0)
        assert not hv.any(), ("fisher-vector product", np.abs(hv).max())
    loss, kl = moved_loss_kl(pol, traj, p_new)
    assert loss == 0.0 and kl == 0.0, ("moved loss / kl", loss, kl)
    g, loss = ra.critic_gradient(cri, traj)
    assert not g.any() and loss == 0.0, ("critic gradient", np.abs(g).max(), loss)
    assert np.array_equal(pol.get_params(), pp)


@pytest.mark.parametrize("s,name", PARAMS)
def test_one_live_tile_on_a_dead_batch(engine, table, s, name):
    cus, cases = table
    case = cases[name]
    B, n, T = case.B, case.n, case.T
    describe(s, case, cus)
    pol, cri, dead_value = dyadic_modules(engine, s)
    traj = ra.Trajectory(engine, n, T, s.in_dim)
    try:
        with Profiled(engine, "%s@%s" % (s.name, name)):
            pp, cp = pol.get_params(), cri.get_params()
            slices = weight_slices(s, 2)
            v = np.random.default_rng(7).standard_normal(pol.P).astype(np.float32)
            v[slices[-1][1]] = 0.5  # equal output-bias entries: the tangent outputs of a dead sample do not differ
            p_new = pp.copy()
            W0 = slices[0][0]
            p_new[W0] += np.float32(0.01) * v[W0]
            for W, _ in slices[1:]:  # weights only, and on the grid again
                p_new[W] = np.round((pp[W] + np.float32(0.01) * v[W]) * 1024.0) / 1024.0
                assert np.mean(p_new[W] != pp[W]) > 0.8
            z = pp[slices[-1][1]].astype(np.float64)
            lp = z - z.max() - np.log(np.exp(z - z.max()).sum())
            h_dead = float(-(np.exp(lp) * lp).sum())
            ppo = M.below_second_round(case, cus)
            planes = dict(obs=np.zeros((s.in_dim, T + 1, n), dtype=np.float32), action=np.zeros((T, n), dtype=np.uint8),
                          adv=np.zeros((T, n), dtype=np.float32), rtg=np.full((T, n), dead_value, dtype=np.float32))
            TW.write(traj, planes)
            assert_dead_batch_is_silent(s, pol, cri, traj, v, p_new, h_dead, ppo)
            # views of the planes in the flat sample order b = t n + lane
            obs_flat = planes["obs"].reshape(s.in_dim, (T + 1) * n)
            act_flat, adv_flat, rtg_flat = (planes[k].reshape(-1) for k in ("action", "adv", "rtg"))
            probes = M.probe_tiles(case, cus, s.form)
            for g in probes:
                lo, hi = 32 * g, min(32 * g + 32, B)
                m = hi - lo
                assert m == (32 if g < B // 32 else B % 32)
                rng = np.random.default_rng([g, B])
                draw = lambda k: (3.0 * rng.standard_normal((k, s.in_dim))).astype(np.float32)  # noqa: E731
                x = draw(m)
                off_the_relu_edges(s, [(pp, 2), (cp, 1), (p_new, 2)], x, draw, reach_the_output=True)
                a = rng.integers(0, 2, size=m).astype(np.uint8)
                adv = rng.standard_normal(m).astype(np.float32)
                rtg = (10.0 * rng.standard_normal(m)).astype(np.float32)
                obs_flat[:, lo:hi], act_flat[lo:hi], adv_flat[lo:hi], rtg_flat[lo:hi] = x.T, a, adv, rtg
                TW.write(traj, planes)
                chk = Checker("%s@%s tile %d (%d live of %d)" % (s.name, name, g, m, B), scale=m / B, samples=m)
                want = reference(s, pp, cp, v, p_new, x, a, adv, rtg)
                run_passes(chk, s, pol, cri, traj, want, v, p_new, ppo, ent_extra=(B - m) / B * h_dead)
                obs_flat[:, lo:hi], act_flat[lo:hi], adv_flat[lo:hi], rtg_flat[lo:hi] = 0.0, 0, 0.0, dead_value
            print("%s@%s: probed tiles %s" % (s.name, name, probes))
    finally:
        traj.close()
        pol.close()
        cri.close()
