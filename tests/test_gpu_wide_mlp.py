"""Feed-forward modules of 9 to 24 inputs (rl_mlp_create_wide / ra.MlpWide) on host-written ra.TrajectoryWide24
trajectories: the fused matrix-pipe passes of relearn_amd/csrc/kernels_wide_mfma.hip (kernel variant 0) and the per-layer f32
kernels (variant 1), each against torch float64 autograd on the CPU, written out below.

Bars, relative to max |g| for vectors, from the tests that hold the same quantities on the general and recurrent paths:
  tests/test_gpu_multi_action.py   gradient (and the clipped PPO gradient, tests/test_gpu_ppo_clip.py "multi") 2e-5 + 1e-9,
                                   Fisher-vector product 5e-5, loss and entropy 2e-5 + 1e-7, KL 2e-4 + 1e-8, TRPO
                                   parameters at 2 CG iterations 2e-3 of the step + 1e-7
  tests/test_gpu_partition.py      critic gradient GRAD_RTOL = 5e-6, critic loss 1e-5
Logits (no existing test holds an f32 forward to f64): the bound of an f32 fma chain, worked out per case by logit_bound.
Every test here fails on a library without rl_mlp_create_wide."""
import functools

import numpy as np
import pytest
import torch

import relearn_amd as ra

pytestmark = pytest.mark.gpu

# (in_dim, hidden, activation, bias, n, T): each axis's edge values against the base case, and two corners
BASE = (24, [64], "Relu", True, 33, 3)
# (the fused kernel takes one hidden layer of at most 64 units with bias vectors: [8], [33] — a second tile with one live
# unit — and [64]; [33, 64], [128] and the bias-less module run the per-layer kernels under both variants)
CASES = [BASE] + [(d,) + BASE[1:] for d in (9, 16, 17, 23)] + [BASE[:1] + (h,) + BASE[2:] for h in ([8], [33], [33, 64], [128])] + [
    (24, [64], "Tanh", True, 33, 3), (24, [64], "Relu", False, 33, 3), (24, [64], "Relu", True, 64, 5),
    (17, [33], "Tanh", True, 64, 5), (17, [33, 64], "Tanh", True, 64, 5), (24, [128], "Tanh", True, 64, 5)]
FUSED = [i for i, c in enumerate(CASES) if len(c[1]) == 1 and c[1][0] <= 64 and c[3]]
IDS = ["%d-%s-%s-%s-%dx%d" % (c[0], "x".join(map(str, c[1])), c[2], "bias" if c[3] else "nobias", c[4], c[5]) for c in CASES]
LR, CLIP = 0.05, 0.2


def forward64(p, dims, act, bias, x):
    fn = {"Relu": torch.relu, "Tanh": torch.tanh}[act]
    h, k = x, 0
    for i, (fi, fo) in enumerate(zip(dims[:-1], dims[1:])):
        h = h @ p[k:k + fi * fo].reshape(fo, fi).T
        k += fi * fo
        if bias:
            h = h + p[k:k + fo]
            k += fo
        if i + 2 < len(dims):
            h = fn(h)
    return h


def logit_bound(c, p, x):
    """per-sample bound on |f32 forward - f64 forward|: a dot product of K terms from the bias by fma in f32 is within
    (K + 1) u of sum |w||a| + |b| (u = 2^-24); Relu and Tanh are 1-Lipschitz, so a layer passes the error below it through
    |W|, and the engine's tanh adds 2.5 ulp of a value below 1"""
    D, hidden, act, bias = c[:4]
    u, dims, k = 2.0 ** -24, [D] + hidden + [2], 0
    mag, err = np.abs(np.asarray(x, np.float64)), np.zeros((len(x), D))
    for i, (fi, fo) in enumerate(zip(dims[:-1], dims[1:])):
        W = np.abs(p[k:k + fi * fo].astype(np.float64)).reshape(fo, fi)
        k += fi * fo
        b = np.abs(p[k:k + fo].astype(np.float64)) if bias else 0.0
        k += fo if bias else 0
        mag, err = mag @ W.T + b, err @ W.T
        err = err + (fi + 1) * u * mag + (2.5 * u if act == "Tanh" and i + 2 < len(dims) else 0.0)
    return err.max()


def policy64(c, p, p0, x, a, adv, vec=None, clip=None):
    """Trpo::update's closure, HessianVectorProduct and Ppo::update's clipped surrogate in f64 autograd"""
    D, hidden, act, bias = c[:4]
    t64 = lambda v: torch.tensor(np.asarray(v, dtype=np.float64))
    p = t64(p).requires_grad_(True)
    z = forward64(p, [D] + hidden + [2], act, bias, t64(x))
    lp = torch.log_softmax(z, dim=1)
    lp0 = torch.log_softmax(forward64(t64(p0), [D] + hidden + [2], act, bias, t64(x)), dim=1)
    at = torch.tensor(a.astype(np.int64))[:, None]
    ratio = torch.exp(lp.gather(1, at)[:, 0] - lp0.gather(1, at)[:, 0])
    u = ratio * t64(adv)
    loss = -(u if clip is None else torch.minimum(u, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * t64(adv))).mean()
    kl = (lp0.exp() * (lp0 - lp)).sum(dim=1).mean()
    out = {"z": z.detach().numpy(), "loss": loss.item(), "kl": kl.item(), "entropy": -(lp.exp() * lp).sum(dim=1).mean().item(),
           "grad": torch.autograd.grad(loss, p, retain_graph=True)[0].numpy()}
    if vec is not None:
        gk = torch.autograd.grad(kl, p, create_graph=True)[0]
        out["fvp"] = torch.autograd.grad((gk * t64(vec)).sum(), p)[0].numpy()
    return out


def critic64(c, p, x, target):
    D, hidden, act, bias = c[:4]
    p = torch.tensor(p.astype(np.float64), requires_grad=True)
    v = forward64(p, [D] + hidden + [1], act, bias, torch.tensor(x.astype(np.float64)))[:, 0]
    loss = ((v - torch.tensor(target.astype(np.float64))) ** 2).mean()
    return loss.item(), torch.autograd.grad(loss, p)[0].numpy()


def history(c):
    """0/1 features and one smooth f32 feature, uniform actions, standard-normal advantages and returns"""
    D, n, T = c[0], c[4], c[5]
    rs = np.random.default_rng(100 + D + n)
    obs = rs.integers(0, 2, (D, T + 1, n)).astype(np.float32)
    obs[D // 2] = rs.random((T + 1, n), dtype=np.float32)
    return {"obs": obs, "term_obs": np.zeros((D, T, n), np.float32), "flag": np.zeros((T, n), np.uint8),
            "reward": np.zeros((T, n), np.float32), "action": rs.integers(0, 2, (T, n)).astype(np.uint8),
            "adv": rs.normal(size=(T, n)).astype(np.float32), "rtg": rs.normal(size=(T, n)).astype(np.float32)}


def setup(engine, c):
    D, hidden, act, bias, n, T = c
    pol, cri = ra.MlpWide(engine, D, hidden, 2, act, bias=bias), ra.MlpWide(engine, D, hidden, 1, act, bias=bias)
    pol.init(11), cri.init(12)
    h = history(c)
    traj = ra.TrajectoryWide24(engine, n, T, D)
    traj.write_all(h)
    traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
    traj.write(ra.TRAJ_RETURNS, h["rtg"])
    x = h["obs"][:, :T].reshape(D, T * n).T
    return pol, cri, traj, x, h["action"].reshape(-1), h["adv"].reshape(-1), h["rtg"].reshape(-1)


@functools.lru_cache(maxsize=None)
def reference(i, p0, c0):
    """the f64 side of case i at the modules' initial parameters (the same under both kernel variants): computed once"""
    c = CASES[i]
    h = history(c)
    D, T, n = c[0], c[5], c[4]
    x, a, adv, rtg = h["obs"][:, :T].reshape(D, T * n).T, h["action"].reshape(-1), h["adv"].reshape(-1), h["rtg"].reshape(-1)
    p0, c0 = np.frombuffer(p0, np.float32), np.frombuffer(c0, np.float32)
    vec = np.random.default_rng(5).normal(size=p0.size).astype(np.float32)
    moved = (p0 + 0.01 * vec).astype(np.float32)
    return dict(vec=vec, moved=moved, zbound=logit_bound(c, p0, x), at0=policy64(c, p0, p0, x, a, adv, vec), at1=policy64(c, moved, p0, x, a, adv),
                critic=critic64(c, c0, x, rtg), x=x, a=a, adv=adv)


def close(what, got, want, rel, floor):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, bound = np.abs(got - want).max(), rel * np.abs(want).max() + floor
    print("%s: max error %.3e, bound %.3e" % (what, err, bound))
    return err <= bound


def sgd_ppo(engine, pol, traj, p0, steps):
    cfg = ra.optimizer_config_default(ra.OPTIMIZER_SGD)
    cfg.learning_rate = LR
    step = ra.ppo_config_default()
    step.opt_steps_per_update, step.clip_distance = steps, CLIP
    pol.set_params(p0)
    ra.ppo_update(pol, ra.Optimizer(pol, cfg), traj, step)
    return pol.get_params().astype(np.float64)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_passes_against_f64(engine, i, variant):
    c = CASES[i]
    engine.set_kernel_variant(variant)
    try:
        pol, cri, traj, x, a, adv, rtg = setup(engine, c)
        p0 = pol.get_params()
        ref = reference(i, p0.tobytes(), cri.get_params().tobytes())
        r0, r1 = ref["at0"], ref["at1"]
        assert close("logits", pol.forward(x), r0["z"], 0.0, ref["zbound"])
        g, loss, ent = ra.policy_gradient(pol, traj)
        assert close("gradient", g, r0["grad"], 2e-5, 1e-9)
        assert abs(loss - r0["loss"]) <= 2e-5 * abs(r0["loss"]) + 1e-7 and abs(ent - r0["entropy"]) <= 2e-5 * r0["entropy"] + 1e-7
        assert close("fvp", ra.policy_fvp(pol, traj, ref["vec"], 0.0), r0["fvp"], 5e-5, 0.0)
        assert close("fvp + damping", ra.policy_fvp(pol, traj, ref["vec"], 1e-5), r0["fvp"] + 1e-5 * ref["vec"].astype(np.float64), 5e-5, 0.0)
        pol.set_params(ref["moved"])
        loss1, kl1 = ra.policy_loss_kl(pol, traj, p0)
        assert abs(loss1 - r1["loss"]) <= 2e-5 * abs(r1["loss"]) + 1e-7 and abs(kl1 - r1["kl"]) <= 2e-4 * r1["kl"] + 1e-8
        # the clipped PPO gradient at the ratios one large SGD step leaves (tests/test_gpu_ppo_clip.py): (p1 - p2) / lr
        # against the reference at the device's p1; the readback costs 2^-24 (|p2| + lr |g|) / lr per entry
        p1, p2 = sgd_ppo(engine, pol, traj, p0, 1), sgd_ppo(engine, pol, traj, p0, 2)
        gp = policy64(c, p1.astype(np.float32), p0, ref["x"], ref["a"], ref["adv"], clip=CLIP)["grad"]
        diff = np.abs((p1 - p2) / LR - gp) - 2.0 ** -24 * (np.abs(p2) + LR * np.abs(gp)) / LR
        print("ppo gradient: max error beyond the readback %.3e, bound %.3e" % (diff.max(), 2e-5 * np.abs(gp).max() + 1e-9))
        assert diff.max() <= 2e-5 * np.abs(gp).max() + 1e-9
        closs, cgrad = ref["critic"]
        cg, cl = ra.critic_gradient(cri, traj)
        assert close("critic gradient", cg, cgrad, 5e-6, 0.0) and abs(cl - closs) <= 1e-5 * closs
    finally:
        engine.set_kernel_variant(0)


@pytest.mark.parametrize("i", FUSED[:1] + FUSED[5:7] + FUSED[-1:], ids=lambda i: IDS[i])
def test_update_steps_agree_between_the_variants(engine, i):
    """one TRPO step with 2 CG iterations and a critic update of 2 Adam steps: the fused path against the per-layer one"""
    got = []
    for variant in (0, 1):
        engine.set_kernel_variant(variant)
        try:
            pol, cri, traj = setup(engine, CASES[i])[:3]
            p0, c0 = pol.get_params(), cri.get_params()
            cfg = ra.trpo_config_default()
            cfg.iterations = 2
            st = ra.trpo_update(pol, traj, cfg)
            cst = ra.critic_update(cri, ra.Adam(cri), traj, 2)
            got.append((st, pol.get_params(), cst, cri.get_params()))
        finally:
            engine.set_kernel_variant(0)
    (s0, p_0, c_0, q_0), (s1, p_1, c_1, q_1) = got
    assert s0.status == s1.status == ra.OPT_OK and s0.num_backtracks == s1.num_backtracks
    assert s0.cg_iterations == s1.cg_iterations == 2
    assert np.abs(p_0 - p_1).max() <= 2e-3 * np.abs(p_1 - p0).max() + 1e-7
    assert abs(c_0.loss_first - c_1.loss_first) <= 1e-5 * c_1.loss_first and c_0.loss_last < c_0.loss_first
    assert np.abs(q_0 - q_1).max() <= 2e-3 * np.abs(q_1 - c0).max() + 1e-7


def test_refusals(engine):
    def code_of(fn):
        with pytest.raises(ra.RelearnError) as e:
            fn()
        return e.value.code, str(e.value)
    BUILD_AGENT, UNSUPPORTED, INVALID_ARGUMENT = 4, 10, 1
    assert code_of(lambda: ra.MlpWide(engine, 25, [16], 2))[0] == BUILD_AGENT
    code, text = code_of(lambda: ra.MlpWide(engine, 24, [16], 3))
    assert code == UNSUPPORTED and "rl_mlp_create_wide" in text
    assert code_of(lambda: ra.Mlp(engine, 24, [16], 2))[0] == BUILD_AGENT  # the older constructor keeps its bound
    pol = ra.MlpWide(engine, 24, [16], 2)
    code, text = code_of(lambda: ra.policy_gradient(pol, ra.TrajectoryWide24(engine, 32, 2, 23)))
    assert code == INVALID_ARGUMENT and "does not match the trajectory" in text
    env = ra.PartitionEnv(engine, 32, max_steps=3, limit=ra.LIMIT_VISIBLE, seed_env=1, seed_actor=2)
    code, text = code_of(lambda: ra.Dqn(env, pol, ra.Adam(pol), ra.dqn_config_default()))
    assert code == UNSUPPORTED and "rl_mlp_create_wide" in text


@pytest.mark.parametrize("D", [5, 8])
def test_inside_the_older_range_it_builds_the_older_module(engine, D):
    out = []
    for cls in (ra.Mlp, ra.MlpWide):
        m = cls(engine, D, [32], 2)
        m.init(3)
        c = (D, [32], "Relu", True, 33, 3)
        h = history(c)
        traj = ra.TrajectoryWide24(engine, 33, 3, D)
        traj.write_all(h)
        traj.write(ra.TRAJ_ADVANTAGES, h["adv"])
        out.append((m.P, m.get_params().tobytes(), ra.policy_gradient(m, traj)[0].tobytes()))
    assert out[0] == out[1]
