"""The case table and the f64 reference of the clipped PPO gradient at ratios off 1 (tests/test_gpu_ppo_clip.py on the
device, tests/test_ppo_clip_cases_cpu.py for the table and the reference themselves).

rl_ppo_update takes the gradient of -mean(min(r A, clamp(r, 1 - d, 1 + d) A)) against the stored log pi_0
(policies/ppo.rs:124-137).  Which samples still pass a gradient is written out four times in the device code, and a row's
STATEMENT names the one its kernels run, per kernel variant:
  "fused"  kernels_mfma.hip, the fused 5-128 kernel (ratio by fast_expf)
  "gen"    kernels_gen_mfma.hip gm_sample_terms, both general matrix-pipe kernels (ratio by fast_expf)
  "terms"  policy_terms.hpp: k_policy_pass of kernel variant 1 and of every 4-input module, and the per-layer path of
           kernels_general.hip (2 to 8 actions)
  "seq"    kernels_seq_bwd.hip k_seq_policy_dlogits, every recurrent chain

The method (tests/test_gpu_ppo_clip.py): under plain SGD at rate lr from p0, one PPO step gives p1 and two give p2; both
steps of the second run share log pi_0 of p0, so (p1 - p2) / lr is the clipped gradient AT p1, where the first, large step
has moved the ratios both ways for both signs of the drawn advantages.

Nothing here imports the device library: the CPU test runs this module alone.
"""
import collections
import functools

import numpy as np

import chain_linear_ref as CL
from oracle import stacked as S

CLIPS = (0.2, 0.0, 4.0)  # PpoConfig::clip_distance: the default; lo = hi = 1; a negative lower bound that never clips
MARGIN = 1e-4            # no ratio this close to a bound: the gradient jumps there and f32 could land on the other side
REGIONS = ("inside", "A>0 r>hi (clipped)", "A>0 r<lo (live)", "A<0 r<lo (clipped)", "A<0 r>hi (live)")
MUTANTS = ("no mask", "max for min", "bounds exchanged for A<0")

# kind "mlp": spec = (in_dim, hidden, actions, activation) — hidden an int: rl_mlp_create's module; a list: the general one
# kind "rnn": spec = (cell, in_dim, hidden, num_layers, mlp_hidden, actions), the MLP-tail chains
# kind "lin": spec = (cell, in_dim, hidden, num_layers, actions), the Linear-tail chains
# statement: kernel variant -> the statement that variant's kernels run (the variants a row is run at)
# bar: whose bar for rl_policy_gradient the row inherits (tests/test_gpu_ppo_clip.py says where each number is from)
Row = collections.namedtuple("Row", "name kind spec n T lr seed gain statement bar")

# Lane counts are ones the path's own tests run (64 x 12 tile walks, narrow_cases' 50 x 13, 70 x 9 and 96 x 9 of the
# general and recurrent gradient tests, 32-lane multiples for the default GruMlp / LstmMlp kernels); B = n T in [256, 1024].
# gain scales p0 beyond its fan-in bound: at gain 1 the narrow and the recurrent modules' logits hardly depend on the
# observations, the first step moves the output biases alone, and every ratio of an action leaves the bounds together.
# lr and seed were searched with the reference alone — lr upwards through (0.1, 0.2, 0.5, 1, 2, 3, 5, 7, 10, 14, 20, 30),
# seeds 1 to 6 at each — until the conditions of tests/test_ppo_clip_cases_cpu.py held with twice the margin (the device's
# p1 is the reference's only to f32 rounding), no ratio exceeded the wide clip's upper bound 5, and 5 % of the ratios lay
# within 0.1 of 1.
# A Relu module of one hidden layer of at most 128 units over 4 or 5 inputs is rl_mlp_create's, never the general one
# (mlp_shape, handle_spec.hpp): the general single-layer rows have six inputs.  In launch_gen_mfma every module of widths
# <= 64 takes k_gen_pair in a gradient mode (gw = 2, and gp_lds_bytes fits at one to three layers); one hidden layer of
# 65..128 units (gw = 4) takes the one-wave k_gen_mfma: 6-[100].
ROWS = [
    Row("5-128", "mlp", (5, 128, 2, "Relu"), 64, 12, 2.0, 5, 1.0, {0: "fused", 1: "terms"}, "single"),
    Row("4-128", "mlp", (4, 128, 2, "Relu"), 50, 13, 1.0, 2, 1.0, {0: "terms", 1: "terms"}, "single"),
    Row("5-[8,8]", "mlp", (5, [8, 8], 2, "Relu"), 70, 9, 1.0, 2, 2.0, {0: "gen", 1: "terms"}, "general"),
    Row("5-[24,24]", "mlp", (5, [24, 24], 2, "Relu"), 64, 12, 3.0, 4, 2.0, {0: "gen", 1: "terms"}, "general"),
    Row("6-[33]", "mlp", (6, [33], 2, "Relu"), 70, 9, 7.0, 1, 1.0, {0: "gen", 1: "terms"}, "general"),
    Row("3-[16,16,16]-tanh", "mlp", (3, [16, 16, 16], 2, "Tanh"), 70, 9, 14.0, 1, 1.0, {0: "gen", 1: "terms"}, "general"),
    Row("6-[100]", "mlp", (6, [100], 2, "Relu"), 64, 10, 5.0, 1, 1.0, {0: "gen", 1: "terms"}, "general"),
    Row("5-[130]", "mlp", (5, [130], 2, "Relu"), 64, 10, 1.0, 1, 1.0, {0: "terms"}, "general"),
    Row("7-[32]-3", "mlp", (7, [32], 3, "Relu"), 64, 10, 3.0, 1, 1.0, {0: "terms"}, "multi"),
    Row("8-[16,16]-5", "mlp", (8, [16, 16], 5, "Tanh"), 64, 10, 7.0, 3, 1.0, {0: "terms"}, "multi"),
    Row("7-[32]-8", "mlp", (7, [32], 8, "Relu"), 64, 10, 5.0, 3, 1.0, {0: "terms"}, "multi"),
    Row("gru-5-128-128", "rnn", ("gru", 5, 128, 1, 128, 2), 32, 9, 2.0, 1, 3.0, {0: "seq"}, "recurrent"),
    Row("lstm-5-128-128", "rnn", ("lstm", 5, 128, 1, 128, 2), 32, 9, 5.0, 1, 3.0, {0: "seq"}, "recurrent"),
    Row("lstm-5-64x2-33", "rnn", ("lstm", 5, 64, 2, 33, 2), 70, 9, 10.0, 5, 3.0, {0: "seq"}, "recurrent"),
    Row("gru-7-12-8", "rnn", ("gru", 7, 12, 1, 8, 2), 70, 9, 2.0, 3, 3.0, {0: "seq"}, "recurrent"),
    Row("gru-6-7-linear", "lin", ("gru", 6, 7, 1, 2), 70, 9, 5.0, 5, 3.0, {0: "seq"}, "recurrent"),
    Row("lstm-5-70-linear", "lin", ("lstm", 5, 70, 1, 2), 70, 9, 3.0, 6, 8.0, {0: "seq"}, "recurrent"),
]
BY_NAME = {r.name: r for r in ROWS}
CASES = [(r.name, v) for r in ROWS for v in sorted(r.statement)]  # (row, kernel variant)


def case_id(case):
    return "%s-v%d" % case


def clip_bounds(d):
    """the f32 bounds rl_ppo_update computes, (float)(1.0 - d) and (float)(1.0 + d), as f64 numbers"""
    return float(np.float32(1.0 - d)), float(np.float32(1.0 + d))


def actions_of(row):
    return row.spec[2] if row.kind == "mlp" else row.spec[-1]


def in_dim_of(row):
    return row.spec[0] if row.kind == "mlp" else row.spec[1]


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def history(name):
    """a synthetic trajectory in the lane layouts (as tests/test_gpu_stacked.py's synthetic_history): random observations,
    flags with Terminate and Interrupt, actions over every index, and drawn advantages independent of the actions.
    Computed once per row; callers leave it unchanged."""
    row = BY_NAME[name]
    n, T, D, A = row.n, row.T, in_dim_of(row), actions_of(row)
    rng = np.random.default_rng(1000 + row.seed)
    h = {"obs": rng.normal(size=(D, T + 1, n)).astype(np.float32),
         "flag": rng.choice(np.array([0, 0, 0, 0, 1, 2], dtype=np.uint8), size=(T, n)),
         "term_obs": rng.normal(size=(D, T, n)).astype(np.float32),
         "action": rng.integers(0, A, size=(T, n)).astype(np.uint8),
         "reward": rng.normal(size=(T, n)).astype(np.float32),
         "adv": rng.normal(size=(T, n)).astype(np.float32)}
    assert sorted(np.unique(h["action"])) == list(range(A)) and set(np.unique(h["flag"])) == {0, 1, 2}
    return h


def mlp_layers(row):
    D, hidden, A, _ = row.spec
    w = [D] + (list(hidden) if isinstance(hidden, (list, tuple)) else [hidden]) + [A]
    return list(zip(w[:-1], w[1:]))


def blocks(row):
    """[(name, slice)] of the module's flat parameter vector, in its own order"""
    out, o = [], 0
    if row.kind == "mlp":
        for i, (fi, fo) in enumerate(mlp_layers(row)):
            out += [("W%d" % i, slice(o, o + fi * fo)), ("b%d" % i, slice(o + fi * fo, o + fi * fo + fo))]
            o += fi * fo + fo
    elif row.kind == "rnn":
        for name, l, shp, off in spec_of(row).slices()[0]:
            out.append((name if l < 0 else "%s%d" % (name, l), slice(off, off + int(np.prod(shp)))))
    else:
        cell, D, H, NL, A = row.spec
        for name, l, shp, off, _ in CL.blocks(cell, D, H, NL, A, True):
            out.append((name if l < 0 else "%s%d" % (name, l), slice(off, off + int(np.prod(shp)))))
    return out


def spec_of(row):
    """the f64 restatement's spec of a recurrent row (a Linear tail: the embedded chain's, tests/chain_linear_ref.py)"""
    if row.kind == "rnn":
        cell, D, H, NL, H2, A = row.spec
        return S.Spec(S.GRU if cell == "gru" else S.LSTM, D, H, NL, H2, A)
    cell, D, H, NL, A = row.spec
    return CL.spec_of(cell, D, H, NL, A)


@functools.lru_cache(maxsize=None)
def initial_params(name):
    """p0 (f32): every block uniform within the row's gain times its fan-in bound, 1 / sqrt(width of the rows it
    multiplies)"""
    row = BY_NAME[name]
    rng = np.random.default_rng(2000 + row.seed)
    if row.kind == "mlp":
        parts = []
        for fi, fo in mlp_layers(row):
            parts.append(row.gain * rng.uniform(-1.0, 1.0, size=fi * fo + fo) / np.sqrt(fi))
        return np.concatenate(parts).astype(np.float32)
    H = row.spec[2]
    P = blocks(row)[-1][1].stop
    p = row.gain * rng.uniform(-1.0, 1.0, size=P) / np.sqrt(H)
    if row.kind == "rnn":
        H2 = row.spec[4]
        for name, s in blocks(row):
            if name in ("W2", "b2"):
                p[s] *= np.sqrt(H / H2)
    return p.astype(np.float32)


# ---------------------------------------------------------------- the rule, per sample
def log_softmax(z):
    """over axis 0"""
    z = z - z.max(axis=0)
    return z - np.log(np.exp(z).sum(axis=0))


def pass_weight(ratio, adv, lo, hi, mutant=None):
    """d min(r A, clamp(r, lo, hi) A) / d r as torch autograd gives it: minimum() splits a tie between its arguments,
    clamp() passes the gradient inside [lo, hi], bounds included.  `mutant`: one of MUTANTS, a deliberately wrong rule."""
    u1, u2 = ratio * adv, np.clip(ratio, lo, hi) * adv
    inside = (ratio >= lo) & (ratio <= hi)
    through_clamp = np.where(inside, adv, 0.0)
    if mutant == "no mask":
        through_clamp = adv
    if mutant == "bounds exchanged for A<0":  # which side is clipped follows the bound alone, not the advantage's sign
        return np.where(ratio > hi, 0.0, adv)
    first = u1 > u2 if mutant == "max for min" else u1 < u2
    return np.where(first, adv, np.where(u1 == u2, 0.5 * adv + 0.5 * through_clamp, through_clamp))


def dloss_dlogits(logits, lp0a, action, adv, lo, hi, mutant=None):
    """d loss / d logits of loss = -mean(min(r A, clamp(r, lo, hi) A)), r = exp(log pi(a) - lp0a), written out.
    logits [A][...]; lp0a, action, adv [...].  -> (d loss / d logits, loss, ratio)"""
    logits = np.asarray(logits, dtype=np.float64)
    adv = np.asarray(adv, dtype=np.float64)
    a = np.asarray(action).astype(np.int64)
    lp = log_softmax(logits)
    lpa = np.take_along_axis(lp, a[None], axis=0)[0]
    ratio = np.exp(lpa - lp0a)
    B = adv.size
    c = -(pass_weight(ratio, adv, lo, hi, mutant) * ratio) / B
    ind = (np.arange(logits.shape[0]).reshape((-1,) + (1,) * a.ndim) == a[None]).astype(np.float64)
    u1, u2 = ratio * adv, np.clip(ratio, lo, hi) * adv
    pick = np.maximum if mutant == "max for min" else np.minimum
    return c[None] * (ind - np.exp(lp)), -pick(u1, u2).mean(), ratio


def census(ratio, adv, lo, hi):
    """sample counts of the five regions, in REGIONS' order"""
    ratio, adv = np.asarray(ratio).reshape(-1), np.asarray(adv, dtype=np.float64).reshape(-1)
    inside = (ratio >= lo) & (ratio <= hi)
    return (int(inside.sum()), int(((adv > 0) & (ratio > hi)).sum()), int(((adv > 0) & (ratio < lo)).sum()),
            int(((adv < 0) & (ratio < lo)).sum()), int(((adv < 0) & (ratio > hi)).sum()))


def margin(ratio, lo, hi):
    """the smallest distance of a ratio from a bound"""
    ratio = np.asarray(ratio).reshape(-1)
    return float(min(np.abs(ratio - lo).min(), np.abs(ratio - hi).min()))


# ---------------------------------------------------------------- the networks in f64
def flat_samples(row):
    """feed-forward modules see the steps as samples: x [B][D], action [B], adv [B], sample b = t n + lane"""
    h = history(row.name)
    D = in_dim_of(row)
    return (h["obs"][:, :row.T, :].reshape(D, -1).T.astype(np.float64), h["action"].reshape(-1).astype(np.int64),
            h["adv"].reshape(-1).astype(np.float64))


def _mlp_logits_torch(row, p, x):
    import torch
    act = {"Relu": torch.relu, "Tanh": torch.tanh}[row.spec[3]]
    h, k, layers = x, 0, mlp_layers(row)
    for i, (fi, fo) in enumerate(layers):
        W, b = p[k:k + fi * fo].reshape(fo, fi), p[k + fi * fo:k + fi * fo + fo]
        k += fi * fo + fo
        h = h @ W.T + b
        if i + 1 < len(layers):
            h = act(h)
    return h  # [B][A]


def logits64(row, params):
    """the module's logits at `params`, [A][T][n] (feed-forward: [A][B])"""
    if row.kind == "mlp":
        import torch
        x, _, _ = flat_samples(row)
        with torch.no_grad():
            return _mlp_logits_torch(row, torch.tensor(np.asarray(params, dtype=np.float64)), torch.tensor(x)).numpy().T.copy()
    return S.forward(spec_of(row), full_params(row, params), history(row.name), want_succ=False)[0]


def full_params(row, params):
    params = np.asarray(params, dtype=np.float64)
    if row.kind == "lin":
        cell, D, H, NL, A = row.spec
        return CL.embed(cell, D, H, NL, A, True, params)
    return params


def vjp(row, params, dz):
    """sum over samples and actions of dz * d logits / d params (flat, f64, the module's own layout)"""
    if row.kind == "mlp":
        import torch
        x, _, _ = flat_samples(row)
        p = torch.tensor(np.asarray(params, dtype=np.float64), requires_grad=True)
        z = _mlp_logits_torch(row, p, torch.tensor(x))
        return torch.autograd.grad((z * torch.tensor(np.ascontiguousarray(dz.T))).sum(), p)[0].numpy().copy()
    g = S.backward(spec_of(row), full_params(row, params), history(row.name), dz)
    if row.kind == "lin":
        cell, D, H, NL, A = row.spec
        return CL.restrict(cell, D, H, NL, A, True, g)
    return g


def logp0_of(row, p0):
    """log pi_0 of the taken actions at p0"""
    h = history(row.name)
    a = (h["action"].reshape(-1) if row.kind == "mlp" else h["action"]).astype(np.int64)
    return np.take_along_axis(log_softmax(logits64(row, p0)), a[None], axis=0)[0]


def reference(row, p0, p1, clip, mutant=None):
    """The clipped surrogate's loss and gradient at p1 against log pi_0 of p0, in f64.  Feed-forward rows without a
    mutant: torch autograd of the loss as written (what tests/test_gpu_multi_action.py's torch_restatement(..., clip=)
    states, for any number of actions); recurrent rows and every mutant: d loss / d logits written out in NumPy
    (dloss_dlogits) through the network's transposed Jacobian.  -> dict(grad, loss, ratio, adv, census, margin)"""
    lo, hi = clip_bounds(clip)
    h = history(row.name)
    if row.kind == "mlp":
        x, a, adv = flat_samples(row)
    else:
        a, adv = h["action"].astype(np.int64), h["adv"].astype(np.float64)
    lp0a = logp0_of(row, p0)
    if row.kind == "mlp" and mutant is None:
        import torch
        p = torch.tensor(np.asarray(p1, dtype=np.float64), requires_grad=True)
        lp = torch.log_softmax(_mlp_logits_torch(row, p, torch.tensor(x)), dim=1)
        ratio = torch.exp(lp.gather(1, torch.tensor(a)[:, None])[:, 0] - torch.tensor(lp0a))
        advt = torch.tensor(adv)
        loss = -torch.minimum(ratio * advt, torch.clamp(ratio, lo, hi) * advt).mean()
        grad = torch.autograd.grad(loss, p)[0].numpy().copy()
        loss, ratio = loss.item(), ratio.detach().numpy().copy()
    else:
        dz, loss, ratio = dloss_dlogits(logits64(row, p1), lp0a, a, adv, lo, hi, mutant)
        grad = vjp(row, p1, dz)
    return dict(grad=grad, loss=float(loss), ratio=ratio, adv=adv, census=census(ratio, adv, lo, hi),
                margin=margin(ratio, lo, hi))


def unclipped_gradient(row, p):
    """the gradient at ratio 1, of -mean(r A) against log pi_0 of p itself: what the first PPO step applies"""
    return reference(row, p, p, 4.0)["grad"]


@functools.lru_cache(maxsize=None)
def reference_first_step(name):
    """the reference's own p1 (f32): one SGD step at the row's rate from p0"""
    row = BY_NAME[name]
    p0 = initial_params(name)
    return (p0.astype(np.float64) - row.lr * unclipped_gradient(row, p0)).astype(np.float32)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@functools.lru_cache(maxsize=None)
def reference_at_own_step(name, clip, mutant=None):
    """reference() at the reference's own p1 (computed once; callers leave it unchanged)"""
    return reference(BY_NAME[name], initial_params(name), reference_first_step(name), clip, mutant)


def f32_oracle_distance(row, p1):
    """e32 of tests/narrow_cases.py's bar for the single-hidden-layer kernels: the f32 oracle's own distance from the f64
    oracle for rl_policy_gradient's vector — the surrogate gradient at ratio 1 — on the row's samples at p1"""
    import narrow_cases as nc
    import oracle as O
    D, H, A, _ = row.spec
    ps = O.MlpShape(D, H, A)
    x, a, adv = flat_samples(row)
    x, a, adv = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(a), np.ascontiguousarray(adv, dtype=np.float32)
    p1 = np.ascontiguousarray(p1, dtype=np.float32)
    return rel_err(nc.policy_grad32(ps, p1, x, a, adv)[0], nc.policy_grad64(ps, p1, x, a, adv)[0])
