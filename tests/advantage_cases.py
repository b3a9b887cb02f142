"""The case table of the advantage / return / value-target paths (tests/test_gpu_advantage_paths.py on the device,
tests/test_advantage_cases_cpu.py for the table itself): host-made histories whose episode ends are PLACED at the steps
where the scans change behaviour, and plain NumPy restatements of the scans to hold them to.

The scans (k_gae_scan, k_seq_gae) walk each lane's time axis backwards in batches of 16 prefetched steps, loads clamped
at step 0, the last batch partial; the array-fed ones take the successor value of a cut episode from an array that
k_gen_successor_values (general critics) or the teacher-forced forward (recurrent critics) filled.  So the ends sit at
t = T-1 (each successor code), at t = 0, and either side of the batch boundary (T-16, T-17); the shapes give a partial
batch only, exactly one batch, a batch plus a step and two batches plus a step, with a patterned lane in a second and a
third 64-thread workgroup.

term_obs is poisoned: NaN wherever flag != INTERRUPT, so that a value read from the wrong place cannot pass a bit
comparison.  No call of the library refuses such a history (the fused kernels' range guard reads the observation planes,
never term_obs), so no finite sentinel is needed; `make_history(..., poison=x)` takes one all the same.

Nothing here imports the device library: the CPU test runs this module alone.
"""
import numpy as np

import oracle as O

GAMMA, LAMBDA = 0.97, 0.9  # rl_gae's in every case
TD_GAMMA = 0.93            # the One-step-TD update's, and the RewardToGo targets' "other" discount

SHAPES = [(1, 1), (3, 2), (65, 15), (63, 16), (65, 17), (130, 33)]  # (n, T)
PATTERNS = ["continue", "term_last", "intr_last", "term_first", "intr_first", "every_step", "intr_batch_edge",
            "term_batch_edge", "random"]
PATTERN_SETS = ["base", "no_interrupt", "only_last_sample", "only_first_sample"]
BATCH = 16  # steps the scans prefetch at a time (AHEAD in k_seq_gae, GAE_AHEAD in k_gae_scan)


def shape_id(shape):
    return "n%d-T%d" % shape


def pattern_of(lane, T):
    """the pattern lane `lane` carries at horizon T: one that needs more steps than T is all Continue"""
    p = PATTERNS[lane % len(PATTERNS)]
    return "continue" if p.endswith("batch_edge") and T < BATCH + 2 else p


def lane_flags(pattern, T, rng):
    f = np.zeros(T, dtype=np.uint8)
    kind = O.TERMINATE if pattern.startswith("term") else O.INTERRUPT
    if pattern in ("term_last", "intr_last"):
        f[T - 1] = kind
    elif pattern in ("term_first", "intr_first"):
        f[0] = kind
    elif pattern == "every_step":
        f[0::2], f[1::2] = O.TERMINATE, O.INTERRUPT
    elif pattern in ("term_batch_edge", "intr_batch_edge"):
        f[T - BATCH] = f[T - BATCH - 1] = kind
    elif pattern == "random":
        f[:] = rng.choice(np.array([0, 0, 0, 1, 2], dtype=np.uint8), size=T)
    else:
        assert pattern == "continue", pattern
    return f


def make_history(D, n, T, pattern_set="base", seed=0, poison=np.nan):
    """the dict Trajectory.write_all takes: obs [D][T+1][n], action, reward, flag [T][n], term_obs [D][T][n]"""
    assert pattern_set in PATTERN_SETS, pattern_set
    rng = np.random.default_rng([seed, D, n, T])
    flag = np.stack([lane_flags(pattern_of(i, T), T, rng) for i in range(n)], axis=1)
    if pattern_set != "base":
        flag[flag == O.INTERRUPT] = O.TERMINATE
    if pattern_set == "only_last_sample":
        flag[T - 1, n - 1] = O.INTERRUPT
    if pattern_set == "only_first_sample":
        flag[0, 0] = O.INTERRUPT
    term = rng.normal(size=(D, T, n)).astype(np.float32)
    term[:, flag != O.INTERRUPT] = poison
    return {"obs": rng.normal(size=(D, T + 1, n)).astype(np.float32),
            "action": rng.integers(0, 2, size=(T, n)).astype(np.uint8),
            "reward": rng.normal(size=(T, n)).astype(np.float32),
            "flag": np.ascontiguousarray(flag), "term_obs": term}


_hist = {}


def history(D, shape, pattern_set="base"):
    """make_history, once per case (shared and never written to)"""
    key = (D, shape, pattern_set)
    if key not in _hist:
        h = make_history(D, shape[0], shape[1], pattern_set, seed=11)
        for a in h.values():
            a.setflags(write=False)
        _hist[key] = h
    return _hist[key]


# ---------------------------------------------------------------- the scans, restated
def successors(hist, v_term, v_last):
    """k_gen_successor_values' rule: V(term_obs) after an Interrupt, V(obs[T]) for a lane the horizon cuts (Continue at
    T-1), 0 elsewhere.  v_term [T][n], v_last [n] -> [T][n]"""
    flag = hist["flag"]
    T = flag.shape[0]
    succ = np.zeros(flag.shape, dtype=np.float32)
    succ[flag == O.INTERRUPT] = np.asarray(v_term, dtype=np.float32)[flag == O.INTERRUPT]
    cut = flag[T - 1] == O.CONTINUE
    succ[T - 1, cut] = np.asarray(v_last, dtype=np.float32)[cut]
    return succ


def next_values(values, succ, hist):
    """(next value [T][n], ends [T][n]): 0 after Terminate, succ[t] after Interrupt or at t = T-1, values[t+1] otherwise"""
    flag = hist["flag"]
    T = flag.shape[0]
    values, succ = np.asarray(values)[:T], np.asarray(succ)
    last = np.zeros(flag.shape, dtype=bool)
    last[T - 1] = True
    shifted = np.concatenate([values[1:], np.zeros_like(values[:1])])
    vn = np.where(flag == O.TERMINATE, values.dtype.type(0), np.where((flag == O.INTERRUPT) | last, succ, shifted))
    return vn, (flag != O.CONTINUE) | last


def scan_f32(values, succ, hist, gamma, lam):
    """k_seq_gae / oracle_seq_gae / inplace_discounted_cumsum_from_end, every operation rounded to f32 in their order:
    dn = gamma*vn; tmp = r + dn; delta = tmp - v; a = delta + adv_next*(lam*gamma); g = r + rtg_next*gamma -> (adv, rtg)"""
    f = np.float32
    gamma, lam = f(gamma), f(lam)
    disc = f(lam * gamma)
    r = np.asarray(hist["reward"], dtype=f)
    T, n = r.shape
    values, succ = np.asarray(values, dtype=f)[:T], np.asarray(succ, dtype=f)
    vn, ends = next_values(values, succ, hist)
    adv, rtg = np.zeros((T, n), dtype=f), np.zeros((T, n), dtype=f)
    adv_next, rtg_next = np.zeros(n, dtype=f), np.zeros(n, dtype=f)
    with np.errstate(invalid="ignore"):
        for t in range(T - 1, -1, -1):
            dn = f(gamma) * vn[t]
            tmp = r[t] + dn
            delta = tmp - values[t]
            pa = adv_next * disc
            pg = rtg_next * gamma
            adv[t] = np.where(ends[t], delta, delta + pa)
            rtg[t] = np.where(ends[t], r[t], r[t] + pg)
            adv_next, rtg_next = adv[t], rtg[t]
    assert adv.dtype == f and rtg.dtype == f
    return adv, rtg


def td_f32(values, succ, hist, gamma):
    """k_seq_value_targets_td / oracle_seq_one_step_targets: dn = gamma*vn; target = r + dn, two f32 roundings"""
    f = np.float32
    r = np.asarray(hist["reward"], dtype=f)
    vn, _ = next_values(np.asarray(values, dtype=f), np.asarray(succ, dtype=f), hist)
    dn = f(gamma) * vn
    out = r + dn
    assert out.dtype == f
    return out


def scan_f64(values, succ, hist, gamma, lam):
    """The definition, in f64 and as explicit sums (no recursion): within the episode segment that ends at step e,
    adv_t = sum_k (gamma*lam)^k delta_{t+k} and rtg_t = sum_k gamma^k r_{t+k}, k = 0..e-t, with
    delta_t = r_t + gamma*next_t - V_t.  gamma and lam are the f32 numbers the device gets, their product exact.
    -> (adv, rtg, steps, S_adv, S_rtg): steps[t] = e - t, and S the sum of the absolute values of the terms of that
    sample's sum — for the advantage the three terms of every delta, each weighted with its power"""
    gamma, lam = float(np.float32(gamma)), float(np.float32(lam))
    r = np.asarray(hist["reward"], dtype=np.float64)
    T, n = r.shape
    vn, ends = next_values(np.asarray(values, dtype=np.float64)[:T], np.asarray(succ, dtype=np.float64), hist)
    v = np.asarray(values, dtype=np.float64)[:T]
    delta = r + gamma * vn - v
    mag = np.abs(r) + np.abs(gamma * vn) + np.abs(v)
    adv, rtg, steps = np.zeros((T, n)), np.zeros((T, n)), np.zeros((T, n), dtype=np.int64)
    s_adv, s_rtg = np.zeros((T, n)), np.zeros((T, n))
    for i in range(n):
        for t in range(T):
            e = t
            while not ends[e, i]:
                e += 1
            k = np.arange(e - t + 1)
            steps[t, i] = e - t
            adv[t, i] = np.sum((gamma * lam) ** k * delta[t:e + 1, i])
            rtg[t, i] = np.sum(gamma ** k * r[t:e + 1, i])
            s_adv[t, i] = np.sum((gamma * lam) ** k * mag[t:e + 1, i])
            s_rtg[t, i] = np.sum(gamma ** k * np.abs(r[t:e + 1, i]))
    return adv, rtg, steps, s_adv, s_rtg


# ---------------------------------------------------------------- critics
FUSED = [(5, 128), (4, 128)]  # ra.Mlp(engine, D, 128, 1): k_gae_scan<5> / <4>, k_value_targets_td<5> / <4>
# general critics, (in_dim, hidden_sizes, activation, bias vectors): none is a shape the fused kernels take
GENERAL = [(3, [16, 16], "Tanh", True), (8, [], "Identity", True), (5, [64, 64], "Relu", True),
           (1, [256], "Sigmoid", True), (7, [32], "Relu", False)]


def general_id(spec):
    D, hidden, act, bias = spec
    return "%d-%s-%s%s" % (D, "x".join(map(str, hidden)) or "linear", act, "" if bias else "-nobias")


def layer_dims(in_dim, hidden, out_dim):
    w = [in_dim] + list(hidden) + [out_dim]
    return list(zip(w[:-1], w[1:]))


def with_zero_biases(p, in_dim, hidden, out_dim):
    """the flat vector of a module without bias vectors, a zero bias inserted after every kernel: what the oracle's
    network takes (`acc = 0; acc = fma(x_k, w_k, acc)` is the bias-less chain)"""
    out, k = [], 0
    for fi, fo in layer_dims(in_dim, hidden, out_dim):
        out += [p[k:k + fi * fo], np.zeros(fo, dtype=np.float32)]
        k += fi * fo
    assert k == p.size
    return np.concatenate(out)


def general_num_params(spec):
    D, hidden, _, bias = spec
    return sum(fi * fo + (fo if bias else 0) for fi, fo in layer_dims(D, hidden, 1))


def general_expectation(spec, params, hist, gamma=GAMMA, lam=LAMBDA, td_gamma=TD_GAMMA, out_act="Identity"):
    """What a general critic's calls must leave, from the oracle's Mlp::forward (a k-ascending fma chain from the bias,
    as both device forwards are): V(obs[t]) for t <= T and V(term_obs) -> successors -> the oracle's array-fed scans"""
    D, hidden, act, bias = spec
    p = np.asarray(params, dtype=np.float32)
    p = p if bias else with_zero_biases(p, D, hidden, 1)
    T, n = hist["flag"].shape

    def V(planes, steps):  # [D][steps][n] -> [steps][n]
        x = np.ascontiguousarray(planes.reshape(D, steps * n).T)
        return O.mlp_layers_forward(D, hidden, 1, p, x, act, out_act)[:, 0].reshape(steps, n)

    values, v_term = V(hist["obs"], T + 1), V(hist["term_obs"], T)
    succ = successors(hist, v_term, values[T])
    adv, rtg = O.seq_gae(values[:T], succ, hist, gamma, lam)
    return dict(values=values, v_term=v_term, succ=succ, adv=adv, rtg=rtg,
                td=O.seq_one_step_targets(values[:T], succ, hist, np.float32(td_gamma)))


def returns_f32(hist, gamma):
    """reward_to_go alone (k_value_targets_rtg, k_gae_scan's rtg_only branch): scan_f32's returns need no value"""
    zero = np.zeros(hist["reward"].shape, dtype=np.float32)
    return scan_f32(zero, zero, hist, gamma, 0.0)[1]
