"""The case table of the narrow and 4-input single-hidden-layer modules (tests/test_gpu_narrow_mlp.py on the device,
tests/test_narrow_cases_cpu.py for the table itself), and the oracle side of every case, computed once and shared.

rl_mlp_create takes in_dim 4 or 5, hidden 1..128, out_dim 1 or 2; only 5-128 runs the fused matrix-pipe kernels.  Every
other shape runs the hand-written f32 family at both kernel variants, and that family has branches 5-128 never takes.
The shapes below are the smallest that reach each of them ((in_dim, hidden)):
  (5, 1)    every unit is in the tail and only thread 0 of a group owns one; P = 10 (policy) and 8 (critic)
  (5, 15)   tail only, and every group size G deals it unevenly
  (5, 17)   one full block of 16 units plus one tail unit
  (5, 100)  six blocks plus four tail units: at G = 16 threads 0-3 own one, at G = 8 threads 0-1 two each
  (5, 127)  seven blocks plus 15 tail units: at G = 2 the second thread owns 7 of its 8 chains
  (5, 64)   no tail, and not the fused shape
  (4, 37), (4, 64), (4, 128)  the <4, ...> instantiations (the fifth slot of the packed LDS record stays empty), on
            lanes without a step limit and with a hidden one; 4-128 is the fused tests' width on the path they never take

Nothing here imports the device library: the CPU test runs this module alone.
"""
import ctypes as C

import numpy as np

import oracle as O

GRAD_RTOL = 1e-6  # tests/test_gpu_parity.py's bar for one f32 gradient, relative to max |g|

SHAPES = [(5, 1), (5, 15), (5, 17), (5, 100), (5, 127), (5, 64), (4, 37), (4, 64), (4, 128)]
TAIL_SHAPES = [s for s in SHAPES if s[1] % 16]


def shape_id(shape):
    return "%d-%d" % shape


# ---------------------------------------------------------------- rollouts, one lane count per group size
# launch_rollout (kernels_rollout.hip) picks the threads per lane, G, from the lane count n and S = 4 * CUs * 64:
#   G = 16 for n <= S / 16, 8 for n <= S / 8, 4 for n <= S / 2, 2 for n <= S, 1 above.
# Whoever changes that rule changes these lane counts with it.  None is a multiple of 64: the last wave is ragged.
ROLLOUT_T, ROLLOUT_MAX_STEPS, ROLLOUT_PERIODS = 9, 9, 2  # two periods: the second crosses word 16 of the actor stream
ROLLOUT_SEEDS = dict(seed_env=5, seed_actor=6)


def rollout_lanes(cus):
    S = 4 * cus * 64
    return {16: 96, 8: S // 16 + 40, 4: S // 8 + 40, 2: S // 2 + 40, 1: S + 40}


def rollout_group(n, cus):
    """the host rule restated (for the CPU test of rollout_lanes)"""
    S, G = 4 * cus * 64, 1
    while G < 16 and n * 2 * G <= (1 if 2 * G >= 8 else 2) * S:
        G *= 2
    return G


# launch_rollout_dqn (kernels_dqn.hip) has another rule: G doubles while n * 2G <= S, so G = 8 for S / 16 < n <= S / 8
# (and G = 1 at kernel variant 1 or when every action is drawn).
def dqn_lanes_g8(cus):
    return 4 * cus * 64 // 16 + 40


def dqn_group(n, cus):
    S, G = 4 * cus * 64, 1
    while G < 16 and n * 2 * G <= S:
        G *= 2
    return G


# (shape, limit, group sizes): every G at three tail shapes, G = 16 at every shape, the 4-input tail shape on both of its
# envs at the widest group, a middle one and one thread per lane
ROLLOUT_CASES = (
    [(s, O.LIMIT_VISIBLE, (16, 8, 4, 2, 1)) for s in ((5, 15), (5, 100), (5, 127))]
    + [(s, O.LIMIT_VISIBLE, (16,)) for s in ((5, 1), (5, 17), (5, 64))]
    + [((4, 37), O.LIMIT_NONE, (16, 8, 1)), ((4, 37), O.LIMIT_LATENT, (16, 8, 1))]
    + [((4, 64), O.LIMIT_NONE, (16,)), ((4, 128), O.LIMIT_LATENT, (16,))])

# ---------------------------------------------------------------- update trajectories
# Two per shape.  "ragged": 50 lanes x 13 steps, B = 650 — no multiple of 8 (k_mlp_backward's one-sample tail loop), a
# ragged last chunk.  "tiny": 3 lanes x 5 steps, B = 15 — less than one chunk, less than two groups of 8.  The lanes run
# `warmup` periods of T steps before the one that is used, so that a window of five steps can hold episode ends.
# Seeds (env, actor) and warm-up were searched with the oracle alone, from (5, 6, 0) upwards, until the data conditions
# of tests/test_narrow_cases_cpu.py held; modules are initialised from MODULE_SEEDS.
# shape -> (policy init seed, critic init seed): 2 and 3 as everywhere in the suite, except where the last hidden unit
# of the module so initialised never fires on the case's data (a lost tail unit would then change nothing): there the next
# seeds upwards for which it does
MODULE_SEEDS = {(5, 1): (2, 3), (5, 15): (2, 4), (5, 17): (2, 3), (5, 100): (5, 5), (5, 127): (3, 3), (5, 64): (2, 3),
                (4, 37): (2, 3), (4, 64): (2, 3), (4, 128): (2, 3)}
GAMMA, LAMBDA = 0.99, 0.95
RAGGED = dict(n=50, T=13)
TINY = dict(n=3, T=5)


def _limit_of(shape):
    return {(4, 37): O.LIMIT_LATENT, (4, 64): O.LIMIT_NONE, (4, 128): O.LIMIT_LATENT}.get(shape, O.LIMIT_VISIBLE)


# shape -> kind -> (max_steps, seed_env, seed_actor, warmup)
UPDATE_SEEDS = {
    (5, 1): {"ragged": (9, 6, 7, 0), "tiny": (9, 19, 20, 1)},
    (5, 15): {"ragged": (9, 5, 6, 0), "tiny": (9, 5, 6, 1)},
    (5, 17): {"ragged": (9, 5, 6, 0), "tiny": (9, 5, 6, 1)},
    (5, 100): {"ragged": (9, 5, 6, 0), "tiny": (9, 5, 6, 1)},
    (5, 127): {"ragged": (9, 8, 9, 0), "tiny": (9, 69, 70, 1)},
    (5, 64): {"ragged": (9, 6, 7, 0), "tiny": (9, 59, 60, 1)},
    (4, 37): {"ragged": (9, 5, 6, 0), "tiny": (9, 5, 6, 1)},
    (4, 64): {"ragged": (9, 5, 6, 0), "tiny": (9, 5, 6, 2)},
    (4, 128): {"ragged": (9, 6, 7, 0), "tiny": (9, 59, 60, 1)},
}


def update_case(shape, kind):
    max_steps, seed_env, seed_actor, warmup = UPDATE_SEEDS[shape][kind]
    return dict(RAGGED if kind == "ragged" else TINY, kind=kind, shape=shape, limit=_limit_of(shape),
                max_steps=max_steps, seed_env=seed_env, seed_actor=seed_actor, warmup=warmup)


UPDATE_KINDS = ("ragged", "tiny")

# Hidden units whose ReLU fires on no sample of a case's trajectory, (shape, kind) -> units, policy and critic: their
# rows of the gradients are zero in the oracle too, and losing one of them changes nothing.  Every other unit's rows, and
# both output biases, have a non-zero f32-oracle gradient (tests/test_narrow_cases_cpu.py checks the lists and that).
DEAD_POLICY_UNITS = {
    ((5, 1), "ragged"): [],
    ((5, 1), "tiny"): [],
    ((5, 15), "ragged"): [0, 1, 12],
    ((5, 15), "tiny"): [0, 1, 3, 12],
    ((5, 17), "ragged"): [0, 1, 3, 11, 12, 15],
    ((5, 17), "tiny"): [0, 1, 3, 11, 12, 15],
    ((5, 100), "ragged"): [5, 20, 23, 34, 76, 77, 84, 92],
    ((5, 100), "tiny"): [5, 20, 23, 24, 29, 34, 39, 40, 43, 52, 54, 60, 74, 76, 77, 78, 79, 82, 84, 89, 90, 92, 98],
    ((5, 127), "ragged"): [8, 10, 14, 19, 35, 37, 62, 68, 81, 99, 109, 119],
    ((5, 127), "tiny"): [8, 10, 14, 17, 18, 19, 26, 35, 37, 57, 62, 68, 81, 84, 94, 99, 107, 109, 119],
    ((5, 64), "ragged"): [10, 23],
    ((5, 64), "tiny"): [5, 10, 11, 19, 23, 25, 33, 35, 38, 40, 54, 57],
    ((4, 37), "ragged"): [15, 24, 27, 28],
    ((4, 37), "tiny"): [4, 7, 11, 12, 15, 17, 24, 27, 28, 29, 32],
    ((4, 64), "ragged"): [20, 42, 57],
    ((4, 64), "tiny"): [12, 15, 20, 37, 42, 43, 53, 56, 57],
    ((4, 128), "ragged"): [19, 45, 58, 67, 68, 81, 91, 113, 114, 116, 124, 125],
    ((4, 128), "tiny"): [1, 5, 6, 9, 10, 19, 20, 23, 30, 35, 45, 46, 51, 53, 58, 61, 62, 65, 67, 68, 77, 81, 86, 87,
                         91, 94, 102, 108, 109, 113, 114, 115, 116, 120, 123, 124, 125],
}
DEAD_CRITIC_UNITS = {
    ((5, 1), "ragged"): [],
    ((5, 1), "tiny"): [],
    ((5, 15), "ragged"): [1, 12],
    ((5, 15), "tiny"): [1, 12, 13],
    ((5, 17), "ragged"): [2, 8, 14],
    ((5, 17), "tiny"): [2, 8, 14],
    ((5, 100), "ragged"): [5, 20, 23, 34, 76, 77, 84, 92],
    ((5, 100), "tiny"): [5, 20, 23, 24, 29, 34, 39, 40, 43, 52, 54, 60, 74, 76, 77, 78, 79, 82, 84, 89, 90, 92, 98],
    ((5, 127), "ragged"): [8, 10, 14, 19, 35, 37, 62, 68, 81, 99, 109, 119],
    ((5, 127), "tiny"): [8, 10, 14, 17, 18, 19, 26, 35, 37, 57, 62, 68, 81, 84, 94, 99, 107, 109, 119],
    ((5, 64), "ragged"): [3, 6, 14, 26, 28, 35, 37, 41],
    ((5, 64), "tiny"): [3, 6, 14, 26, 28, 31, 35, 37, 41, 50, 52, 57],
    ((4, 37), "ragged"): [4, 17, 20, 26],
    ((4, 37), "tiny"): [0, 1, 4, 16, 17, 20, 25, 26, 31, 32],
    ((4, 64), "ragged"): [3, 11, 17, 19, 27, 47, 54, 61, 63],
    ((4, 64), "tiny"): [1, 3, 5, 11, 17, 19, 27, 33, 45, 47, 54, 58, 61, 63],
    ((4, 128), "ragged"): [4, 8, 9, 15, 17, 19, 26, 27, 33, 38, 45, 47, 53, 61, 73, 82, 92, 104, 107, 113, 116],
    ((4, 128), "tiny"): [2, 4, 8, 9, 12, 15, 17, 19, 22, 26, 27, 33, 35, 37, 38, 45, 46, 47, 48, 50, 53, 58, 59, 61,
                         63, 65, 67, 69, 73, 82, 90, 92, 96, 99, 104, 107, 113, 116, 120],
}


def shapes_of(shape):
    D, H = shape
    return O.MlpShape(D, H, 2), O.MlpShape(D, H, 1)


def blocks(shape, out_dim):
    """the flat parameter vector's blocks, in the reference's order"""
    D, H = shape
    return {"W1": slice(0, D * H), "b1": slice(D * H, D * H + H), "W2": slice(D * H + H, D * H + H + out_dim * H),
            "b2": slice(D * H + H + out_dim * H, D * H + H + out_dim * H + out_dim)}


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def drop_last_unit(shape, out_dim, params):
    """the parameters a kernel that loses the last hidden unit computes with: that unit's W2 column zeroed"""
    D, H = shape
    p = params.copy()
    for a in range(out_dim):
        p[D * H + H + a * H + H - 1] = 0.0
    return p


# ---------------------------------------------------------------- the oracle side, once per case
_cache = {}


def oracle_rollout(shape, limit, n, T=ROLLOUT_T, max_steps=ROLLOUT_MAX_STEPS, periods=ROLLOUT_PERIODS, params=None,
                   **seeds):
    """`periods` successive rollouts of the oracle's lanes, and the lane state after each"""
    seeds = seeds or ROLLOUT_SEEDS
    key = ("rollout", shape, limit, n, T, max_steps, periods, tuple(sorted(seeds.items())), params is None)
    if params is None and key in _cache:
        return _cache[key]
    ps, _ = shapes_of(shape)
    pp = O.mlp_init(ps, MODULE_SEEDS[shape][0]) if params is None else params
    sim = O.LaneSim(n, max_steps=max_steps, limit=limit, **seeds)
    out = []
    for _ in range(periods):
        want = sim.rollout(ps, pp, T)
        out.append((want, sim.get_state()))
    if params is None:
        _cache[key] = out
    return out


def policy_grad32(ps, pp, x, a, adv):
    g, loss = np.zeros_like(pp), C.c_float()
    O.lib().oracle_policy_grad_f32(ps, O.f32p(pp), O.f32p(x), O.i64p(a), O.f32p(adv), len(a), O.f32p(g), C.byref(loss))
    return g, loss.value


def policy_grad64(ps, pp, x, a, adv):
    g, loss = np.zeros(len(pp), dtype=np.float64), C.c_double()
    O.lib().oracle_policy_grad_f64(ps, O.f64p(pp.astype(np.float64)), O.f64p(x.astype(np.float64)), O.i64p(a),
                                   O.f64p(adv.astype(np.float64)), len(a), O.f64p(g), C.byref(loss))
    return g, loss.value


def policy_fvp32(ps, pp, x, v, reg):
    hv = np.zeros_like(pp)
    O.lib().oracle_policy_fvp_f32(ps, O.f32p(pp), O.f32p(x), len(x), O.f32p(v), reg, O.f32p(hv))
    return hv


def policy_fvp64(ps, pp, x, v, reg):
    hv = np.zeros(len(pp), dtype=np.float64)
    O.lib().oracle_policy_fvp_f64(ps, O.f64p(pp.astype(np.float64)), O.f64p(x.astype(np.float64)), len(x),
                                  O.f64p(v.astype(np.float64)), float(np.float32(reg)), O.f64p(hv))
    return hv


def critic_grad32(cs, cp, x, tgt):
    g, loss = np.zeros_like(cp), C.c_float()
    O.lib().oracle_critic_grad_f32(cs, O.f32p(cp), O.f32p(x), O.f32p(tgt), len(x), O.f32p(g), C.byref(loss))
    return g, loss.value


def critic_grad64(cs, cp, x, tgt):
    return O.grad_f64_mt("critic", cs, cp, x, aux=tgt)


FVP_REG = 1e-5


def oracle_update_case(shape, kind):
    """everything the update checks of one case need from the oracle: the trajectory (after the warm-up periods), the
    flat samples, values / advantages / returns / TD targets, and the f32 and f64 gradients"""
    key = ("update", shape, kind)
    if key in _cache:
        return _cache[key]
    case = update_case(shape, kind)
    ps, cs = shapes_of(shape)
    pp, cp = O.mlp_init(ps, MODULE_SEEDS[shape][0]), O.mlp_init(cs, MODULE_SEEDS[shape][1])
    periods = oracle_rollout(shape, case["limit"], case["n"], case["T"], case["max_steps"], case["warmup"] + 1,
                             seed_env=case["seed_env"], seed_actor=case["seed_actor"])
    want = periods[-1][0]
    r = dict(case=case, ps=ps, cs=cs, pp=pp, cp=cp, want=want, state=periods[-1][1])
    r["values"], adv, rtg = O.lanes_gae(cs, cp, want, GAMMA, LAMBDA)
    r["adv2d"], r["rtg2d"] = adv, rtg
    r["td2d"] = O.lanes_one_step_targets(cs, cp, want, np.float32(GAMMA))
    x, a = O.flat_samples(want)
    adv, rtg = np.ascontiguousarray(adv.reshape(-1)), np.ascontiguousarray(rtg.reshape(-1))
    r.update(x=x, a=a, adv=adv, rtg=rtg, td=np.ascontiguousarray(r["td2d"].reshape(-1)))
    r["g32"], r["loss32"] = policy_grad32(ps, pp, x, a, adv)
    r["c32"], r["closs32"] = critic_grad32(cs, cp, x, rtg)
    r["v"] = np.random.default_rng(1).standard_normal(len(pp)).astype(np.float32)
    r["u"] = np.random.default_rng(7).standard_normal(len(pp)).astype(np.float32)
    r["hv32"] = policy_fvp32(ps, pp, x, r["v"], FVP_REG)
    r["g64"], r["loss64"] = policy_grad64(ps, pp, x, a, adv)
    r["c64"], r["closs64"] = critic_grad64(cs, cp, x, rtg)
    r["hv64"] = policy_fvp64(ps, pp, x, r["v"], FVP_REG)
    _cache[key] = r
    return r


def adam_cfg(lr=1e-3):
    cfg = O.AdamCfg()
    O.lib().oracle_adam_cfg_default(C.byref(cfg))
    cfg.lr = lr
    return cfg


PPO_RUNS = {"default": (1e-3, 10), "clipping-active": (2e-2, 8)}  # tests/test_gpu_ppo.py's (learning rate, steps)


def policy_logp32(ps, pp, x, a):
    lp = np.zeros(len(a), np.float32)
    O.lib().oracle_policy_logp_f32(ps, O.f32p(pp), O.f32p(x), O.i64p(a), len(a), O.f32p(lp), None)
    return lp


def oracle_ppo(shape, kind, run):
    """the oracle's clipped PPO steps on a case -> (parameters, per-step losses, entropy, share of the samples whose
    ratio under the final parameters is outside [0.8, 1.2])"""
    key = ("ppo", shape, kind, run)
    if key not in _cache:
        r = oracle_update_case(shape, kind)
        lr, steps = PPO_RUNS[run]
        p, losses, ent, cfg = r["pp"].copy(), np.zeros(steps, np.float32), C.c_float(), adam_cfg(lr)
        st = O.lib().oracle_adam_new(len(p))
        O.lib().oracle_ppo_update_f32(r["ps"], O.f32p(p), st, C.byref(cfg), O.f32p(r["x"]), O.i64p(r["a"]),
                                      O.f32p(r["adv"]), len(r["a"]), steps, 0.2, O.f32p(losses), C.byref(ent))
        O.lib().oracle_adam_free(st)
        ratio = np.exp(policy_logp32(r["ps"], p, r["x"], r["a"]) - policy_logp32(r["ps"], r["pp"], r["x"], r["a"]))
        _cache[key] = (p, losses, ent.value, float(((ratio < 0.8) | (ratio > 1.2)).mean()))
    return _cache[key]


def oracle_critic_steps(shape, kind, targets, steps):
    """`steps` Adam steps of the oracle's critic on the case's samples against `targets` ("rtg" or "td")"""
    key = ("critic", shape, kind, targets, steps)
    if key not in _cache:
        r = oracle_update_case(shape, kind)
        c, losses, cfg = r["cp"].copy(), np.zeros(steps, np.float32), adam_cfg()
        st = O.lib().oracle_adam_new(len(c))
        O.lib().oracle_critic_update_f32(r["cs"], O.f32p(c), st, C.byref(cfg), O.f32p(r["x"]), O.f32p(r[targets]),
                                         len(r["a"]), steps, O.f32p(losses))
        O.lib().oracle_adam_free(st)
        _cache[key] = (c, losses)
    return _cache[key]


# ---------------------------------------------------------------- DQN collection (the oracle half of test_gpu_dqn.make)
# (hidden, limit, seed of the action-value module).  make() initialises from seed 77; the 5-100-2 module of that seed
# prefers one action by 0.57 or more on every state these lanes reach, so its greedy branch never notices a lost unit:
# that case runs the parameters of seed 83, the next seed upwards whose collection changes when the last unit is lost.
DQN_CASES = [(100, O.LIMIT_VISIBLE, 83), (37, O.LIMIT_NONE, 77)]
DQN_COLLECT = dict(capacity=48, T=30, reps=2, eps=0.3, max_steps=23)  # the second collection evicts


def grad_check(name, shape, out_dim, got, f32, f64):
    """The bar of a device gradient or Fisher-vector product (tests/test_gpu_dqn_update_steps.py's form): with e32 the
    f32 oracle's own distance from the f64 oracle, the device is no farther from f64 than GRAD_RTOL + 2 e32, relative to
    max |g|, and every parameter block is within 50 times that, relative to the whole vector's maximum.  (Two correct
    f32 sums differ by more than 1e-6 here: the f32 oracle itself sits up to 7.6e-7 from f64 at B = 650.)  Returns
    (device error, e32, bar, failures): the caller asserts that `failures` is empty."""
    e32, err = rel_err(f32, f64), rel_err(got, f64)
    bar = GRAD_RTOL + 2.0 * e32
    scale = max(np.abs(f64).max(), 1e-30)
    per_block = {k: np.abs(np.asarray(got, dtype=np.float64)[s] - f64[s]).max() / scale
                 for k, s in blocks(shape, out_dim).items()}
    print("%s %s: e32 %.3g, device vs f64 %.3g (bar %.3g); per block %s (bar %.3g)" % (
        shape_id(shape), name, e32, err, bar, {k: "%.3g" % v for k, v in per_block.items()}, 50.0 * bar))
    failures = [] if err <= bar else [("whole", err, bar)]
    failures += [(k, v, 50.0 * bar) for k, v in per_block.items() if not v <= 50.0 * bar]
    return err, e32, bar, failures
