"""The slab reduction and the optimiser's column step return the bits they returned when tests/golden/reduce_bits.json
was recorded.

The table was recorded on the PARENT of the commit that wrote the column sum and the optimiser column once
(kernels_update.hip: k_reduce<CW>, k_reduce_opt<RULE, CW, XCHG> and k_opt_step over column_sum / OptColumn).
That fold changes no sum order and no rule, so every hash must survive
it, and every later edit of these kernels that means to keep the arithmetic.  The other GPU tests compare with an oracle
or a restatement within a tolerance or per rule; a reordered addition, a row group summed twice with a compensating miss,
or a state slot stored from the wrong register on ONE of the paths passes some of them and fails here.

The slabs' row counts follow the fused kernels' grid, and that the device's compute-unit count: the table holds the count
it was recorded on, and the test FAILS (it does not skip) on another.  It was recorded twice and the two records were equal.

One rank throughout.  Every rule runs with settings off its defaults so that every state slot it can have is live (RULES).
Cases, each the smallest shape that reaches a path of the shared code (CartPole rollouts of Mlp(5, 128, 2) unless said):

  step-narrow-RULE    critic_update of 3 steps on Mlp(5, 128, 1), 50 lanes x 13 steps, kernel variant 0.  P = 897, so
                      P + 4 = 56 x 16 + 5: 57 workgroups of 16 columns, the last with one gradient column and the four sum
                      columns.  3 slab rows for 64 row groups: most groups sum nothing.
  step-wide-RULE      the same on Mlp(5, [64, 32], 1): P = 2,497, P + 4 = 2,501 > 2,048 takes 64 columns per workgroup,
                      2,501 = 39 x 64 + 5.
  reduce-W-vV         reduce only: policy_gradient, policy_fvp, policy_loss_kl (slab B only) and critic_gradient on
                      Mlp(5, 128, 2) / Mlp(5, 128, 1) (W = narrow: P + 4 = 1,030 = 64 x 16 + 6) and on Mlp(5, [64, 32], 2) /
                      Mlp(5, [64, 32], 1) (W = wide), kernel variants 0 and 1.
  rows-257x64         kernel variant 1 at 257 lanes x 64 steps: B = 16,448 gives 257 rows of slab A — the row loop's second
                      trip holds exactly one row, in group 0 only — and 65 rows of slab B, a ragged last round of groups in
                      both widths.  policy_gradient, critic_gradient, and critic_update of 2 steps with Adam, on the
                      narrow and on the wide modules.
  host-RULE           Optimizer.step_host with a fixed gradient, twice, on Mlp(5, 128, 1): the stand-alone step without a
                      loss slot, veto word or weight image.
  gru-RULE            critic_update of 2 steps on GruMlp(5, 1) at 32 lanes x 3 steps of a Chain: the stand-alone step behind
                      the recurrent chains' reduction, with a loss slot.
What a step case hashes: the parameters, every state slot the rule has, the device's step count, and the losses.

    python tests/test_gpu_reduce_bits.py --record [--out FILE]

writes the table (run it on the commit whose bits are to be pinned).
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import relearn_amd as ra  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reduce_bits.json")

# rule -> (kind, settings off the defaults, number of live state slots)
RULES = {
    "adam": (ra.OPTIMIZER_ADAM, dict(learning_rate=3e-3, beta1=0.8, beta2=0.99, eps=1e-6), 2),
    "adamw": (ra.OPTIMIZER_ADAMW, dict(learning_rate=3e-3, weight_decay=5e-2), 2),
    "sgd": (ra.OPTIMIZER_SGD, dict(learning_rate=1e-3, momentum=0.9, nesterov=1, weight_decay=1e-3), 1),
    "rmsprop": (ra.OPTIMIZER_RMSPROP, dict(learning_rate=1e-3, alpha=0.95, momentum=0.9, centered=1, weight_decay=1e-3), 3),
}
WIDTHS = {"narrow": 128, "wide": [64, 32]}  # the hidden sizes whose P + 4 lies below / above reduce_width's threshold

CASES = {}
for _rule in RULES:
    for _w in WIDTHS:
        CASES["step-%s-%s" % (_w, _rule)] = ("step", _w, _rule)
for _w in WIDTHS:
    for _v in (0, 1):
        CASES["reduce-%s-v%d" % (_w, _v)] = ("reduce", _w, _v)
CASES["rows-257x64"] = ("rows",)
for _rule in RULES:
    CASES["host-%s" % _rule] = ("host", _rule)
for _rule in RULES:
    CASES["gru-%s" % _rule] = ("gru", _rule)


def bits(*arrays):
    """sha256 of the bytes a call returned and its first four values as hex words"""
    raw = b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)
    first = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint32) for a in arrays])[:4]
    return {"sha256": hashlib.sha256(raw).hexdigest(), "first": ["%08x" % w for w in first]}


def f32(*values):
    return np.array(values, dtype=np.float32)


def optimizer(module, rule):
    kind, settings, _ = RULES[rule]
    cfg = ra.optimizer_config_default(kind)
    for k, v in settings.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return ra.Optimizer(module, cfg)


def step_bits(module, opt, rule, losses):
    """parameters, every state slot the rule has, the device's step count, the losses"""
    state = [opt.state(s) for s in range(RULES[rule][2])]
    return bits(module.get_params(), *state, np.array([opt.step_count], dtype=np.uint64), losses)


def cartpole(eng, n, T):
    """a CartPole rollout of Mlp(5, 128, 2) with advantages and targets from Mlp(5, 128, 1)"""
    env = ra.CartPoleEnv(eng, n, max_steps=9, seed_env=5, seed_actor=6)
    pol, cri = ra.Mlp(eng, 5, 128, 2), ra.Mlp(eng, 5, 128, 1)
    pol.init(2)
    cri.init(3)
    traj = ra.Trajectory(eng, n, T, 5)
    ra.rollout(env, pol, traj)
    ra.gae(traj, cri, 0.99, 0.95)
    return traj


def modules(eng, width):
    pol, cri = ra.Mlp(eng, 5, WIDTHS[width], 2), ra.Mlp(eng, 5, WIDTHS[width], 1)
    pol.init(12)
    cri.init(13)
    return pol, cri


def reduce_only(out, tag, pol, cri, traj, every_call=True):
    g, loss, ent = ra.policy_gradient(pol, traj)
    out[tag + "rl_policy_gradient"] = bits(g, f32(loss, ent))
    g, loss = ra.critic_gradient(cri, traj)
    out[tag + "rl_critic_gradient"] = bits(g, f32(loss))
    if every_call:
        v = np.linspace(-1.0, 1.0, pol.P).astype(np.float32)
        out[tag + "rl_policy_fvp"] = bits(ra.policy_fvp(pol, traj, v, 1e-5))
        p0 = (pol.get_params() + np.float32(0.01) * v).astype(np.float32)
        out[tag + "rl_policy_loss_kl"] = bits(f32(*ra.policy_loss_kl(pol, traj, p0)))


def run_case(name):
    case = CASES[name]
    eng = ra.Engine(0)
    out = {}
    if case[0] == "step":
        _, width, rule = case
        eng.set_kernel_variant(0)
        traj = cartpole(eng, 50, 13)
        _, cri = modules(eng, width)
        assert cri.P == (897 if width == "narrow" else 2497), cri.P
        opt = optimizer(cri, rule)
        _, losses = ra.critic_update(cri, opt, traj, 3, want_losses=True)
        out["rl_critic_update"] = step_bits(cri, opt, rule, losses)
    elif case[0] == "reduce":
        _, width, variant = case
        eng.set_kernel_variant(variant)
        traj = cartpole(eng, 50, 13)
        pol, cri = modules(eng, width)
        reduce_only(out, "", pol, cri, traj)
    elif case[0] == "rows":
        eng.set_kernel_variant(1)
        traj = cartpole(eng, 257, 64)
        for width in WIDTHS:
            pol, cri = modules(eng, width)
            reduce_only(out, width + ":", pol, cri, traj, every_call=False)
            opt = optimizer(cri, "adam")
            _, losses = ra.critic_update(cri, opt, traj, 2, want_losses=True)
            out[width + ":rl_critic_update"] = step_bits(cri, opt, "adam", losses)
    elif case[0] == "host":
        rule = case[1]
        m = ra.Mlp(eng, 5, 128, 1)
        m.init(9)
        opt = optimizer(m, rule)
        g = (np.sin(np.arange(m.P, dtype=np.float64) * 0.37) * 0.5).astype(np.float32)
        opt.step_host(g)
        opt.step_host(g)
        out["rl_optimizer_step_host"] = step_bits(m, opt, rule, f32())
    else:
        rule = case[1]
        env = ra.ChainEnv(eng, 32, max_steps=2, seed_env=3, seed_actor=4)
        pol, cri = ra.GruMlp(eng, 5, 2), ra.GruMlp(eng, 5, 1)
        pol.init(21)
        cri.init(22)
        traj = ra.Trajectory(eng, 32, 3, 5)
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.95, 0.9)
        opt = optimizer(cri, rule)
        _, losses = ra.critic_update(cri, opt, traj, 2, want_losses=True)
        out["rl_critic_update"] = step_bits(cri, opt, rule, losses)
    eng.close()
    return out


def compute_units():
    eng = ra.Engine(0)
    cus = eng.info()[2]
    eng.close()
    return int(cus)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        table = json.load(f)
    cus = compute_units()
    assert cus == table["compute_units"], (
        "the table was recorded on a device with %d compute units, this one has %d: the slabs' row counts, and with them "
        "the order of the sums, differ — record a table for this device" % (table["compute_units"], cus))
    return table


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_reduce_bits(golden, name):
    got, want = run_case(name), golden["cases"][name]
    for call in sorted(got):
        print(name, call, got[call])
    assert got == want, {c: (got.get(c), want.get(c)) for c in set(got) | set(want) if got.get(c) != want.get(c)}


def record(path):
    table = {"compute_units": compute_units(), "cases": {name: run_case(name) for name in CASES}}
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(table["cases"]), path))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="write the table instead of checking it")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    if not args.record:
        ap.error("run under pytest to check; --record writes the table")
    record(args.out)
