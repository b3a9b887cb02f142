"""The general-MLP fused kernels return the bits they returned when tests/golden/gen_mfma_bits.json was recorded.

k_gen_mfma (a 32-sample tile per wave) and k_gen_pair (a tile per pair of waves) share their image layout, tile fetch,
piece packing, slab row, f32 -> f64 fold and epilogue (kernels_gen_mfma.hip).  Every sum in them has a fixed
order, so for a fixed grid a call returns the same bytes every time; this test pins those bytes — the sha256 of what
each call returns and its first four words — for kernel variant 0 on one rank, with fixed seeds.  The other GPU tests
compare with an f64 network within a tolerance; a reordered addition, a flush taken at another tile or a padding lane
that counts passes them and fails here.

The grid size, and with it the order of the sums, follows the device's compute-unit count: the table holds the count it
was recorded on, and the test FAILS (it does not skip) on another.

Calls per case: policy_gradient (PASS_INIT), policy_fvp (PASS_JVP), policy_loss_kl at perturbed parameters (PASS_EVAL,
always the one-wave kernel), critic_gradient (GM_CRITIC) and one ppo_update of one step (PASS_PPO; the parameters).

Networks (biases on; each the smallest that reaches an instantiation), on a CartPole rollout by a fused 5-128 policy:
  [64, 64] Relu            NL = 2: the gradient modes and the JVP take the pair kernel
  [33] Relu                one hidden layer of at most 128 Relu units with an Identity output over 5 inputs is NOT a
                           general module: these calls run the single-hidden-layer kernels, and the case pins those
  [33] Relu, Tanh output   ... so this one is the NL = 1 case with a padded second tile on the pair kernel
  [32, 16, 8] Sigmoid, Tanh output   NL = 3 with padded widths; its JVP needs more than 160 KB of LDS on both kernels
                           and takes the per-layer path: policy_fvp is left out of its hash
  [128] Tanh               GW = 4: the one-wave kernel in every mode, the JVP included
and [16, 16] Relu over 7 inputs (GM_MAX_IN: the bias input in the eighth slot) on a host-made history of n = 70, T = 9.

Sample counts (tile arithmetic for 256 compute units):
  n = 3, T = 5         15 samples: one ragged tile; three of a workgroup's four pairs run on zeros, three waves of the
                       one-wave kernel leave at wave_id >= n_tiles
  n = 50, T = 13       650 samples: 20 full tiles and a ragged one of 10: 6 workgroups, 24 pairs, 3 without a tile; fewer
                       slab rows than waves in the one-wave launch
  n = 16400, T = 129   ([64, 64] Relu and [128] Tanh) 66,113 tiles, the last of 16 samples, on 1,024 waves or pairs: 577
                       walk 65 tiles — the mid-walk flush at 64 (GM_FLUSH), one more tile, the final flush; the others
                       walk 64 — the period flush is the last one, and a pair runs a 65th iteration on zeros.  No
                       smaller size reaches a second flush.

    python tests/test_gpu_gen_mfma_bits.py --record [--out FILE]

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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_mfma_bits.json")
GAMMA = 0.99

# name -> (hidden sizes, activation, output activation, hash policy_fvp)
NETS = {"64-64-relu": ([64, 64], "Relu", "Identity", True),
        "33-relu": ([33], "Relu", "Identity", True),
        "33-relu-tanh-out": ([33], "Relu", "Tanh", True),
        "32-16-8-sigmoid-tanh-out": ([32, 16, 8], "Sigmoid", "Tanh", False),
        "128-tanh": ([128], "Tanh", "Identity", True)}
SIZES = {"3x5": (3, 5), "50x13": (50, 13)}
BIG = {"16400x129": (16400, 129)}
BIG_NETS = ("64-64-relu", "128-tanh")
ROLLOUT_CASES = {"%s@%s" % (net, size): (net, nT) for size, nT in SIZES.items() for net in NETS}
ROLLOUT_CASES.update({"%s@%s" % (net, size): (net, nT) for size, nT in BIG.items() for net in BIG_NETS})
HOST_CASE = "in7-16-16-relu@70x9"
ALL_CASES = list(ROLLOUT_CASES) + [HOST_CASE]


def bits(*arrays):
    """sha256 of the bytes a call returned and its first four values as hex words"""
    raw = b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)
    first = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint32) for a in arrays])[:4]
    return {"sha256": hashlib.sha256(raw).hexdigest(), "first": ["%08x" % w for w in first]}


def f32(*values):
    return np.array(values, dtype=np.float32)


def hash_calls(eng, pol, cri, traj, with_fvp):
    out = {}
    g, loss, ent = ra.policy_gradient(pol, traj)
    out["rl_policy_gradient"] = bits(g, f32(loss, ent))
    v = np.linspace(-1.0, 1.0, pol.P).astype(np.float32)
    if with_fvp:
        out["rl_policy_fvp"] = bits(ra.policy_fvp(pol, traj, v, 1e-5))
    p0 = (pol.get_params() + np.float32(0.01) * v).astype(np.float32)
    out["rl_policy_loss_kl"] = bits(f32(*ra.policy_loss_kl(pol, traj, p0)))
    g, loss = ra.critic_gradient(cri, traj)
    out["rl_critic_gradient"] = bits(g, f32(loss))
    ppo = ra.ppo_config_default()
    ppo.opt_steps_per_update = 1
    popt = ra.Optimizer(pol, ra.optimizer_config_default(ra.OPTIMIZER_ADAM))
    ra.ppo_update(pol, popt, traj, ppo)
    out["rl_ppo_update"] = bits(pol.get_params())
    return out


def run_rollout_case(name):
    net, (n, T) = ROLLOUT_CASES[name]
    hidden, act, out_act, with_fvp = NETS[net]
    eng = ra.Engine(0)
    eng.set_kernel_variant(0)
    env = ra.CartPoleEnv(eng, n, max_steps=9, seed_env=5, seed_actor=6)
    fpol = ra.Mlp(eng, 5, 128, 2)
    fpol.init(2)
    pol, cri = ra.Mlp(eng, 5, hidden, 2, act, out_act), ra.Mlp(eng, 5, hidden, 1, act, out_act)
    pol.init(4)
    cri.init(3)
    traj = ra.Trajectory(eng, n, T, 5)
    ra.rollout(env, fpol, traj)
    ra.gae(traj, cri, GAMMA, 0.95)
    out = hash_calls(eng, pol, cri, traj, with_fvp)
    eng.close()
    return out


def run_host_case():
    in_dim, hidden, n, T = 7, [16, 16], 70, 9
    eng = ra.Engine(0)
    eng.set_kernel_variant(0)
    rng = np.random.default_rng(in_dim * 31 + len(hidden))
    pol, cri = ra.Mlp(eng, in_dim, hidden, 2, "Relu", "Identity"), ra.Mlp(eng, in_dim, hidden, 1, "Relu", "Identity")
    pol.init(21)
    cri.init(22)
    traj = ra.Trajectory(eng, n, T, in_dim)
    traj.write_all({"obs": rng.normal(size=(in_dim, T + 1, n)).astype(np.float32),
                    "flag": rng.choice(np.array([0, 0, 0, 1, 2], dtype=np.uint8), size=(T, n)),
                    "term_obs": rng.normal(size=(in_dim, T, n)).astype(np.float32),
                    "action": rng.integers(0, 2, size=(T, n)).astype(np.uint8),
                    "reward": rng.normal(size=(T, n)).astype(np.float32)})
    ra.gae(traj, cri, GAMMA, 0.95)
    out = hash_calls(eng, pol, cri, traj, True)
    eng.close()
    return out


def run_case(name):
    return run_host_case() if name == HOST_CASE else run_rollout_case(name)


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
        "the table was recorded on a device with %d compute units, this one has %d: the grid, and with it the order "
        "of the sums, differs — record a table for this device" % (table["compute_units"], cus))
    return table


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_CASES)
def test_gen_mfma_bits(golden, name):
    got, want = run_case(name), golden["cases"][name]
    for call in sorted(got):
        print(name, call, got[call])
    assert got == want, {c: (got.get(c), want.get(c)) for c in set(got) | set(want) if got.get(c) != want.get(c)}


def record(path):
    table = {"compute_units": compute_units(), "cases": {name: run_case(name) for name in ALL_CASES}}
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
