"""The fused 5-128 kernels return the bits they returned when tests/golden/fused_5_128_bits.json was recorded.

k_policy_bf16, k_critic_step_mfma<1>, k_critic_step_mfma<2> and k_dqn_step_bf16 share their weight prologue, tile
dealing and walk, output transpose, owner-lane reduction and epilogue (bf16_tile.hpp).  Every sum in them has
a fixed order, so for a fixed grid a call returns the same bytes every time; this test pins those bytes — the sha256 of
what each call returns and its first four values — for kernel variant 0 on one rank, with fixed seeds and data from a
CartPole rollout.  The other GPU tests compare with an oracle within a tolerance; a reordered addition, a tile dealt
twice with a compensating miss, or a flush taken at another tile passes them and fails here.

The grid size, and with it the order of the sums, follows the device's compute-unit count: the table holds the count it
was recorded on, and the test FAILS (it does not skip) on another.

Shapes, each the smallest that reaches a path of the shared code:
  n = 64, T = 16       32 full tiles — fewer than one workgroup's virtual waves: most waves walk nothing and still define
                       their image
  n = 50, T = 13       20 full tiles and a ragged tile of 10 samples on the wave whose turn it is
  n = 32768, T = 128   (policy and critic calls) 131,072 tiles: on 256 compute units an older wave walks 80, more than
                       both flush periods (16 and 64) — the mid-walk flush, the f32 -> f64 fold and the final flush
  DQN                  a minibatch of whole episodes, >= 600 steps and not a multiple of 32, with reward-to-go and with
                       one-step TD targets.  rl_dqn_minibatch_gradient is given its targets either way and takes
                       k_critic_step_mfma<2>; k_dqn_step_bf16 forms one-step TD targets in the launch and is the kernel
                       of rl_dqn_update only, so each case also hashes the parameters after one update of two steps.  No
                       minibatch of practical size spans a flush period of those kernels (64 or 16 tiles per wave on
                       every wave of the grid: half a million steps and more), so none is built here.

    python tests/test_gpu_fused_bits.py --record [--out FILE]

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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_5_128_bits.json")
GAMMA = 0.99

# name -> (lanes, steps)
MODULE_CASES = {"64x16": (64, 16), "50x13": (50, 13), "32768x128": (32768, 128)}
# name -> one-step TD targets
DQN_CASES = {"dqn-reward-to-go": False, "dqn-one-step-td": True}
ALL_CASES = list(MODULE_CASES) + list(DQN_CASES)


def bits(*arrays):
    """sha256 of the bytes a call returned and its first four values as hex words"""
    raw = b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)
    first = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint32) for a in arrays])[:4]
    return {"sha256": hashlib.sha256(raw).hexdigest(), "first": ["%08x" % w for w in first]}


def f32(*values):
    return np.array(values, dtype=np.float32)


def run_module_case(name):
    n, T = MODULE_CASES[name]
    eng = ra.Engine(0)
    eng.set_kernel_variant(0)
    env = ra.CartPoleEnv(eng, n, max_steps=9, seed_env=5, seed_actor=6)
    pol, cri = ra.Mlp(eng, 5, 128, 2), ra.Mlp(eng, 5, 128, 1)
    pol.init(2)
    cri.init(3)
    traj = ra.Trajectory(eng, n, T, 5)
    ra.rollout(env, pol, traj)
    ra.gae(traj, cri, GAMMA, 0.95)
    out = {}
    g, loss, ent = ra.policy_gradient(pol, traj)
    out["rl_policy_gradient"] = bits(g, f32(loss, ent))
    v = np.linspace(-1.0, 1.0, pol.P).astype(np.float32)
    out["rl_policy_fvp"] = bits(ra.policy_fvp(pol, traj, v, 1e-5))
    p0 = pol.get_params()
    p0 = (p0 + np.float32(0.01) * v).astype(np.float32)
    out["rl_policy_loss_kl"] = bits(f32(*ra.policy_loss_kl(pol, traj, p0)))
    g, loss = ra.critic_gradient(cri, traj)
    out["rl_critic_gradient"] = bits(g, f32(loss))
    ppo = ra.ppo_config_default()
    ppo.opt_steps_per_update = 1
    popt = ra.Optimizer(pol, ra.optimizer_config_default(ra.OPTIMIZER_ADAM))
    ra.ppo_update(pol, popt, traj, ppo)
    out["rl_ppo_update"] = bits(pol.get_params())
    eng.close()
    return out


def run_dqn_case(name):
    td = DQN_CASES[name]
    eng = ra.Engine(0)
    eng.set_kernel_variant(0)
    env = ra.CartPoleEnv(eng, 64, max_steps=9, limit=ra.LIMIT_VISIBLE, seed_env=21, seed_actor=34)
    q = ra.Mlp(eng, 5, 128, 2)
    q.init(77)
    opt = ra.Optimizer(q, ra.optimizer_config_default(ra.OPTIMIZER_ADAM))
    cfg = ra.dqn_config_default()
    cfg.target = ra.DQN_TARGET_ONE_STEP_TD if td else ra.DQN_TARGET_REWARD_TO_GO
    cfg.exploration_kind, cfg.exploration_start = ra.SCHEDULE_CONSTANT, 0.3
    cfg.minibatch_steps, cfg.opt_steps_per_update, cfg.buffer_capacity, cfg.discount_factor = 600, 2, 64, GAMMA
    dqn = ra.Dqn(env, q, opt, cfg)
    dqn.collect(32)
    # whole episodes until the minibatch holds >= 600 steps: keep the first draw whose count is off the tile grid
    for _ in range(8):
        _, steps = dqn.minibatch_sample()
        if steps % 32:
            break
    assert 600 <= steps <= 4096 and steps % 32, steps
    g, loss = dqn.minibatch_gradient()
    out = {"rl_dqn_minibatch_gradient": bits(g, f32(loss), np.array([steps], dtype=np.uint32))}
    st, losses = dqn.update(want_losses=True)
    out["rl_dqn_update"] = bits(q.get_params(), losses, np.array([st.last_minibatch_steps], dtype=np.uint32))
    dqn.close()
    eng.close()
    return out


def run_case(name):
    return (run_module_case if name in MODULE_CASES else run_dqn_case)(name)


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
def test_fused_bits(golden, name):
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
