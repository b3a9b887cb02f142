"""Which kernels every update entry point launches, per module family, pinned against a recorded table.

The host code chooses a kernel family for a module (fused 5-128, general matrix-pipe, per-layer, recurrent tile,
recurrent lane-per-thread) and sequences forward, backward, slab reduction and all-reduce.  The other GPU tests check
what those passes compute; this one checks WHICH launches make them up: with rl_profile_* enabled, one call is made and
the per-class launch counts are compared with tests/golden/pass_launch_counts.json.  A module that silently moves to
another family, a pass that gains or loses a launch, or a reduce-and-step that stops being fused shows up here even
where the numbers stay right.

No count depends on data: the TRPO updates run two CG iterations and two line-search candidates (both enqueued before
the first read-back, the CG exit is taken on the device), and per-kernel profiling keeps the DQN draws on one stream.

    python tests/test_gpu_pass_paths.py --record [--out FILE]

writes the table (run it on the commit whose sequences are to be pinned).
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import relearn_amd as ra  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pass_launch_counts.json")
N, T = 64, 16  # 64 lanes keep the 32-lane recurrent tiles, B = 1024 spans several slab rows
GAMMA = 0.99


def mlp(hidden, **kw):
    return lambda eng, out_dim: ra.Mlp(eng, 5, hidden, out_dim, **kw)


def rnn(cls, *widths, **kw):
    return lambda eng, out_dim: cls(eng, 5, out_dim, *widths, **kw)


# name -> (module constructor, kernel variant, host collective installed, three-armed bandit)
MODULE_CASES = {
    "fused-5-128": (mlp(128), 0, False, False),
    "fused-5-128-variant-1": (mlp(128), 1, False, False),
    "hidden-64": (mlp(64), 0, False, False),               # the fused launcher declines; not `general`
    "general-64-64": (mlp([64, 64]), 0, False, False),     # the general matrix-pipe kernel
    "no-hidden-layer": (mlp([]), 0, False, False),         # per-layer
    "no-bias": (mlp(128, bias=False), 0, False, False),    # per-layer
    "gru-128": (rnn(ra.GruMlp), 0, False, False),
    "gru-32-padded-twin": (rnn(ra.GruMlp, 32, 32), 0, False, False),
    "lstm-2-layers": (rnn(ra.LstmMlp, 16, 12, num_layers=2), 0, False, False),  # lane-per-thread
    "bandit-3-actions": (mlp([32]), 0, False, True),
    "fused-5-128-host-collective": (mlp(128), 0, True, False),  # the un-fused reduce-then-step path
}

# name -> (hidden_sizes, one-step TD targets, kernel variant)
DQN_CASES = {
    "dqn-fused-reward-to-go": (128, False, 0),
    "dqn-fused-one-step-td": (128, True, 0),
    "dqn-general-one-step-td": ([64, 64], True, 0),
    "dqn-fused-variant-1": (128, False, 1),
}


class Case:
    """an engine of its own (kernel variant, collective and profiling are engine state) and the counts of its calls"""

    def __init__(self, variant=0, host_collective=False):
        self.eng = ra.Engine(0)
        self.eng.set_kernel_variant(variant)
        if host_collective:
            self.eng.comm_init_host(0, 1, lambda a: None)  # one rank: the sum is the array itself
        self.eng.profile_enable(True)
        self.counts = {}

    def call(self, entry, fn):
        """make one call and keep the launch count of every kernel class it used"""
        self.eng.profile_read(reset=True)
        out = fn()
        self.counts[entry] = {k: int(c) for k, (_, c) in self.eng.profile_read(reset=True).items() if c}
        return out

    def close(self):
        self.eng.profile_enable(False)
        self.eng.close()


def adam(module):
    return ra.Optimizer(module, ra.optimizer_config_default(ra.OPTIMIZER_ADAM))


def values_opt_config(target):
    cfg = ra.values_opt_config_default()
    cfg.opt_steps_per_update, cfg.target, cfg.discount_factor = 2, target, GAMMA
    return cfg


def run_module_case(name, case_type=Case):
    make, variant, host_collective, bandit = MODULE_CASES[name]
    c = case_type(variant, host_collective)
    eng = c.eng
    if bandit:
        env, A = ra.BanditEnv(eng, N, values=(0.25, -1.0, 1.5), seed_env=5, seed_actor=6), 3
    else:
        env, A = ra.CartPoleEnv(eng, N, max_steps=9, seed_env=5, seed_actor=6), 2
    c.policy, c.critic = make(eng, A), make(eng, 1)
    c.policy.init(2)
    c.critic.init(3)
    c.policy_opt, c.critic_opt = adam(c.policy), adam(c.critic)
    pol, cri, popt, copt = c.policy, c.critic, c.policy_opt, c.critic_opt
    c.traj = traj = ra.Trajectory(eng, N, T, 5)
    ra.rollout(env, pol, traj)
    rtg, td = values_opt_config(ra.VALUE_TARGET_REWARD_TO_GO), values_opt_config(ra.VALUE_TARGET_ONE_STEP_TD)
    # value fitting before any advantage pass has scanned the rewards of this rollout ...
    c.call("values_opt_update reward-to-go", lambda: ra.values_opt_update(cri, copt, traj, rtg, want_losses=True))
    c.call("values_opt_update one-step-td", lambda: ra.values_opt_update(cri, copt, traj, td, want_losses=True))
    c.call("gae", lambda: ra.gae(traj, cri, GAMMA, 0.95))
    # ... and behind one at the same discount factor
    c.call("values_opt_update reward-to-go after gae",
           lambda: ra.values_opt_update(cri, copt, traj, rtg, want_losses=True))
    c.call("values_opt_update one-step-td after gae",
           lambda: ra.values_opt_update(cri, copt, traj, td, want_losses=True))
    c.call("policy_gradient", lambda: ra.policy_gradient(pol, traj))
    v = np.linspace(-1.0, 1.0, pol.P).astype(np.float32)
    c.call("policy_fvp", lambda: ra.policy_fvp(pol, traj, v, 1e-5))
    p0 = pol.get_params()
    c.call("policy_loss_kl", lambda: ra.policy_loss_kl(pol, traj, p0))
    c.call("critic_gradient", lambda: ra.critic_gradient(cri, traj))
    c.call("critic_update", lambda: ra.critic_update(cri, copt, traj, 2, want_losses=True))
    trpo = ra.trpo_config_default()
    trpo.iterations, trpo.max_backtracks = 2, 2  # both candidates are enqueued before the first read-back
    c.call("trpo_update", lambda: ra.trpo_update(pol, traj, trpo).as_dict())
    ppo = ra.ppo_config_default()
    ppo.opt_steps_per_update = 2
    c.call("ppo_update", lambda: ra.ppo_update(pol, popt, traj, ppo, want_losses=True))
    c.call("reinforce_update", lambda: ra.reinforce_update(pol, popt, traj))

    def actor_critic():
        pst, cst, losses = ra.actor_critic_update(pol, cri, copt, traj, trpo, td, want_losses=True)
        return pst.as_dict(), cst, losses

    c.call("actor_critic_update", actor_critic)
    eng.set_serial_update(True)
    c.call("actor_critic_update serial", actor_critic)
    c.close()
    return c.counts


def run_dqn_case(name, case_type=Case):
    hidden, td, variant = DQN_CASES[name]
    c = case_type(variant)
    env = ra.CartPoleEnv(c.eng, N, max_steps=9, limit=ra.LIMIT_VISIBLE, seed_env=21, seed_actor=34)
    c.policy = q = ra.Mlp(c.eng, 5, hidden, 2)
    q.init(77)
    c.policy_opt = adam(q)
    cfg = ra.dqn_config_default()
    cfg.target = ra.DQN_TARGET_ONE_STEP_TD if td else ra.DQN_TARGET_REWARD_TO_GO
    cfg.exploration_kind, cfg.exploration_start = ra.SCHEDULE_CONSTANT, 0.3
    cfg.minibatch_steps, cfg.opt_steps_per_update, cfg.buffer_capacity, cfg.discount_factor = 200, 2, 64, GAMMA
    dqn = ra.Dqn(env, q, c.policy_opt, cfg)
    c.call("collect", lambda: dqn.collect(T))
    c.call("update", lambda: dqn.update(want_losses=True))
    dqn.close()
    c.close()
    return c.counts


def run_case(name, case_type=Case):
    return (run_module_case if name in MODULE_CASES else run_dqn_case)(name, case_type)


ALL_CASES = list(MODULE_CASES) + list(DQN_CASES)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_CASES)
def test_launch_counts(golden, name):
    got, want = run_case(name), golden[name]
    for entry in sorted(set(got) | set(want)):
        print(name, entry, got.get(entry))
    assert got == want, {e: (got.get(e), want.get(e)) for e in set(got) | set(want) if got.get(e) != want.get(e)}


def record(path):
    table = {name: run_case(name) for name in ALL_CASES}
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(table), path))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="write the table instead of checking it")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    if not args.record:
        ap.error("run under pytest to check; --record writes the table")
    record(args.out)
