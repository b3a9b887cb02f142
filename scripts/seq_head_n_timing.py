"""Timing of the update of a GRU(128) -> ReLU -> MLP([128]) chain policy over `--outputs` actions with its one-output critic
under the two engine kernel variants — 0: the update passes on the tile kernels (PASS_PATH_RECURRENT_TILE; 3 to 12
outputs: the head of kernels_seq_head_n.hip); 1: the lane-per-thread kernels, the path of such a policy before.  The
method of scripts/partition_gru_timing.py: one process, host clock around synchronised calls, the variants alternated
period by period on the same models and the same trajectory, the median of `--repeats` with min and max.

`--env mdp`: RL² random-MDP lanes (S states x A actions, S + A + 4 features), one rollout per period.  `--env written`: a
host-written trajectory of `--features` inputs (no lanes of 24 features have more than two actions), an episode end every
32 steps, staggered across lanes.

Per variant: the period's update (rl_gae + rl_trpo_update + rl_values_opt_update), its shares, and the four single calls
rl_policy_gradient, rl_policy_fvp, rl_policy_loss_kl, rl_critic_gradient.  One JSON line.

    python scripts/seq_head_n_timing.py --env mdp --lanes 1024 --horizon 38 --outputs 5 --critic-steps 50
    python scripts/seq_head_n_timing.py --env written --features 24 --lanes 256 --horizon 128 --outputs 12 --critic-steps 80
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relearn_amd as ra  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", choices=["mdp", "written"], default="mdp")
    ap.add_argument("--states", type=int, default=10)
    ap.add_argument("--features", type=int, default=24)
    ap.add_argument("--outputs", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=38)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--critic-steps", type=int, default=50)
    a = ap.parse_args()
    eng = ra.Engine(0)
    A = a.outputs
    if a.env == "mdp":
        env = ra.MetaMdpEnvWide(eng, a.lanes, a.states, A, seed_env=0, seed_actor=1)
        D = env.D
    else:
        env, D = None, a.features
    pol = ra.RnnChainWide24(eng, "gru", D, 128, A, mlp_hidden=128)
    cri = ra.RnnChainWide24(eng, "gru", D, 128, 1, mlp_hidden=128)
    pol.init(2), cri.init(3)
    p0, c0 = pol.get_params(), cri.get_params()
    traj = ra.TrajectoryWide24(eng, a.lanes, a.horizon, D)
    if env is None:
        rng = np.random.default_rng(0)
        n, T = a.lanes, a.horizon
        step, lane = np.arange(T)[:, None], np.arange(n)[None, :]
        traj.write_all({"obs": rng.normal(size=(D, T + 1, n)).astype(np.float32),
                        "action": rng.integers(0, A, size=(T, n)).astype(np.uint8),
                        "reward": rng.normal(size=(T, n)).astype(np.float32),
                        "flag": ((step + lane) % 32 == 31).astype(np.uint8),
                        "term_obs": rng.normal(size=(D, T, n)).astype(np.float32)})
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = a.critic_steps
    ccfg.discount_factor = 0.99
    v = np.linspace(-1.0, 1.0, pol.P).astype(np.float32)

    def timed(fn):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    times, paths = {0: {}, 1: {}}, {}
    for rep in range(a.repeats + 1):  # (the first round pays for the first launches and is dropped)
        if env is not None:
            ra.rollout(env, pol, traj)
        for variant in ((0, 1) if rep % 2 == 0 else (1, 0)):
            eng.set_kernel_variant(variant)
            pol.set_params(p0), cri.set_params(c0)  # both variants update the same models on the same trajectory
            opt = ra.Adam(cri)
            t = {"gae": timed(lambda: ra.gae(traj, cri, 0.99, 0.3)),
                 "trpo": timed(lambda: ra.trpo_update(pol, traj)),
                 "critic": timed(lambda: ra.values_opt_update(cri, opt, traj, ccfg))}
            t["period"] = t["gae"] + t["trpo"] + t["critic"]
            pol.set_params(p0), cri.set_params(c0)
            t["rl_policy_gradient"] = timed(lambda: ra.policy_gradient(pol, traj))
            paths[variant] = traj.last_pass_path()
            t["rl_policy_fvp"] = timed(lambda: ra.policy_fvp(pol, traj, v, 1e-5))
            t["rl_policy_loss_kl"] = timed(lambda: ra.policy_loss_kl(pol, traj, p0))
            t["rl_critic_gradient"] = timed(lambda: ra.critic_gradient(cri, traj))
            if rep > 0:
                for k, ms in t.items():
                    times[variant].setdefault(k, []).append(ms)
        eng.set_kernel_variant(0)
    name, arch, cus = eng.info()
    print(json.dumps({"device": name, "arch": arch, "env": a.env, "features": D, "outputs": A, "lanes": a.lanes,
                      "horizon": a.horizon, "critic_steps": a.critic_steps, "repeats": a.repeats, "pass_path": paths,
                      "median_ms": {str(vv): {k: float(np.median(x)) for k, x in times[vv].items()} for vv in times},
                      "min_max_ms": {str(vv): {k: [float(min(x)), float(max(x))] for k, x in times[vv].items()} for vv in times},
                      "how": "time.perf_counter around synchronised calls; one process; variants alternated per period"}))


if __name__ == "__main__":
    main()
