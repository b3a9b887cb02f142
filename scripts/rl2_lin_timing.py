"""Timing of the RL² bandit experiment's update (scripts/rl2_bandits.py's `linear` model: GRU(128) -> ReLU -> Linear as
policy and critic, arms + 4 features) under the two engine kernel variants — 0: the training passes on the tile kernels
with the head in kernels_seq_lin.hip (PASS_PATH_RECURRENT_TILE); 1: the lane-per-thread kernels, the path before.  One
process, host clock around synchronised calls, the variants alternated period by period, the median of `--repeats`.

Per variant: the period's update (rl_gae + rl_trpo_update + rl_values_opt_update), its TRPO and critic shares, and the four
single calls rl_policy_gradient, rl_policy_fvp, rl_policy_loss_kl, rl_critic_gradient.  One JSON line.

    python scripts/rl2_lin_timing.py [--lanes 1024] [--arms 10] [--episodes 10] [--trials 2] [--repeats 10] [--critic-steps 50]
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
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--arms", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--trials", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--critic-steps", type=int, default=50)
    a = ap.parse_args()
    horizon = a.trials * (2 * a.episodes - 1)
    eng = ra.Engine(0)
    env = ra.MetaBanditEnvWide(eng, a.lanes, a.arms, a.episodes, "uniform_bernoulli", seed_env=0, seed_actor=1)
    pol = ra.RnnChainWide(eng, "gru", env.D, 128, a.arms)
    cri = ra.RnnChainWide(eng, "gru", env.D, 128, 1)
    pol.init(2), cri.init(3)
    p0, c0 = pol.get_params(), cri.get_params()
    traj = ra.Trajectory(eng, a.lanes, horizon, env.D)
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
    print(json.dumps({"device": name, "arch": arch, "lanes": a.lanes, "arms": a.arms, "horizon": horizon,
                      "critic_steps": a.critic_steps, "repeats": a.repeats, "pass_path": paths,
                      "median_ms": {str(vv): {k: float(np.median(x)) for k, x in times[vv].items()} for vv in times},
                      "min_max_ms": {str(vv): {k: [float(min(x)), float(max(x))] for k, x in times[vv].items()} for vv in times},
                      "how": "time.perf_counter around synchronised calls; one process; variants alternated per period"}))


if __name__ == "__main__":
    main()
