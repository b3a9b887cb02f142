"""Times of the meta-MDP lanes (rl_env_create_meta_mdp) for DESIGN's record:

  rl_env_step_resident and rl_env_reset per call at 16,384 lanes, for 5 x 5 and 8 x 4 (a reset draws S A (S + 1)
      variates per lane and writes the lane's tables)
  one rollout of 4,096 lanes x one trial (T = 109 at the default L = E = 10), GRU(128) -> Relu -> Linear: all steps in
      one launch (kernel variant 0) against the launch sequence per step (variant 1), alternated
  the share of the one-launch rollout that the trial's table draw takes: the same launch on lanes whose trial is longer
      than the horizon (E = 11: no lane ends a trial in it), every run started at a trial's start

  python scripts/meta_mdp_timing.py [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relearn_amd as ra  # noqa: E402


def per_call_us(eng, f, calls=200, repeats=5, warm=20):
    for _ in range(warm):
        f()
    eng.sync()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        eng.sync()
        out.append((time.perf_counter() - t0) / calls * 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--lanes", type=int, default=16384)
    args = ap.parse_args()
    eng = ra.Engine(0)
    res = {"lanes": args.lanes}
    r = np.random.RandomState(0)
    for S, A in ((5, 5), (8, 4)):
        # (trials far longer than the timed steps: no step of the window resets a lane)
        env = ra.MetaMdpEnv(eng, args.lanes, S, A, max_inner_steps=1000, episodes_per_trial=1000)
        env.upload_actions(r.randint(0, A, args.lanes).astype(np.uint8))
        res["%dx%d_step_resident_us" % (S, A)] = per_call_us(eng, env.step_resident)
        res["%dx%d_reset_us" % (S, A)] = per_call_us(eng, env.reset, calls=50, warm=5)
        env.close()
    n, H = 4096, 128
    rollouts = {}
    for name, E in (("trial_ends_in_the_launch", 10), ("no_trial_ends", 11)):
        env = ra.MetaMdpEnv(eng, n, 5, 5, max_inner_steps=10, episodes_per_trial=E)
        T = 10 * 11 - 1
        pol = ra.RnnChainWide(eng, "gru", env.D, H, env.A)
        pol.init(1)
        traj = ra.Trajectory(eng, n, T, env.D)
        times = {0: [], 1: []}
        for rep in range(7):
            for variant in (0, 1) if E == 10 else (0,):
                eng.set_kernel_variant(variant)
                env.reset()  # every run starts at a trial's start
                eng.sync()
                t0 = time.perf_counter()
                ra.rollout(env, pol, traj)
                eng.sync()
                if rep >= 2:  # (two warm-up runs per variant)
                    times[variant].append((time.perf_counter() - t0) * 1e3)
        eng.set_kernel_variant(0)
        rollouts[name] = times
        resets = int((traj.read(ra.TRAJ_FLAG) == 2).sum())
        assert resets == (n if E == 10 else 0), resets
    res["rollout_4096x109_gru128_linear_one_launch_ms"] = rollouts["trial_ends_in_the_launch"][0]
    res["rollout_4096x109_gru128_linear_per_step_ms"] = rollouts["trial_ends_in_the_launch"][1]
    res["rollout_4096x109_gru128_linear_one_launch_no_reset_ms"] = rollouts["no_trial_ends"][0]
    a, b = np.median(res["rollout_4096x109_gru128_linear_one_launch_ms"]), np.median(rollouts["no_trial_ends"][0])
    res["reset_share_of_one_launch_rollout"] = float((a - b) / a)
    for k, v in res.items():
        print(k, v if not isinstance(v, list) else " ".join("%.3f" % x for x in v))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
