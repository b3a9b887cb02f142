"""Times of the meta-MDP lanes at the reference's size, 10 states x 5 actions (rl_env_create_meta_mdp_wide), for DESIGN's
record, and of the older recurrent rollouts that must not move:

  rl_env_step_resident and rl_env_reset per call at 16,384 lanes, 10 x 5 (a reset draws 550 variates per lane and writes
      50 rows of sixteen floats)
  one rollout of 4,096 lanes x one trial (T = 109 at L = E = 10), GRU(128) -> Relu -> Linear, 19 inputs: all steps in one
      launch (kernel variant 0) against the launch sequence per step (variant 1), alternated
  the share of the one-launch rollout that the trial's table draw takes: the same launch on lanes whose trial is longer
      than the horizon (E = 11), every run started at a trial's start
  the first rollout of the process (it pays for loading the code object), apart
  --older: instead of all that, the two-arm meta-bandit rollout (4,096 lanes x T = 39, GRU 128, MLP and Linear tail) and
      the 5 x 5 meta-MDP rollout (4,096 x 109, GRU 128 Linear) through the OLDER entry points — the figures a library
      from before this size existed can be asked for too (RELEARN_LIB selects the library)

  python scripts/meta_mdp_wide_timing.py [--older] [--json out.json]"""
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


def timed_rollouts(eng, env, pol, traj, variants, reps=7, warm=2):
    times = {v: [] for v in variants}
    first = None
    for rep in range(reps):
        for variant in variants:
            eng.set_kernel_variant(variant)
            env.reset()  # every run starts at a trial's start
            eng.sync()
            t0 = time.perf_counter()
            ra.rollout(env, pol, traj)
            eng.sync()
            dt = (time.perf_counter() - t0) * 1e3
            if first is None:
                first = dt
            if rep >= warm:
                times[variant].append(dt)
    eng.set_kernel_variant(0)
    return times, first


def older(eng, res):
    n, H = 4096, 128
    for name, tail in (("two_arm_mlp_tail", H), ("two_arm_linear_tail", None)):
        env = ra.MetaBanditEnv(eng, n, 2, 10)
        pol = ra.RnnChain(eng, "gru", env.D, H, 2, mlp_hidden=tail)
        pol.init(1)
        traj = ra.Trajectory(eng, n, 39, env.D)
        times, first = timed_rollouts(eng, env, pol, traj, (0,))
        res["%s_4096x39_ms" % name] = times[0]
        res.setdefault("first_rollout_of_the_process_ms", first)
    env = ra.MetaMdpEnv(eng, n, 5, 5, max_inner_steps=10, episodes_per_trial=10)
    pol = ra.RnnChainWide(eng, "gru", env.D, H, env.A)
    pol.init(1)
    traj = ra.Trajectory(eng, n, 109, env.D)
    times, _ = timed_rollouts(eng, env, pol, traj, (0, 1))
    res["meta_mdp_5x5_4096x109_one_launch_ms"], res["meta_mdp_5x5_4096x109_per_step_ms"] = times[0], times[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--lanes", type=int, default=16384)
    ap.add_argument("--older", action="store_true")
    args = ap.parse_args()
    eng = ra.Engine(0)
    res = {"library": os.path.basename(os.path.dirname(ra.LIB_PATH)) + "/" + os.path.basename(ra.LIB_PATH)}
    if args.older:
        older(eng, res)
    else:
        S, A, n, H = 10, 5, 4096, 128
        rollouts = {}
        for name, E in (("trial_ends_in_the_launch", 10), ("no_trial_ends", 11)):
            env = ra.MetaMdpEnvWide(eng, n, S, A, max_inner_steps=10, episodes_per_trial=E)
            pol = ra.RnnChainWide20(eng, "gru", env.D, H, env.A)
            pol.init(1)
            traj = ra.TrajectoryWide(eng, n, 109, env.D)
            times, first = timed_rollouts(eng, env, pol, traj, (0, 1) if E == 10 else (0,))
            res.setdefault("first_rollout_of_the_process_ms", first)
            rollouts[name] = times
            resets = int((traj.read(ra.TRAJ_FLAG) == 2).sum())
            assert resets == (n if E == 10 else 0), resets
        res["rollout_10x5_4096x109_gru128_linear_one_launch_ms"] = rollouts["trial_ends_in_the_launch"][0]
        res["rollout_10x5_4096x109_gru128_linear_per_step_ms"] = rollouts["trial_ends_in_the_launch"][1]
        res["rollout_10x5_4096x109_gru128_linear_one_launch_no_reset_ms"] = rollouts["no_trial_ends"][0]
        a, b = np.median(rollouts["trial_ends_in_the_launch"][0]), np.median(rollouts["no_trial_ends"][0])
        res["reset_share_of_one_launch_rollout"] = float((a - b) / a)
        r = np.random.RandomState(0)
        # (trials far longer than the timed steps: no step of the window resets a lane)
        env = ra.MetaMdpEnvWide(eng, args.lanes, S, A, max_inner_steps=1000, episodes_per_trial=1000)
        env.upload_actions(r.randint(0, A, args.lanes).astype(np.uint8))
        res["lanes"] = args.lanes
        res["10x5_step_resident_us"] = per_call_us(eng, env.step_resident)
        res["10x5_reset_us"] = per_call_us(eng, env.reset, calls=20, warm=3)
    for k, v in res.items():
        print(k, v if not isinstance(v, list) else " ".join("%.3f" % x for x in v), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
