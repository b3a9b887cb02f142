"""Time per rl_env_step_resident at 16,384 lanes on tabular-MDP (8, 8) lanes beside MemoryGame(4, 4) lanes (the two kinds
share the launch: k_env_step<Env, 8>), and one feed-forward rollout period on the MDP lanes.

  python scripts/tabular_mdp_timing.py [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relearn_amd as ra  # noqa: E402


def per_call_us(eng, f, calls=200, repeats=5):
    for _ in range(20):
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
    n = args.lanes
    r = np.random.RandomState(0)
    tr = r.dirichlet(np.ones(8), size=(8, 8)).astype(np.float32)
    mean = r.normal(size=(8, 8))
    res = {"lanes": n}
    for name, stddev in (("mdp_8x8_noisy", None), ("mdp_8x8_stddev0", np.zeros((8, 8)))):
        env = ra.TabularMdpEnv(eng, tr, mean, stddev, n_lanes=n, max_steps=100, limit=ra.LIMIT_LATENT)
        env.upload_actions(r.randint(0, 8, n).astype(np.uint8))
        res[name + "_step_resident_us"] = per_call_us(eng, env.step_resident)
        env.close()
    mem = ra.MemoryEnv(eng, n, 4, 4)
    mem.upload_actions(r.randint(0, 4, n).astype(np.uint8))
    res["memory_4_4_step_resident_us"] = per_call_us(eng, mem.step_resident)
    # one feed-forward rollout period: 8 x 8 under a visible limit is refused (9 features); 7 x 8 is the widest
    tr7 = r.dirichlet(np.ones(7), size=(7, 8)).astype(np.float32)
    env = ra.TabularMdpEnv(eng, tr7, r.normal(size=(7, 8)), None, n_lanes=n, max_steps=16, limit=ra.LIMIT_VISIBLE)
    pol = ra.Mlp(eng, env.D, [16], env.A)
    pol.init(1)
    traj = ra.Trajectory(eng, n, 16, env.D)
    res["rollout_7x8_T16_mlp16_ms"] = [x / 1e3 for x in per_call_us(eng, lambda: ra.rollout(env, pol, traj), calls=10)]
    for k, v in res.items():
        print(k, v if not isinstance(v, list) else " ".join("%.2f" % x for x in v))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
