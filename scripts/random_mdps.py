"""The second task of the RL^2 paper, one MDP at a time: sample a tabular MDP from DirichletRandomMdps
(ra.sample_random_mdp), solve it exactly under the step limit (finite-horizon dynamic programming in f64 NumPy), train
feed-forward TRPO on ra.TabularMdpEnv lanes and print the mean episode reward per period beside the optimal and the
uniform-random value.

  python scripts/random_mdps.py [--states 4] [--actions 3] [--limit 16] [--lanes 1024] [--periods 40] [--mdp-seed 5]
                                [--seeds 100,200,300] [--json out.json]

--json: the curves and, per seed, the first period whose mean episode reward exceeds the midpoint of the two values."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relearn_amd as ra  # noqa: E402


def finite_horizon_values(transitions, reward_mean, horizon):
    """-> (optimal, uniform-random) expected episode reward from state 0 over `horizon` steps, discount factor 1"""
    P, R = np.asarray(transitions, np.float64), np.asarray(reward_mean, np.float64)
    v_opt, v_uni = np.zeros(P.shape[0]), np.zeros(P.shape[0])
    for _ in range(horizon):
        v_opt = (R + P @ v_opt).max(axis=1)
        v_uni = (R + P @ v_uni).mean(axis=1)
    return float(v_opt[0]), float(v_uni[0])


def train(eng, tr, mean, args, seed):
    env = ra.TabularMdpEnv(eng, tr, mean, None, n_lanes=args.lanes, max_steps=args.limit, limit=ra.LIMIT_VISIBLE,
                           seed_env=seed, seed_actor=seed + 1)
    pol, cri = ra.Mlp(eng, env.D, [args.hidden], env.A), ra.Mlp(eng, env.D, [args.hidden], 1)
    pol.init(seed + 2)
    cri.init(seed + 3)
    opt = ra.Adam(cri)
    traj = ra.Trajectory(eng, args.lanes, args.limit, env.D)  # one whole episode per lane and period
    curve = []
    for _ in range(args.periods):
        ra.rollout(env, pol, traj)
        curve.append(float(traj.read(ra.TRAJ_REWARD).astype(np.float64).sum() / args.lanes))
        ra.gae(traj, cri, 1.0, 0.95)
        ra.trpo_update(pol, traj)
        ra.critic_update(cri, opt, traj, opt_steps=20)
    return curve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=4)
    ap.add_argument("--actions", type=int, default=3)
    ap.add_argument("--limit", type=int, default=16)
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--periods", type=int, default=40)
    ap.add_argument("--mdp-seed", type=int, default=5)
    ap.add_argument("--seeds", default="100,200,300")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cfg = ra.random_mdps_config_default()
    cfg.num_states, cfg.num_actions = args.states, args.actions
    tr, mean = ra.sample_random_mdp(cfg, args.mdp_seed, 0)
    optimal, uniform = finite_horizon_values(tr, mean, args.limit)
    bar = 0.5 * (optimal + uniform)
    print("MDP %d x %d (seed %d), step limit %d: optimal %.3f, uniform-random %.3f, midpoint %.3f" % (
        args.states, args.actions, args.mdp_seed, args.limit, optimal, uniform, bar))
    eng = ra.Engine(0)
    runs = []
    for seed in [int(s) for s in args.seeds.split(",")]:
        curve = train(eng, tr, mean, args, seed)
        crossed = next((i + 1 for i, c in enumerate(curve) if c > bar), None)
        print("seed %d: crosses the midpoint in period %s; %s" % (seed, crossed, " ".join("%.2f" % c for c in curve)))
        runs.append(dict(seed=seed, crossed_in_period=crossed, mean_episode_reward=curve))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(states=args.states, actions=args.actions, mdp_seed=args.mdp_seed, step_limit=args.limit,
                           lanes=args.lanes, hidden=args.hidden, optimal=optimal, uniform_random=uniform, midpoint=bar,
                           runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
