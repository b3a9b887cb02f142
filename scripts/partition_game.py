"""The partition-game experiment (relearn_experiments/src/bin/partition-game.rs) on the PartitionGame lanes:
`PartitionGame::default().wrap(VisibleStepLimit::new(1000))` (ra.PartitionEnv: 24 observation features, two actions) under
`ActorCriticConfig<TrpoConfig<GruMlpConfig>, ValuesOptConfig<GruMlpConfig>>::default()` — GRU(128) -> ReLU -> MLP([128])
as policy (two outputs) and as critic (one), TRPO at its default max KL, the critic fitted with 80 Adam steps per period on
reward-to-go targets, GAE with lambda 0.95, discount factor min(0.999, 0.99) — on `--lanes` lanes of `--horizon` steps per
period (the reference collects at least 5,000 steps per worker thread; 256 lanes x 128 steps are 32,768).

Per period one JSON line: the device-side StepsSummary of the period (src/simulation/summary.rs) — mean step reward, and the
episodes that ended in it with their mean reward and length — the update's statistics and the wall-clock times of the
rollout and of the update.  A uniform-random policy's expected step reward is 0 by construction (either label is as
likely as the other, whatever the axis); +1 is a policy that has found the axis, which takes the feedback of several steps.

    python scripts/partition_game.py [--lanes 256] [--horizon 128] [--periods 20] [--max-steps 1000] [--hidden 128]
        [--critic-steps 80] [--seed 0] [--json out.json] [--timing-json out.json]
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
    ap.add_argument("--lanes", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--periods", type=int, default=20)
    ap.add_argument("--max-steps", type=int, default=1000, help="VisibleStepLimit::new(max_steps)")
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--critic-steps", type=int, default=80)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, help="also write all lines to this file as one JSON list")
    ap.add_argument("--timing-json", default=None, help="write the per-period times and their medians to this file")
    a = ap.parse_args()

    eng = ra.Engine(0)
    env = ra.PartitionEnv(eng, a.lanes, max_steps=a.max_steps, limit=ra.LIMIT_VISIBLE, seed_env=a.seed, seed_actor=a.seed + 1)
    pol = ra.RnnChainWide24(eng, "gru", env.D, a.hidden, env.A, mlp_hidden=a.hidden)
    cri = ra.RnnChainWide24(eng, "gru", env.D, a.hidden, 1, mlp_hidden=a.hidden)
    pol.init(a.seed + 2)  # input weights Uniform(FanAvg), hidden weights Orthogonal, biases Zeros; LinearConfig::default
    cri.init(a.seed + 3)
    opt = ra.Adam(cri)
    trpo = ra.trpo_config_default()
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = a.critic_steps
    gamma = min(ra.PartitionEnv.DISCOUNT_FACTOR, 0.99)  # max_discount_factor.min(env discount) (critics/opt.rs:73)
    ccfg.discount_factor = gamma
    traj = ra.TrajectoryWide24(eng, a.lanes, a.horizon, env.D)
    summary = ra.StepsSummary(eng, a.lanes)
    lines = []
    for period in range(a.periods):
        eng.sync()
        t0 = time.perf_counter()
        ra.rollout(env, pol, traj)
        eng.sync()
        t1 = time.perf_counter()
        ra.gae(traj, cri, gamma, 0.95)
        pst, cst = ra.actor_critic_update(pol, cri, opt, traj, trpo, ccfg)
        eng.sync()
        t2 = time.perf_counter()
        summary.clear()
        summary.push(traj)
        s = summary.read()
        line = {"period": period, "lanes": a.lanes, "horizon": a.horizon, "max_steps": a.max_steps, "hidden": a.hidden,
                "steps": s.step_reward.count, "mean_step_reward": s.step_reward.mean,
                "uniform_random_step_reward": 0.0,
                "episodes": s.episode_reward.count,
                "mean_episode_reward": s.episode_reward.mean if s.episode_reward.count else None,
                "mean_episode_length": s.episode_length.mean if s.episode_length.count else None,
                "trpo_status": pst.status, "kl": pst.constraint_val_final, "entropy": pst.entropy,
                "critic_loss": [cst.loss_first, cst.loss_last],
                "rollout_ms": (t1 - t0) * 1e3, "update_ms": (t2 - t1) * 1e3}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.json:
        with open(a.json, "w") as f:  # one period per line
            f.write("[\n" + ",\n".join(json.dumps(l) for l in lines) + "\n]\n")
    if a.timing_json:
        name, arch, cus = eng.info()
        warm = lines[1:] if len(lines) > 1 else lines  # (the first period pays for the first launches)
        with open(a.timing_json, "w") as f:
            json.dump({"device": name, "arch": arch, "lanes": a.lanes, "horizon": a.horizon, "hidden": a.hidden,
                       "critic_steps": a.critic_steps, "periods": a.periods,
                       "rollout_ms": [l["rollout_ms"] for l in lines], "update_ms": [l["update_ms"] for l in lines],
                       "rollout_ms_median_after_first": float(np.median([l["rollout_ms"] for l in warm])),
                       "update_ms_median_after_first": float(np.median([l["update_ms"] for l in warm])),
                       "how": "time.perf_counter around rl_rollout and around rl_gae + rl_actor_critic_update, the engine "
                              "synchronised before and after each; one process, one run"}, f)


if __name__ == "__main__":
    main()
