"""The second task of the RL^2 paper, random tabular MDPs, on the meta-MDP lanes:
`MetaEnv::new(DirichletRandomMdps{..}.wrap(LatentStepLimit::new(inner))).wrap(TrialEpisodeLimit::new(episodes))`
(ra.MetaMdpEnvWide: every lane draws its own MDP at each trial's start; up to 10 states, `--states 10 --actions 5` is the
reference's default size), a GRU chain as policy and one as critic — GRU(hidden)
-> Relu -> Linear (`linear`, the experiment's model) or with an MLP tail of one hidden layer (`mlp`) — TRPO at max KL
0.01, the critic fitted with Adam steps per period, GAE with lambda 0.3, discount factor 0.99.  Every lane collects whole
trials per period (horizon = trials_per_lane * (episodes * (inner + 1) - 1)).

Per period one JSON line: the mean trial reward (from the device-side StepsSummary: an episode of the summary is a
trial), and beside it, over the tables read back from the lanes at the period's end — the MDPs of the trials the lanes
are in — the mean over lanes of the uniform-random policy's expected trial reward and of each lane's optimal
finite-horizon value, by f64 dynamic programming over `inner` steps from state 0, `episodes` times (the restart steps earn
nothing), as scripts/random_mdps.py solves one MDP.  The optimum is that of an agent that KNOWS its MDP: a meta-learner
that has to find it out within the trial stays below it.

    python scripts/rl2_mdps.py [--lanes 1024] [--states 5] [--actions 5] [--inner 10] [--episodes 10] [--periods 20]
        [--trials-per-lane 1] [--hidden 128] [--critic-steps 50] [--model linear] [--alpha 1] [--reward-stddev 1]
        [--seed 0] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relearn_amd as ra  # noqa: E402


def lane_values(cum, mean, inner, episodes):
    """cum [n][S][A][S] f32 running sums, mean [n][S][A] f64 -> per lane (optimal, uniform-random) expected trial reward"""
    P = np.diff(np.concatenate([np.zeros(cum.shape[:3] + (1,)), cum.astype(np.float64)], axis=3), axis=3)
    v_opt = np.zeros(cum.shape[:2])
    v_uni = np.zeros(cum.shape[:2])
    for _ in range(inner):
        v_opt = (mean + np.einsum("nsaj,nj->nsa", P, v_opt)).max(axis=2)
        v_uni = (mean + np.einsum("nsaj,nj->nsa", P, v_uni)).mean(axis=2)
    return episodes * v_opt[:, 0], episodes * v_uni[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--states", type=int, default=5)
    ap.add_argument("--actions", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--periods", type=int, default=20)
    ap.add_argument("--trials-per-lane", type=int, default=1)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--critic-steps", type=int, default=50)
    ap.add_argument("--model", choices=("linear", "mlp"), default="linear")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--prior-mean", type=float, default=1.0)
    ap.add_argument("--prior-stddev", type=float, default=1.0)
    ap.add_argument("--reward-stddev", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, help="also write all lines to this file as one JSON list")
    a = ap.parse_args()

    eng = ra.Engine(0)
    # (MetaMdpEnvWide: up to 10 states and 20 features — `--states 10 --actions 5` is DirichletRandomMdps::default — and
    # MetaMdpEnv's own handle inside that one's range; likewise the chains and the trajectory)
    env = ra.MetaMdpEnvWide(eng, a.lanes, a.states, a.actions, max_inner_steps=a.inner, episodes_per_trial=a.episodes,
                            alpha=a.alpha, reward_prior_mean=a.prior_mean, reward_prior_stddev=a.prior_stddev,
                            reward_stddev=a.reward_stddev, seed_env=a.seed, seed_actor=a.seed + 1)
    T = a.trials_per_lane * env.trial_steps
    tail = a.hidden if a.model == "mlp" else None
    pol = ra.RnnChainWide20(eng, "gru", env.D, a.hidden, env.A, mlp_hidden=tail)
    cri = ra.RnnChainWide20(eng, "gru", env.D, a.hidden, 1, mlp_hidden=tail)
    pol.init(a.seed + 2)  # input weights Uniform(FanAvg), hidden weights Orthogonal, biases Zeros; LinearConfig::default
    cri.init(a.seed + 3)
    opt = ra.Adam(cri)
    trpo = ra.trpo_config_default()
    trpo.max_policy_step_kl = 0.01
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = a.critic_steps
    ccfg.discount_factor = 0.99
    traj = ra.TrajectoryWide(eng, a.lanes, T, env.D)
    summary = ra.StepsSummary(eng, a.lanes)
    lines = []
    for period in range(a.periods):
        # the MDPs of the trials this period collects first (with whole trials per period: of its first trial)
        opt_v, uni_v = lane_values(*env.read_tables(), a.inner, a.episodes)
        eng.sync()
        t0 = time.perf_counter()
        ra.rollout(env, pol, traj)
        eng.sync()
        t1 = time.perf_counter()
        ra.gae(traj, cri, 0.99, 0.3)
        pst, cst = ra.actor_critic_update(pol, cri, opt, traj, trpo, ccfg)
        eng.sync()
        t2 = time.perf_counter()
        summary.clear()
        summary.push(traj)
        s = summary.read()
        line = {"period": period, "lanes": a.lanes, "states": a.states, "actions": a.actions, "inner_steps": a.inner,
                "episodes_per_trial": a.episodes, "horizon": T, "model": a.model, "hidden": a.hidden,
                "trials": s.episode_reward.count, "mean_trial_reward": s.episode_reward.mean,
                "trial_reward_stddev": s.episode_reward.stddev(),
                "uniform_random_trial_reward": float(uni_v.mean()), "optimal_trial_value": float(opt_v.mean()),
                "trpo_status": pst.status, "kl": pst.constraint_val_final, "entropy": pst.entropy,
                "critic_loss": [cst.loss_first, cst.loss_last],
                "rollout_ms": (t1 - t0) * 1e3, "update_ms": (t2 - t1) * 1e3}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
