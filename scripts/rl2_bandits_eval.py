"""The `eval` half of the reference's RL^2 bandit experiment (relearn_experiments/src/bin/rl2-bandits.rs:166-261) on the
meta-bandit lanes: a classical bandit algorithm, wrapped in a ResettingMetaAgent that builds a fresh inner agent per
trial, over `MetaEnv::new(D::new(arms)).wrap(TrialEpisodeLimit::new(episodes))` for `trials` trials — one lane per trial,
one collection of 2 * episodes - 1 steps.  `agent` is one of the experiment's AgentType values the library builds:
random, eps_greedy (tabular Q-learning 0.2, 2, 0.5), greedy (0.0, 2, 0.5), ucb1 (0.2), ts (Beta Thompson sampling,
num_samples 1), ots (num_samples 10) — all six of the experiment's; 2..12 arms (the reference's default is ten;
ra.MetaBanditEnvWide).  The summary is the device-side StepsSummary, of which an
episode is a trial.  Prints one JSON line with the reference's EvalResults: trial_reward_mean, trial_reward_stddev.

    python scripts/rl2_bandits_eval.py [agent] [arms] [episodes] [trials] [distribution]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relearn_amd as ra  # noqa: E402

AGENTS = {"random": ("random", {}), "eps_greedy": ("tabular_q", dict(exploration_rate=0.2, initial_action_count=2,
                                                                   initial_action_value=0.5)),
          "greedy": ("tabular_q", dict(exploration_rate=0.0, initial_action_count=2, initial_action_value=0.5)),
          "ucb1": ("ucb1", dict(exploration_rate=0.2)), "ts": ("thompson", dict(num_samples=1)),
          "ots": ("thompson", dict(num_samples=10))}

arg = lambda i, d: type(d)(sys.argv[i]) if len(sys.argv) > i else d
name, arms, E, trials, dist = arg(1, "ucb1"), arg(2, 2), arg(3, 10), arg(4, 1000), arg(5, "uniform_bernoulli")
if name not in AGENTS:
    sys.exit("agent must be one of %s" % sorted(AGENTS))
kind, params = AGENTS[name]
T = 2 * E - 1

eng = ra.Engine(0)
env = ra.MetaBanditEnvWide(eng, trials, arms, E, dist, seed_env=0, seed_actor=1)
agent = ra.BanditAgent(env, kind, **params)
traj = ra.Trajectory(eng, trials, T, env.D)
summary = ra.StepsSummary(eng, trials)
eng.sync()
t0 = time.perf_counter()
agent.rollout(env, traj)
eng.sync()
t1 = time.perf_counter()
summary.push(traj)
s = summary.read()
print(json.dumps({"agent": name, "num_arms": arms, "num_episodes": E, "num_trials": s.episode_reward.count,
                  "distribution": dist, "trial_reward_mean": s.episode_reward.mean,
                  "trial_reward_stddev": s.episode_reward.stddev(), "mean_step_reward": s.step_reward.mean,
                  "rollout_ms": (t1 - t0) * 1e3}), flush=True)
