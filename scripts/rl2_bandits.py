"""The reference's RL^2 bandit experiment (relearn_experiments/src/bin/rl2-bandits.rs:379-425) on the meta-bandit lanes:
`MetaEnv::new(UniformBernoulliBandits::new(arms)).wrap(TrialEpisodeLimit::new(episodes))`, TRPO at max KL 0.01, the
critic fitted with 50 Adam steps per period, GAE with lambda 0.3, discount factor 0.99.  Policy and critic are one
recurrent chain each, chosen by `model`:
    linear  the experiment's own `type Model = Chain<Gru, Linear>` (rl2-bandits.rs:349): GRU(128) -> Relu ->
            Linear(128, out), ra.GruLinear
    mlp     (the default) GRU(128) -> Relu -> Linear(128, 128) -> Relu -> Linear(128, out), ra.GruMlp: the chain with
            an MLP tail, one hidden layer more than the experiment's model
`arms` is 2 (the default) .. 12 (the experiment's own default is 10): two arms build the two-action constructors'
modules, three and more the same chains with one output per arm through ra.RnnChainWide (rl_rnn_chain_create_wide; up to
four arms and eight features that is rl_rnn_chain_create), on ra.MetaBanditEnvWide lanes.  Every lane collects whole
trials per period (horizon = trials_per_lane * (2 * episodes - 1)); the mean trial reward of a period comes from the
device-side StepsSummary (an episode of the summary is a trial).  Prints one JSON line per period.

    python scripts/rl2_bandits.py [lanes] [episodes] [periods] [trials_per_lane] [distribution] [hidden] \\
        [critic_steps] [model] [arms]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relearn_amd as ra  # noqa: E402

arg = lambda i, d: type(d)(sys.argv[i]) if len(sys.argv) > i else d
N, E, periods, trials = arg(1, 1024), arg(2, 10), arg(3, 20), arg(4, 2)
dist, H, critic_steps = arg(5, "uniform_bernoulli"), arg(6, 128), arg(7, 50)
model = arg(8, "mlp")
arms = arg(9, 2)
assert model in ("mlp", "linear"), "model: mlp | linear"
assert 2 <= arms <= 12, "arms: 2..12"
T = trials * (2 * E - 1)

eng = ra.Engine(0)
env = ra.MetaBanditEnvWide(eng, N, arms, E, dist, seed_env=0, seed_actor=1)
if model == "linear":
    pol = ra.GruLinear(eng, env.D, 2, H) if arms == 2 else ra.RnnChainWide(eng, "gru", env.D, H, arms)
    cri = ra.GruLinear(eng, env.D, 1, H) if env.D <= 8 else ra.RnnChainWide(eng, "gru", env.D, H, 1)
    glorot = ("Uniform", "FanAvg", 0.0)
    gru_config = (glorot, ("Orthogonal", "FanAvg", 0.0), ("Zeros", "FanAvg", 0.0))
    pol.init_with(2, *gru_config, glorot, glorot)  # the experiment's GruConfig, LinearConfig::default
    cri.init_with(3, *gru_config, glorot, glorot)
else:
    pol = ra.GruMlp(eng, env.D, 2, H, H) if arms == 2 else ra.RnnChainWide(eng, "gru", env.D, H, arms, mlp_hidden=H)
    cri = ra.GruMlp(eng, env.D, 1, H, H) if env.D <= 8 else ra.RnnChainWide(eng, "gru", env.D, H, 1, mlp_hidden=H)
    pol.init(2)  # input weights Uniform(FanAvg), hidden weights Orthogonal, biases Zeros: the experiment's GruConfig
    cri.init(3)
opt = ra.Adam(cri)
trpo = ra.trpo_config_default()
trpo.max_policy_step_kl = 0.01
ccfg = ra.values_opt_config_default()
ccfg.opt_steps_per_update = critic_steps
ccfg.discount_factor = 0.99
traj = ra.Trajectory(eng, N, T, env.D)
summary = ra.StepsSummary(eng, N)

for period in range(periods):
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
    # ("model" only for `linear`, "arms" only above two: the default's lines stay what they were before the arguments
    # existed, byte for byte)
    print(json.dumps({**({"model": model} if model == "linear" else {}), **({"arms": arms} if arms != 2 else {}),
                      "period": period, "lanes": N, "episodes_per_trial": E, "horizon": T, "distribution": dist,
                      "trials": s.episode_reward.count, "mean_trial_reward": s.episode_reward.mean,
                      "trial_reward_stddev": s.episode_reward.stddev(), "mean_step_reward": s.step_reward.mean,
                      "trpo_status": pst.status, "kl": pst.constraint_val_final, "entropy": pst.entropy,
                      "critic_loss": [cst.loss_first, cst.loss_last],
                      "rollout_ms": (t1 - t0) * 1e3, "update_ms": (t2 - t1) * 1e3}), flush=True)
