"""A recurrent policy learns to use a trial's history on the meta-MDP lanes, against a bar derived from the env.

S = A = 2, one inner step per inner episode (L = 1), five inner episodes per trial (E = 5), reward stddev 0, reward means
N(1, 1): every inner episode is one step from state 0, so a trial is five pulls of a two-armed bandit whose arms pay their
N(1, 1) means exactly.  Any policy that ignores the trial's history earns 5 x 1 = 5.0 per trial.  Trying both actions and
then keeping the better one earns 2 + 3 E[max(m0, m1)] = 2 + 3 (1 + 1 / sqrt(pi)) = 6.69.  The bar is their midpoint,
5.85, on 4,096 fresh evaluation trials (an env of its own seed, never trained on).

GRU(32) -> Relu -> Linear policy and critic, TRPO at max KL 0.01, 20 Adam critic steps, GAE lambda 0.3, 4,096 lanes x one
trial per period.  Measured on the device (profiles/meta_mdp_learning.json): seeds 0, 10 and 20 are all past the bar at the
first evaluation, after 10 periods (6.80, 6.68, 6.77), and stay between 6.7 and 7.1 for 400 periods; the test runs 20
periods, twice that.  Fails on a library without the constructor."""
import numpy as np
import pytest

import relearn_amd as ra

pytestmark = pytest.mark.gpu
BAR = 0.5 * (5.0 + 2.0 + 3.0 * (1.0 + 1.0 / np.sqrt(np.pi)))
PERIODS = 20


@pytest.mark.parametrize("seed", [0, 10, 20])
def test_a_gru_policy_learns_to_use_the_trial(engine, seed):
    assert abs(BAR - 5.85) < 0.005
    make = lambda n, s: ra.MetaMdpEnv(engine, n, 2, 2, max_inner_steps=1, episodes_per_trial=5, reward_stddev=0.0,
                                      seed_env=s, seed_actor=s + 1)
    env, fresh = make(4096, seed), make(4096, seed + 1000)
    assert env.trial_steps == 9
    pol, cri = ra.RnnChainWide(engine, "gru", env.D, 32, 2), ra.RnnChainWide(engine, "gru", env.D, 32, 1)
    pol.init(seed + 2), cri.init(seed + 3)
    opt = ra.Adam(cri)
    trpo = ra.trpo_config_default()
    trpo.max_policy_step_kl = 0.01
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update, ccfg.discount_factor = 20, 0.99
    traj, held = ra.Trajectory(engine, 4096, 9, env.D), ra.Trajectory(engine, 4096, 9, env.D)
    summary = ra.StepsSummary(engine, 4096)

    def evaluate():
        ra.rollout(fresh, pol, held)  # whole trials: the evaluation lanes draw new MDPs at every call
        summary.clear()
        summary.push(held)
        s = summary.read()
        assert s.episode_reward.count == 4096
        return s.episode_reward.mean

    before = evaluate()
    for _ in range(PERIODS):
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.3)
        ra.actor_critic_update(pol, cri, opt, traj, trpo, ccfg)
    after = evaluate()
    print("seed %d: mean trial reward on fresh trials %.3f before, %.3f after %d periods (bar %.3f)" % (
        seed, before, after, PERIODS, BAR))
    assert before < BAR < after
