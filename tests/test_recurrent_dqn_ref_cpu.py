"""tests/recurrent_dqn_ref.py — the restated DqnActor over a sequence module and its targets — checked on the CPU, and
the cases of tests/test_gpu_recurrent_dqn.py shown to be able to fail a wrong kernel.  CPU only.

(a) at eps = 0 every step is greedy and the lane's state has seen the lane's whole history: the restated actor's
    Q-values are the teacher-forced forward's over the recorded trajectory, bit for bit (this pins the restatement's
    "list of seen observations" against the oracle's own state carrying and episode restarts);
(b) for every eps = 0.5 case the GPU test runs, the right actor (an exploring step holds the state) and the wrong one (it
    advances the state) choose a different greedy action on at least one step of the right actor's own trajectory — up
    to that step the two see the same lanes, so a kernel that advances the state on exploring steps records another
    action there and fails the GPU test's comparison.  The bandit's one-step episodes cannot tell them apart under any
    seed (recurrent_dqn_ref.COLLECT_CASES): there the two are asserted equal instead;
(c) no greedy step of those cases has Q0 == Q1: the first-maximal-index rule never decides, nothing has to be left out."""
import numpy as np
import pytest

import oracle as O
import recurrent_dqn_ref as R


def run(case, eps, hold=True):
    env, mod, seed = case
    sim_of, D, _ = R.ENVS[env]
    m = R.MODULES[mod]
    params = R.module_params(m, D, seed)
    actor = R.RecurrentActor(m, D, params, R.N_LANES, R.SEEDS["seed_actor"], hold=hold)
    sim = sim_of(R.N_LANES)
    R.warm_up(env, sim)
    return m, D, params, [R.closed_loop(actor, sim, T, eps) for T in R.HORIZONS]


@pytest.mark.parametrize("case", R.COLLECT_CASES, ids=R.case_id)
def test_greedy_actor_is_the_teacher_forced_forward(case):
    m, D, params, collections = run(case, 0.0)
    shape, _, full, _ = R.embedded(m, D, params)
    for steps in collections:
        T, n = len(steps), R.N_LANES
        obs = np.zeros((D, T + 1, n), dtype=np.float32)
        for t, s in enumerate(steps):
            obs[:, t, :] = s["obs"]
            assert not s["explore"].any()
        traj = dict(obs=obs, flag=np.array([s["env_flag"] for s in steps], dtype=np.uint8),
                    term_obs=np.zeros((D, T, n), dtype=np.float32))
        out, _ = O.stack_seq_forward(shape, m.L, full, traj, want_succ=False)
        for t, s in enumerate(steps):
            assert np.array_equal(out[:, t, :], s["q"]), t
            assert np.array_equal(s["q"], s["q_other"])  # nothing was explored: both actors have seen every step
        assert (traj["flag"] != O.CONTINUE).any()


@pytest.mark.parametrize("case", R.COLLECT_CASES, ids=R.case_id)
def test_cases_separate_holding_from_stepping(case):
    _, _, _, collections = run(case, 0.5)
    differ = greedy = 0
    for steps in collections:
        for s in steps:
            g = ~s["explore"]
            greedy += int(g.sum())
            a = s["q"][1, g] > s["q"][0, g]
            b = s["q_other"][1, g] > s["q_other"][0, g]
            differ += int((a != b).sum())
            assert not (s["q"][0, g] == s["q"][1, g]).any()  # (c)
            if case[0] == "bandit":
                assert np.array_equal(s["q"][:, g], s["q_other"][:, g])
    assert greedy > 0.3 * R.N_LANES * sum(R.HORIZONS)
    if case[0] != "bandit":
        assert differ > 0, "change the case's seed: the wrong actor is not told apart"


@pytest.mark.parametrize("case", R.COLLECT_CASES, ids=R.case_id)
def test_no_greedy_tie_at_eps_0(case):
    _, _, _, collections = run(case, 0.0)
    for steps in collections:
        for s in steps:
            assert not (s["q"][0] == s["q"][1]).any()  # (c)


def test_targets_restatement():
    """the f32 targets on a hand-made episode: reward-to-go by hand; one-step TD against the f64 forward"""
    from oracle import stacked as S
    m = R.MODULES["gru-5-mlp-6"]
    D = 5
    params = R.module_params(m, D, 3)
    shape, spec, full, _ = R.embedded(m, D, params)
    rng = np.random.default_rng(1)
    for last in (O.TERMINATE, O.INTERRUPT):
        n_steps = 4
        obs = rng.normal(size=(n_steps, D)).astype(np.float32)
        succ = rng.normal(size=(n_steps, D)).astype(np.float32)
        reward = rng.normal(size=n_steps).astype(np.float32)
        flags = np.array([0, 0, 0, last], dtype=np.uint8)
        rtg = R.episode_targets(shape, m.L, full, obs, reward, flags, succ, 0.5, td=False)
        want = [reward[3]]
        for j in (2, 1, 0):
            want.insert(0, np.float32(reward[j] + np.float32(want[0] * np.float32(0.5))))
        assert np.array_equal(rtg, np.array(want, dtype=np.float32))
        td = R.episode_targets(shape, m.L, full, obs, reward, flags, succ, 0.5, td=True)
        traj = dict(obs=np.concatenate([obs.T[:, :, None], np.zeros((D, 1, 1))], axis=1), flag=flags[:, None],
                    term_obs=succ.T[:, :, None])
        q, qs, _ = S.forward(spec, full, traj)
        v = [q[:, j + 1, 0].max() for j in range(3)] + [0.0 if last == O.TERMINATE else qs[:, 3, 0].max()]
        assert np.allclose(td, reward + 0.5 * np.array(v), rtol=1e-5, atol=1e-6)
        assert (td[3] == reward[3]) == (last == O.TERMINATE)
