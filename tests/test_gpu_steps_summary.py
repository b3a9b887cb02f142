"""StepsSummary on the device (rl_summary_*, relearn_amd/csrc/kernels_summary.hip): OnlineStepsSummary::push per lane
(src/simulation/summary.rs:198-214) and the completed statistics (src/utils/stats.rs) against the numpy restatement, on
synthetic planes, real rollouts and a DQN collection; run-to-run determinism; the C++ train loop's logged set."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import relearn_amd as ra
from steps_summary_ref import close, episodes, mean_variance, period_summaries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("step_reward", "episode_reward", "episode_length")


def synthetic_planes(rng, n, T, periods=3):
    """rewards with +-1e6 and 0 among normal values; random flags; lanes that never end, lanes where every step ends,
    lanes whose one episode spans all pushes"""
    rewards, flags = [], []
    for p in range(periods):
        r = rng.normal(2.0, 1.0, (T, n)).astype(np.float32)
        r[rng.random((T, n)) < 0.05] = 0.0
        k = max(2, (T * n) // 1000)
        r.reshape(-1)[rng.choice(T * n, k, replace=False)] = 1e6
        r.reshape(-1)[rng.choice(T * n, k // 2, replace=False)] = -1e6
        f = np.where(rng.random((T, n)) < 0.1, rng.integers(1, 3, (T, n)), 0).astype(np.uint8)
        f[:, 0] = 0                          # never ends
        if n > 1:
            f[:, 1] = ra.SUCC_TERMINATE      # every step ends
        if n > 2:
            f[:, 2] = 0                      # one episode over all pushes, ends at the last step of the last
            if p == periods - 1:
                f[T - 1, 2] = ra.SUCC_INTERRUPT
        rewards.append(r)
        flags.append(f)
    return rewards, flags


def check(got, want):
    for f in FIELDS:
        close(getattr(got, f), want[f], f)


@pytest.mark.gpu
@pytest.mark.parametrize("n,T", [(96, 1), (96, 7), (1000, 128), (65536, 128)])
def test_synthetic_planes_match_numpy(engine, n, T):
    rng = np.random.default_rng(n * 1000 + T)
    rewards, flags = synthetic_planes(rng, n, T)
    traj = ra.Trajectory(engine, n, T, 5)
    s = ra.StepsSummary(engine, n)
    want = period_summaries(rewards, flags)
    for p in range(3):
        traj.write(ra.TRAJ_REWARD, rewards[p])
        traj.write(ra.TRAJ_FLAG, flags[p])
        s.push(traj)
        check(s.read(), want[p])
        s.clear()
    # an episode in progress is carried across clear(); clear(forget=True) drops it
    r = rng.normal(0.0, 1.0, (T, n)).astype(np.float32)
    f = np.zeros((T, n), np.uint8)
    f[0, :] = ra.SUCC_TERMINATE
    traj.write(ra.TRAJ_REWARD, r)
    traj.write(ra.TRAJ_FLAG, f)
    s.clear(forget=True)
    s.push(traj)
    got = s.read()
    assert got.episode_length.count == n and got.episode_length.mean == 1.0
    assert got.episode_length.squared_residual_sum == 0.0
    close(got.episode_reward, mean_variance(r[0].astype(np.float64)), "episode_reward")
    s.close()
    traj.close()


@pytest.mark.gpu
def test_cartpole_rollouts(engine):
    n, T = 4096, 128
    env = ra.CartPoleEnv(engine, n, max_steps=500, seed_env=5, seed_actor=6)
    pol = ra.Mlp(engine, 5, 128, 2)
    pol.init(2)
    traj = ra.Trajectory(engine, n, T, 5)
    s = ra.StepsSummary(engine, n)
    rewards, flags, reads = [], [], []
    for _ in range(3):
        ra.rollout(env, pol, traj)
        s.push(traj)
        reads.append(s.read())
        s.clear()
        rewards.append(traj.read(ra.TRAJ_REWARD))
        flags.append(traj.read(ra.TRAJ_FLAG))
    want = period_summaries(rewards, flags)
    for p, got in enumerate(reads):
        er, el = got.episode_reward, got.episode_length  # CartPole: reward 1 per step, episode reward = length
        assert (er.mean, er.squared_residual_sum, er.count) == (el.mean, el.squared_residual_sum, el.count)
        sr = got.step_reward
        assert (sr.mean, sr.squared_residual_sum, sr.count) == (1.0, 0.0, n * T) and sr.stddev() == 0.0
        assert el.count == int((flags[p] != ra.SUCC_CONTINUE).sum())
        check(got, want[p])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["chain", "memory", "bandit"])
def test_other_env_rollouts(engine, kind):
    n, T = 512, 40
    env = {"chain": lambda: ra.ChainEnv(engine, n, max_steps=30, seed_env=3, seed_actor=4),
           "memory": lambda: ra.MemoryEnv(engine, n, seed_env=3, seed_actor=4),
           "bandit": lambda: ra.BanditEnv(engine, n, values=(0.25, 1.5), seed_env=3, seed_actor=4)}[kind]()
    pol = ra.Mlp(engine, 5, 128, 2)
    pol.init(9)
    traj = ra.Trajectory(engine, n, T, 5)
    s = ra.StepsSummary(engine, n)
    rewards, flags, reads = [], [], []
    for _ in range(3):
        ra.rollout(env, pol, traj)
        s.push(traj)
        reads.append(s.read())
        s.clear()
        rewards.append(traj.read(ra.TRAJ_REWARD))
        flags.append(traj.read(ra.TRAJ_FLAG))
    want = period_summaries(rewards, flags)
    for p, got in enumerate(reads):
        check(got, want[p])
        if kind == "bandit":
            el = got.episode_length
            assert (el.mean, el.squared_residual_sum, el.count) == (1.0, 0.0, n * T) and el.stddev() == 0.0
    assert reads[-1].episode_length.count > 0


@pytest.mark.gpu
def test_dqn_collection(engine):
    n, T = 256, 60
    env = ra.CartPoleEnv(engine, n, max_steps=500, seed_env=21, seed_actor=34)
    q = ra.Mlp(engine, 5, 128, 2)
    q.init(77)
    opt = ra.Adam(q)
    cfg = ra.dqn_config_default()
    cfg.exploration_kind, cfg.exploration_start = ra.SCHEDULE_CONSTANT, 0.3
    cfg.buffer_capacity = 200
    cfg.discount_factor = 0.99
    dqn = ra.Dqn(env, q, opt, cfg)
    s = ra.StepsSummary(engine, n)
    with pytest.raises(ra.RelearnError):
        s.push_dqn(dqn)  # nothing collected yet
    rewards, flags = [], []
    for _ in range(3):
        st = dqn.collect(T)
        s.push_dqn(dqn)
        got = s.read()
        s.clear()
        assert got.step_reward.count == st.steps and got.episode_length.count == st.episodes_ended
        fl = dqn.replay_read(ra.REPLAY_LAST_FLAGS)
        total = dqn.replay_read(ra.REPLAY_TOTAL).astype(np.int64)
        ring = dqn.replay_read(ra.REPLAY_REWARD)  # [C][n]
        slots = (total[None, :] - T + np.arange(T)[:, None]) % cfg.buffer_capacity
        rw = np.take_along_axis(ring, slots, axis=0)
        rewards.append(rw)
        flags.append(fl)
        want = period_summaries(rewards, flags)[-1]
        check(got, want)
    dqn.close()


@pytest.mark.gpu
def test_deterministic_from_run_to_run(engine):
    n, T = 65536, 128
    rewards, flags = synthetic_planes(np.random.default_rng(3), n, T, periods=1)
    traj = ra.Trajectory(engine, n, T, 5)
    traj.write(ra.TRAJ_REWARD, rewards[0])
    traj.write(ra.TRAJ_FLAG, flags[0])
    a, b = ra.StepsSummary(engine, n), ra.StepsSummary(engine, n)
    a.push(traj)
    b.push(traj)
    assert bytes(a.read()) == bytes(b.read())
    a.push(traj)
    b.push(traj)
    assert bytes(a.read()) == bytes(b.read())


@pytest.mark.gpu
def test_cpp_train_loop_logs_the_reference_set(engine):
    ra.build()
    exe = os.path.join(tempfile.mkdtemp(), "steps_summary_demo")
    libdir = os.path.join(ROOT, "relearn_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", ROOT,
                           os.path.join(ROOT, "tests", "cpp", "steps_summary_demo.cpp"), "-o", exe, "-L", libdir,
                           "-lrelearn_hip", "-Wl,-rpath," + libdir])
    out = json.loads(subprocess.check_output([exe], timeout=300).decode())
    # the same run through the ctypes binding (tests/test_host_api_cpp.py's agent: build_agent(seed 2))
    env = ra.CartPoleEnv(engine, 256, max_steps=500, seed_env=0, seed_actor=1)
    pol, cri = ra.Mlp(engine, 5, 128, 2), ra.Mlp(engine, 5, 128, 1)
    pol.init(2)
    cri.init(3)
    opt = ra.Adam(cri)
    traj = ra.Trajectory(engine, 256, 32, 5)
    s = ra.StepsSummary(engine, 256)
    episodes_total = 0
    for _ in range(2):
        ra.rollout(env, pol, traj)
        s.push(traj)
        got = s.read()
        s.clear()
        episodes_total += got.episode_length.count
        ra.gae(traj, cri, 0.99, 0.95)
        ra.trpo_update(pol, traj)
        ra.critic_update(cri, opt, traj, 5)
    sc = out["scalars"]
    assert got.episode_length.count > 0
    assert sc["sim/ep/fbk/reward/mean"] == got.episode_reward.mean
    assert sc["sim/ep/fbk/reward/stddev"] == got.episode_reward.stddev()
    assert sc["sim/ep/length_mean"] == got.episode_length.mean
    assert sc["sim/ep/length_stddev"] == got.episode_length.stddev()
    assert sc["sim/step/fbk/reward/mean"] == got.step_reward.mean == 1.0
    assert sc["sim/step/fbk/reward/stddev"] == got.step_reward.stddev() == 0.0
    assert out["counters"] == {"agent_update/count": 2, "sim/ep/count": episodes_total, "sim/step/count": 2 * 256 * 32}
    assert set(out["durations"]) == {"adv_est_time", "agent_update/time", "critic/update_time", "policy/update_time",
                                     "sim/time"}
    assert out["display"].split("\n") == [
        "step_feedback: (μ = 1.000; σ = 0.000; n = 8)",
        "episode_feedback: (μ = 2.500; σ = 0.500; n = 4)",
        "episode_length: (μ = 2.500; σ = 0.500; n = 4)",
        "step_feedback: (μ = -; σ = -; n = 0)",
        "episode_feedback: (μ = -; σ = -; n = 0)",
        "episode_length: (μ = -; σ = -; n = 0)"]
