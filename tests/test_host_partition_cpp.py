"""tests/cpp/partition_demo.cpp: the partition-game experiment's agent through the C++ host API (PartitionGameLanes,
GruMlpConfig, ActorCriticAgent, DeviceHistory of relearn_amd/csrc/host/agents.hpp; the scalar env PartitionGame of
host/envs.hpp) under a VisibleStepLimit of 3 steps: 24 observation features.  At this size the host mirror goes through
rl_env_create_partition, rl_rnn_chain_create_wide24 (policy 24 -> 2, critic 24 -> 1) and rl_traj_create_wide24: a wrong
threshold is a refusal by an older entry point and the demo's exit code 1.  CPU: the demo compiles and links against the
library.  GPU: inside the demo the scalar env on the streams of lanes 0 and 63 equals the lanes step for step (it exits
with a code of its own otherwise); its driven steps, and two periods of rollout, GAE with a recurrent critic and
batch_update, leave what the same work leaves through the ctypes binding (ra.PartitionEnv, ra.RnnChainWide24,
ra.TrajectoryWide24) — exactly."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import relearn_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "partition_demo.cpp")


def checksum(p):
    """the demo's sum, term after term in its order"""
    s = 0.0
    for i, x in enumerate(np.asarray(p).ravel().tolist()):
        s += float(x) * float(1 + i % 7)
    return s


def build_demo():
    ra.build()
    out = os.path.join(tempfile.mkdtemp(), "partition_demo")
    libdir = os.path.join(ROOT, "relearn_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", ROOT, SRC,
                           "-o", out, "-L", libdir, "-lrelearn_hip", "-Wl,-rpath," + libdir])
    return out


def test_partition_demo_compiles_and_links():
    assert os.path.exists(build_demo())


@pytest.mark.gpu
def test_partition_demo_matches_the_ctypes_path(engine):
    exe = build_demo()
    proc = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert proc.returncode == 0, (proc.returncode, proc.stderr.decode()[-2000:])
    out = json.loads(proc.stdout.decode())
    print(out)
    n, L, T, H, periods, A = 64, 3, 7, 16, 2, 2
    make = lambda: ra.PartitionEnv(engine, n, max_steps=L, limit=ra.LIMIT_VISIBLE, seed_env=91, seed_actor=92)
    env = make()
    assert (env.D, env.A) == (24, 2)
    rewards, obs = [], []
    for t in range(8):
        r, _, o, _ = env.step(((t + np.arange(n)) % 2).astype(np.uint8))
        rewards.append(r), obs.append(o)
    assert out["driven_rewards_checksum"] == checksum(np.array(rewards)) and out["driven_obs_checksum"] == checksum(np.array(obs))
    env = make()
    pol = ra.RnnChainWide24(engine, "gru", env.D, H, A, mlp_hidden=H)
    cri = ra.RnnChainWide24(engine, "gru", env.D, H, 1, mlp_hidden=H)
    rnn = 3 * H * env.D + 3 * H * H + 6 * H
    assert (out["policy_params"], out["critic_params"]) == (pol.P, cri.P) == (rnn + H * H + H + A * H + A, rnn + H * H + H + H + 1)
    pol.init(93)
    cri.init(94)
    opt = ra.Adam(cri)
    ccfg = ra.values_opt_config_default()  # discount factor min(the env's 0.999, max_discount_factor 0.99)
    ccfg.opt_steps_per_update = 5
    traj = ra.TrajectoryWide24(engine, n, T, env.D)
    episodes, actions = 0, set()
    for _ in range(periods):
        ra.rollout(env, pol, traj)
        ended = int((traj.read(ra.TRAJ_FLAG) != 0).sum())  # (episodes of 3 steps in periods of 7)
        episodes += ended
        actions |= set(np.unique(traj.read(ra.TRAJ_ACTION)))
        ra.gae(traj, cri, 0.99, 0.95)
        st, cs = ra.actor_critic_update(pol, cri, opt, traj, None, ccfg)
    assert episodes == n * ((periods * T) // L) and actions == {0, 1}
    assert out["policy_checksum"] == checksum(pol.get_params()) and out["critic_checksum"] == checksum(cri.get_params())
    assert out["status"] == st.status
    assert out["counters"] == {"agent_update/count": periods, "sim/ep/count": episodes, "sim/step/count": periods * n * T}
    want = {"policy/entropy": st.entropy, "policy/step_size": st.step_size, "policy/loss_initial": st.loss_initial,
            "policy/loss_final": st.loss_final, "policy/constraint_val_final": st.constraint_val_final,
            "critic/loss": cs.loss_last, "sim/ep/length_mean": float(n * T) / ended}  # (of the last period: steps / episode ends)
    got = dict(out["scalars"])
    if st.num_backtracks >= 0:
        want.update({"policy/num_backtracks": float(st.num_backtracks), "policy/step_scale": st.step_scale})
    else:  # (the logger keeps a name's last value: these two may be the first period's)
        got.pop("policy/num_backtracks", None), got.pop("policy/step_scale", None)
    assert got == want
    assert np.isfinite(list(want.values())).all() and st.step_size > 0  # (an update that moved the policy)
