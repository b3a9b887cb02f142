"""tests/cpp/rl2_wide_demo.cpp: the RL2 experiment at ten arms through the C++ host API (MetaBanditLanes — through
rl_env_create_meta_bandit_wide above four arms — GruLinearConfig — through rl_rnn_chain_create_wide above eight inputs or
outputs — ActorCriticAgent of relearn_amd/csrc/host/agents.hpp).  CPU: the demo compiles and links against the library.  GPU: two periods of rollout,
GAE with a recurrent critic and batch_update (TRPO + critic fitting) leave the parameters, counters and logged scalars of
the same two periods driven through the ctypes binding — exactly."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import relearn_amd as ra
from test_host_api_cpp import checksum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rl2_wide_demo.cpp")


def build_demo():
    ra.build()
    out = os.path.join(tempfile.mkdtemp(), "rl2_wide_demo")
    libdir = os.path.join(ROOT, "relearn_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", ROOT, SRC, "-o", out,
                           "-L", libdir, "-lrelearn_hip", "-Wl,-rpath," + libdir])
    return out


def test_rl2_wide_demo_compiles_and_links():
    assert os.path.exists(build_demo())


@pytest.mark.gpu
def test_rl2_wide_demo_matches_the_ctypes_path(engine):
    exe = build_demo()
    out = json.loads(subprocess.check_output([exe], timeout=120).decode())
    print(out)
    n, E, T, H, periods, arms = 64, 3, 10, 16, 2, 10
    env = ra.MetaBanditEnvWide(engine, n, arms, E, "uniform_bernoulli", seed_env=71, seed_actor=72)
    assert (env.D, env.A) == (14, 10)
    pol, cri = ra.RnnChainWide(engine, "gru", env.D, H, arms), ra.RnnChainWide(engine, "gru", env.D, H, 1)
    rnn = 3 * H * env.D + 3 * H * H + 6 * H
    assert (out["policy_params"], out["critic_params"]) == (pol.P, cri.P) == (rnn + arms * H + arms, rnn + H + 1)
    pol.init(73)
    cri.init(74)
    opt = ra.Adam(cri)
    ccfg = ra.values_opt_config_default()  # discount factor min(the env's 1.0, max_discount_factor 0.99)
    ccfg.opt_steps_per_update = 5
    traj = ra.Trajectory(engine, n, T, env.D)
    episodes, actions = 0, set()
    for _ in range(periods):
        ra.rollout(env, pol, traj)
        episodes += int((traj.read(ra.TRAJ_FLAG) != 0).sum())
        actions |= set(np.unique(traj.read(ra.TRAJ_ACTION)))
        ra.gae(traj, cri, 0.99, 0.3)
        st, cs = ra.actor_critic_update(pol, cri, opt, traj, None, ccfg)
    assert episodes == periods * n * (T // (2 * E - 1)) and actions == set(range(arms))
    assert out["policy_checksum"] == checksum(pol.get_params()) and out["critic_checksum"] == checksum(cri.get_params())
    assert out["status"] == st.status
    assert out["counters"] == {"agent_update/count": periods, "sim/ep/count": episodes, "sim/step/count": periods * n * T}
    want = {"policy/entropy": st.entropy, "policy/step_size": st.step_size, "policy/loss_initial": st.loss_initial,
            "policy/loss_final": st.loss_final, "policy/constraint_val_final": st.constraint_val_final,
            "critic/loss": cs.loss_last, "sim/ep/length_mean": float(2 * E - 1)}
    got = dict(out["scalars"])
    if st.num_backtracks >= 0:
        want.update({"policy/num_backtracks": float(st.num_backtracks), "policy/step_scale": st.step_scale})
    else:  # (the logger keeps a name's last value: these two may be the first period's)
        got.pop("policy/num_backtracks", None), got.pop("policy/step_scale", None)
    assert got == want
    assert np.isfinite(list(want.values())).all() and st.step_size > 0  # (an update that moved the policy)
