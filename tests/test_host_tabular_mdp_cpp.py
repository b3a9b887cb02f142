"""tests/cpp/tabular_mdp_demo.cpp: tabular-MDP lanes through the C++ host API (DirichletRandomMdps, TabularMdp of
host/envs.hpp; TabularMdpLanes, MlpConfig, ActorCriticAgent of host/agents.hpp).  CPU: the demo compiles and links against
the library; the samplers of include/rl_normal.h and the host sampler run under AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program (tests/cpp/tabular_mdp_sanitize_main.cpp).  GPU: the sampled tables,
the scalar env on lane 0's stream and two periods of rollout, GAE and batch_update leave what the same work leaves through
the ctypes binding — exactly."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import relearn_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tabular_mdp_demo.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


def checksum(p):
    """the demo's sum, term after term in its order"""
    s = 0.0
    for i, x in enumerate(np.asarray(p).ravel().tolist()):
        s += float(x) * float(1 + i % 7)
    return s


def build_demo():
    ra.build()
    out = os.path.join(tempfile.mkdtemp(), "tabular_mdp_demo")
    libdir = os.path.join(ROOT, "relearn_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", ROOT, SRC,
                           "-o", out, "-L", libdir, "-lrelearn_hip", "-Wl,-rpath," + libdir])
    return out


def test_tabular_mdp_demo_compiles_and_links():
    assert os.path.exists(build_demo())


def test_samplers_under_asan_and_ubsan():
    """a plain C++ program with its own main: no runtime is preloaded, leak checking on"""
    exe = os.path.join(tempfile.mkdtemp(prefix="relearn_san_"), "tabular_mdp_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", ROOT, "-I", os.path.join(ROOT, "include")]
                          + SAN + [os.path.join(ROOT, "tests", "cpp", "tabular_mdp_sanitize_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([exe], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=200)
    out = proc.stdout.decode()
    assert proc.returncode == 0 and "tabular mdp sanitize ok" in out, out[-4000:]
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out and "runtime error:" not in out, out[-4000:]


@pytest.mark.gpu
def test_tabular_mdp_demo_matches_the_ctypes_path(engine):
    exe = build_demo()
    out = json.loads(subprocess.check_output([exe], timeout=120).decode())
    print(out)
    n, limit, periods = 64, 8, 2
    cfg = ra.random_mdps_config_default()
    cfg.num_states, cfg.num_actions = 4, 3
    tr, mean = ra.sample_random_mdp(cfg, 5, 0)
    assert out["transitions_checksum"] == checksum(tr) and out["reward_mean_checksum"] == checksum(mean)
    # the scalar mirror against lane 0 of a limit-free handle
    one = ra.TabularMdpEnv(engine, tr, mean, None, n_lanes=1, seed_env=61, seed_actor=62)
    rewards, states = [], []
    for t in range(20):
        reward, _, obs, _ = one.step(np.array([t % 3], np.uint8))
        rewards.append(reward[0])
        states.append(float(obs[:, 0].argmax()))
    assert out["scalar_rewards_checksum"] == checksum(np.array(rewards, np.float32))
    assert out["scalar_states_checksum"] == checksum(states)
    # two periods through the binding
    env = ra.TabularMdpEnv(engine, tr, mean, None, n_lanes=n, max_steps=limit, limit=ra.LIMIT_VISIBLE, seed_env=61,
                           seed_actor=62)
    assert (env.D, env.A) == (5, 3)
    pol, cri = ra.Mlp(engine, env.D, [16], 3), ra.Mlp(engine, env.D, [16], 1)
    pol.init(63)
    cri.init(64)
    opt = ra.Adam(cri)
    ccfg = ra.values_opt_config_default()  # discount factor min(the env's 1.0, max_discount_factor 0.99)
    ccfg.opt_steps_per_update = 5
    traj = ra.Trajectory(engine, n, limit, env.D)
    for _ in range(periods):
        ra.rollout(env, pol, traj)
        assert int((traj.read(ra.TRAJ_FLAG) != 0).sum()) == n  # one whole episode per lane
        ra.gae(traj, cri, 0.99, 0.95)
        st, cs = ra.actor_critic_update(pol, cri, opt, traj, None, ccfg)
    assert out["policy_checksum"] == checksum(pol.get_params()) and out["critic_checksum"] == checksum(cri.get_params())
    assert out["status"] == st.status
    assert out["counters"] == {"agent_update/count": periods, "sim/ep/count": periods * n, "sim/step/count": periods * n * limit}
    got = dict(out["scalars"])
    assert got["policy/entropy"] == st.entropy and got["policy/loss_final"] == st.loss_final
    assert got["critic/loss"] == cs.loss_last and got["sim/ep/length_mean"] == float(limit)
    assert np.isfinite(list(got.values())).all() and st.step_size > 0
