"""tests/cpp/thompson_agents_demo.cpp: the Thompson-sampling baselines through the C++ host API (MetaBanditLanes,
ResettingMetaAgent over BetaThompsonSamplingAgentConfig, StepsSummaryLanes of relearn_amd/csrc/host/agents.hpp).  CPU: the
demo compiles and links against the library.  GPU: two collections per agent leave the planes, the counts, the word
positions and the summary of the same two collections through the ctypes binding — exactly."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import relearn_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "thompson_agents_demo.cpp")


def build_demo():
    ra.build()
    out = os.path.join(tempfile.mkdtemp(), "thompson_agents_demo")
    libdir = os.path.join(ROOT, "relearn_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", ROOT, SRC, "-o", out,
                           "-L", libdir, "-lrelearn_hip", "-Wl,-rpath," + libdir])
    return out


def checksum(p):
    """the demo's: a sequential f64 sum, element i weighted 1 + i mod 7"""
    s = 0.0
    for i, v in enumerate(np.asarray(p).reshape(-1).tolist()):
        s += float(v) * float(1 + i % 7)
    return s


def test_thompson_agents_demo_compiles_and_links():
    assert os.path.exists(build_demo())


@pytest.mark.gpu
def test_thompson_agents_demo_matches_the_ctypes_path(engine):
    exe = build_demo()
    out = json.loads(subprocess.check_output([exe], timeout=120).decode())
    n, k, E, T = 70, 3, 4, 10
    specs = [("ts", 1), ("ots", 10)]
    assert [o["agent"] for o in out] == [s[0] for s in specs]
    for o, (name, num_samples) in zip(out, specs):
        env = ra.MetaBanditEnv(engine, n, k, E, seed_env=71, seed_actor=72)
        agent = ra.BanditAgent(env, "thompson", num_samples=num_samples)
        traj = ra.Trajectory(engine, n, T, env.D)
        summary = ra.StepsSummary(engine, n)
        for period in range(2):
            agent.rollout(env, traj)
            summary.push(traj)
            got = traj.read_all()
            assert o["collections"][period] == {key: checksum(got[key]) for key in ("obs", "action", "reward", "flag")}, (
                name, period)
        st = agent.state()
        assert o["pos"] == checksum(st["pos"]) and o["low"] == checksum(st["low"]) and o["high"] == checksum(st["high"]), name
        stats = summary.read()
        assert o["trials"] == stats.episode_reward.count == 2 * n  # 20 steps hold two whole trials of 7
        assert o["trial_reward_mean"] == stats.episode_reward.mean
        assert o["trial_reward_stddev"] == stats.episode_reward.stddev()
    # the agents differ (the demo ran what it says): OTS draws ten times the samples
    assert out[1]["pos"] > 9 * out[0]["pos"] > 0
    assert out[0]["collections"] != out[1]["collections"]
