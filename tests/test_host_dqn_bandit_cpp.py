"""tests/cpp/dqn_bandit_demo.cpp: the reference's DQN acceptance test (src/torch/agents/tests/dqn.rs,
testing::train_deterministic_bandit) over the C++ host API.  CPU: the demo compiles and links against the library.
GPU: it pulls arm 1 in at least 900 of 1,000 greedy evaluation steps, and its trained parameters are those of the same
run through the ctypes binding (tests/test_gpu_dqn_index_envs.py::train_deterministic_bandit)."""
import json
import os
import subprocess
import tempfile

import pytest

import relearn_amd as ra
from test_host_api_cpp import checksum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dqn_bandit_demo.cpp")


def build_demo():
    ra.build()
    out = os.path.join(tempfile.mkdtemp(), "dqn_bandit_demo")
    libdir = os.path.join(ROOT, "relearn_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", ROOT, SRC, "-o", out,
                           "-L", libdir, "-lrelearn_hip", "-Wl,-rpath," + libdir])
    return out


def test_dqn_bandit_demo_compiles_and_links():
    assert os.path.exists(build_demo())


@pytest.mark.gpu
@pytest.mark.parametrize("n_lanes", [10, 2], ids=["10-lanes-x-1-step", "2-lanes-x-5-steps"])
def test_dqn_bandit_demo_learns_and_matches_the_ctypes_path(engine, n_lanes):
    from test_gpu_dqn_index_envs import greedy_evaluation, train_deterministic_bandit
    exe = build_demo()
    out = json.loads(subprocess.check_output([exe, str(n_lanes)], timeout=120).decode())
    print(out)
    assert out["lanes"] == n_lanes and out["steps"] == 1000 and out["arm1"] >= 900
    env, q, dqn = train_deterministic_bandit(engine, n_lanes, [128])
    assert out["checksum"] == checksum(q.get_params())
    assert out["arm1"] == greedy_evaluation(env, q)
