"""tests/cpp/dqn_k_bandit_demo.cpp: the reference's DQN acceptance test (src/agents/testing.rs:14-64,
train_deterministic_bandit) at four arms over the C++ host API — DqnConfig<MlpConfig, AdamConfig> over hidden_sizes
[16, 16] builds through rl_dqn_create_finite on an env of more than two actions.  CPU: the demo compiles and links against
the library.  GPU: it pulls the best arm in at least 900 of 1,000 greedy evaluation steps, and its trained parameters are
those of the same run through the ctypes binding (tests/test_gpu_finite_dqn.py::train_k_bandit)."""
import json
import os
import subprocess
import tempfile

import pytest

import relearn_amd as ra
from test_host_api_cpp import checksum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dqn_k_bandit_demo.cpp")


def build_demo():
    ra.build()
    out = os.path.join(tempfile.mkdtemp(), "dqn_k_bandit_demo")
    libdir = os.path.join(ROOT, "relearn_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", ROOT, SRC, "-o", out,
                           "-L", libdir, "-lrelearn_hip", "-Wl,-rpath," + libdir])
    return out


def test_dqn_k_bandit_demo_compiles_and_links():
    assert os.path.exists(build_demo())


@pytest.mark.gpu
@pytest.mark.parametrize("target", ["rtg", "td"], ids=["reward-to-go", "one-step-td"])
def test_dqn_k_bandit_demo_learns_and_matches_the_ctypes_path(engine, target):
    from test_gpu_finite_dqn import train_k_bandit
    exe = build_demo()
    out = json.loads(subprocess.check_output([exe, target], timeout=120).decode())
    print(out)
    assert out["target"] == target and out["arms"] == 4 and out["steps"] == 1000 and out["best"] >= 900
    q, best = train_k_bandit(engine, "4-arms", "16x16", target == "td")
    assert out["checksum"] == checksum(q.get_params())
    assert out["best"] == best
