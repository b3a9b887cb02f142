"""tests/cpp/dqn_gru_bandit_demo.cpp: the reference's GRU acceptance test of DQN (src/torch/agents/tests/dqn.rs,
default_gru_mlp_learns_derministic_bandit) over the C++ host API — DqnConfig<GruMlpConfig, AdamConfig> builds through
rl_dqn_create_recurrent.  CPU: the demo compiles and links against the library.  GPU: it pulls arm 1 in at least 900 of
1,000 greedy evaluation steps, and its trained parameters are those of the same run through the ctypes binding
(tests/test_gpu_recurrent_dqn.py::train_deterministic_bandit)."""
import json
import os
import subprocess
import tempfile

import pytest

import relearn_amd as ra
from test_host_api_cpp import checksum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dqn_gru_bandit_demo.cpp")


def build_demo():
    ra.build()
    out = os.path.join(tempfile.mkdtemp(), "dqn_gru_bandit_demo")
    libdir = os.path.join(ROOT, "relearn_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", ROOT, SRC, "-o", out,
                           "-L", libdir, "-lrelearn_hip", "-Wl,-rpath," + libdir])
    return out


def test_dqn_gru_bandit_demo_compiles_and_links():
    assert os.path.exists(build_demo())


@pytest.mark.gpu
@pytest.mark.parametrize("target", ["rtg", "td"], ids=["reward-to-go", "one-step-td"])
def test_dqn_gru_bandit_demo_learns_and_matches_the_ctypes_path(engine, target):
    from test_gpu_recurrent_dqn import train_deterministic_bandit
    exe = build_demo()
    out = json.loads(subprocess.check_output([exe, target], timeout=120).decode())
    print(out)
    assert out["target"] == target and out["steps"] == 1000 and out["arm1"] >= 900
    q, ones = train_deterministic_bandit(engine, "gru-mlp-default", target == "td")
    assert out["checksum"] == checksum(q.get_params())
    assert out["arm1"] == ones
