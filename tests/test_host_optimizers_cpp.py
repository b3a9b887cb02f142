"""The host API's optimiser configurations (relearn_amd/csrc/host/agents.hpp): SgdConfig, RmsPropConfig and AdamWConfig
beside AdamConfig, as the second template parameter `OC` of ValuesOptConfig, PpoConfig, ReinforceConfig and DqnConfig.  A
small client (tests/cpp/host_optimizers_demo.cpp) builds an actor-critic agent whose critic steps with SGD and a DQN
agent that steps with RMSProp, runs one period each and exits 0; static assertions in it hold the defaulted OC to
AdamConfig.  Compile step as in tests/test_host_api_cpp.py."""
import json
import os
import subprocess
import tempfile

import pytest

import relearn_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "host_optimizers_demo.cpp")


def build_demo():
    ra.build()
    out = os.path.join(tempfile.mkdtemp(), "host_optimizers_demo")
    libdir = os.path.join(ROOT, "relearn_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", ROOT, SRC, "-o", out,
                           "-L", libdir, "-lrelearn_hip", "-Wl,-rpath," + libdir])
    return out


def test_cpp_optimizer_configs_compile_and_link():
    assert os.path.exists(build_demo())


@pytest.mark.gpu
def test_cpp_agents_with_sgd_and_rmsprop_run_a_period(engine):
    out = subprocess.run([build_demo()], timeout=300, capture_output=True)
    assert out.returncode == 0, out.stderr.decode()
    r = json.loads(out.stdout.decode())
    assert r["critic_moved"] > 0 and r["ppo_moved"] > 0 and r["q_moved"] > 0
