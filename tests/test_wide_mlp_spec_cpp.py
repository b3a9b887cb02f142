"""wide_mlp_shape and rl_rollout's path for a wide module (relearn_amd/csrc/handle_spec.hpp) on the CPU, through
tests/cpp/wide_mlp_spec_demo.cpp, built plainly with -Wall -Wextra -Werror: the shape and parameter count of accepted
modules, the older constructors' answers inside their range, every refusal with code and words."""
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID_ARGUMENT, BUILD_AGENT, UNSUPPORTED = 1, 4, 10


@pytest.fixture(scope="module")
def demo():
    exe = os.path.join(tempfile.mkdtemp(prefix="relearn_wide_mlp_spec_"), "demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.dirname(HERE),
                           os.path.join(HERE, "cpp", "wide_mlp_spec_demo.cpp"), "-o", exe])
    out = {}
    for line in subprocess.check_output([exe], timeout=60).decode().splitlines():
        fields, message = line.split(" |")
        name, *numbers = fields.split()
        out[name] = (tuple(int(v) for v in numbers), message.strip())
    return out


@pytest.mark.parametrize("name,want", [
    # (code, in, out, P, general, wide, has_bias)
    ("policy_24", (0, 24, 2, 24 * 128 + 128 + 2 * 128 + 2, 1, 1, 1)),
    ("critic_23_two_layers", (0, 23, 1, 23 * 33 + 33 + 33 * 64 + 64 + 64 + 1, 1, 1, 1)),
    ("nobias_9_no_hidden", (0, 9, 2, 18, 1, 1, 0)),
    ("fused_5", (0, 5, 2, 5 * 128 + 128 + 2 * 128 + 2, 0, 0, 1)),  # inside the older range: the older modules
    ("general_8", (0, 8, 3, 8 * 16 + 16 + 3 * 16 + 3, 1, 0, 1)),
])
def test_accepted_shapes(demo, name, want):
    assert demo[name] == (want, "")


@pytest.mark.parametrize("name,code,words", [
    ("in_25", BUILD_AGENT, "rl_mlp_create_wide: in_dim 1..24"), ("in_0", BUILD_AGENT, "supported MLP shapes: in_dim 1..8"),
    ("out_3_at_24", UNSUPPORTED, "rl_mlp_create_wide: "), ("out_0_at_24", BUILD_AGENT, "rl_mlp_create_wide: "),
    ("out_9_at_24", BUILD_AGENT, "rl_mlp_create_wide: "), ("width_257_at_9", BUILD_AGENT, "rl_mlp_create_wide: "),
    ("four_layers_at_9", BUILD_AGENT, "rl_mlp_create_wide: "), ("activation_4_at_9", BUILD_AGENT, "activation"),
    ("wide_on_partition_23", INVALID_ARGUMENT, "does not match the env"),
    ("narrow_on_partition", UNSUPPORTED, "rl_rollout: feed-forward modules are not built for RL_ENV_PARTITION"),
    ("wide_on_meta_mdp", UNSUPPORTED, "rl_rollout: a module of rl_mlp_create_wide"),
])
def test_refusals(demo, name, code, words):
    assert demo[name][0][0] == code and words in demo[name][1], demo[name]


def test_rollout_takes_a_wide_module_on_partition_lanes_as_the_general_path(demo):
    (code, path, general, *_), _ = demo["wide_on_partition"]
    assert code == 0 and path == general
