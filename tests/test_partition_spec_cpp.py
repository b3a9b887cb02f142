"""The HIP-free side of the PartitionGame lanes on the CPU (tests/cpp/partition_spec_demo.cpp, which includes
relearn_amd/csrc/handle_spec.hpp alone): env_spec_partition's D, A and constants under each limit kind; every refusal with
code and words, and the order of the refusals; the older constructors' answer to the new kind; rl_rnn_chain_create_wide24's
routing and refusals; the trajectory constructors' plane bounds; rl_rollout's path for these lanes and its refusal of
feed-forward modules by name; and the scalar env PartitionGame of host/envs.hpp against tests/partition_ref.py.  Built twice:
plainly with -Wall -Wextra -Werror, and with -fsanitize=address,undefined as an executable of its own."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import partition_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLAGS = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", ROOT]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
INVALID_ARGUMENT, BUILD_AGENT, BUILD_ENV, UNSUPPORTED = 1, 4, 5, 10
ENV_PARTITION = 7


@pytest.fixture(scope="module")
def workdir():
    return tempfile.mkdtemp(prefix="relearn_partition_spec_")


def build_and_run(workdir, name, extra, env=None):
    exe = os.path.join(workdir, name)
    subprocess.check_call(FLAGS + extra + [os.path.join(HERE, "cpp", "partition_spec_demo.cpp"), "-o", exe])
    proc = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=200)
    return proc.returncode, proc.stdout.decode(), proc.stderr.decode()


@pytest.fixture(scope="module")
def demo(workdir):
    rc, out, err = build_and_run(workdir, "partition_spec_demo", ["-O1"])
    assert rc == 0, err[-4000:]
    return json.loads(out)


def test_under_asan_and_ubsan(workdir, demo):
    """a sanitizer-instrumented executable with its own main (no preloaded runtime; leak checking on): no report, and the
    same document"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    rc, out, err = build_and_run(workdir, "partition_spec_demo_san", SAN, env)
    assert rc == 0, err[-4000:]
    assert "AddressSanitizer" not in err and "LeakSanitizer" not in err and "runtime error:" not in err, err[-4000:]
    assert json.loads(out) == demo


ACCEPTED = {
    # name: (D, max_steps the lanes read, limit kind)
    "visible_1000": (24, 1000, 2), "latent_3": (23, 3, 1), "no_limit": (23, 0, 0), "kind_not_read": (24, 3, 2),
    "no_limit_ignores_max_steps": (23, 7, 0),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_spec_decides_dims_and_constants(demo, name):
    D, max_steps, limit = ACCEPTED[name]
    got = demo["spec"][name]
    assert got["code"] == 0 and got["dims"] == [D, 2] and got["kind"] == ENV_PARTITION
    assert (got["max_steps"], got["limit_kind"]) == (max_steps, limit)
    # nothing takes these lanes for an index env, a MemoryGame or a bandit; they have no tables
    assert (got["chain_size"], got["mem_actions"], got["bandit"], got["tables"]) == (0, 0, 0, 0)
    assert got["lane_offset"] == 25 and got["key_env_is_seed_3"] is True


REFUSED = {
    "limit_kind_3": "limit_kind", "limit_kind_negative": "limit_kind", "visible_0_steps": "step limit",
    "latent_2_32_steps": "step limit", "no_lanes": "n_lanes", "lanes_2_31": "n_lanes",
    # the order of the refusals is behaviour
    "limit_kind_before_steps": "limit_kind", "steps_before_lanes": "step limit",
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_spec_refusals_and_their_order(demo, name):
    got = demo["spec"][name]
    assert got["code"] == BUILD_ENV and REFUSED[name] in got["message"], got
    if REFUSED[name] == "limit_kind":  # (the step count and the lane count are every env's checks, in every env's words)
        assert got["message"].startswith("rl_env_create_partition: ")


def test_every_spec_case_is_checked(demo):
    assert sorted(demo["spec"]) == sorted(list(ACCEPTED) + list(REFUSED))
    assert demo["constants"] == [16, 20, 24, 10, 23, ENV_PARTITION]
    assert demo["traj"] == [16, 20, 24]


def test_the_older_constructors_name_the_new_one(demo):
    for name in ("rl_env_create", "rl_env_create_bandit"):
        got = demo["kinds"][name]
        assert got["code"] == BUILD_ENV and got["message"] == "RL_ENV_PARTITION lanes are created by rl_env_create_partition"


def test_chain_routing_and_refusals(demo):
    c = demo["chains"]
    G, H, H2 = 3, 8, 6
    rnn = G * H * 24 + G * H * H + 2 * G * H
    assert c["policy_24_2"] == {"code": 0, "in": 24, "out": 2, "P": rnn + H2 * H + H2 + 2 * H2 + 2, "lane_kernels": True}
    assert c["critic_24_1"] == {"code": 0, "in": 24, "out": 1, "P": rnn + H2 * H + H2 + H2 + 1, "lane_kernels": True}
    assert c["policy_23_2"]["code"] == 0 and c["in_21"]["code"] == 0 and c["in_24_out_12"]["code"] == 0
    for name in ("in_25", "out_13_at_24", "out_0_at_24", "hidden_257_at_24"):
        assert c[name]["code"] == BUILD_AGENT and c[name]["message"].startswith("rl_rnn_chain_create_wide24: in_dim 1..24, "), c[name]
    # at up to 20 inputs it is the older constructors, bound and words
    assert c["in_0"]["code"] == BUILD_AGENT and c["in_0"]["message"].startswith("supported recurrent chain shapes: in_dim 1..8")
    assert c["out_13_at_19"]["message"].startswith("rl_rnn_chain_create_wide20: in_dim 1..20")
    assert c["out_13_at_14"]["message"].startswith("rl_rnn_chain_create_wide: in_dim 1..16")
    assert c["in_9_out_9"]["code"] == 0
    assert c["routing"] == [1, 1, 1, 1, 1, 1]


def test_rollout_path_and_the_refusal_of_feed_forward_modules(demo):
    r = demo["rollout"]
    assert r["gru_24"] == {"code": 0, "path": r["stack"]} == r["lstm_23"]
    for name in ("gru_24_on_23", "three_outputs"):
        assert r[name]["code"] == INVALID_ARGUMENT and "does not match the env" in r[name]["message"]
    for name in ("fused_mlp", "general_mlp"):  # by name, before a shape is compared
        assert r[name]["code"] == UNSUPPORTED and r[name]["message"].startswith("rl_rollout: feed-forward modules")
        assert "RL_ENV_PARTITION" in r[name]["message"]
    assert r["cartpole_fused_mlp"] == {"code": 0, "path": r["cartpole"]}  # the older kinds keep their paths
    assert r["chain_fused_mlp"] == {"code": 0, "path": r["index_mlp"]}


def test_scalar_env_equals_the_python_lanes(demo):
    s = demo["scalar"]
    assert (s["features"], s["actions"], s["discount"]) == (23, 2, 0.999)
    lane = P.PartitionLane(11, 5)
    assert s["axis"] == lane.axis and s["pos0"] == lane.env_pos
    assert s["obs0"] == lane.obs_features().astype(int).tolist()
    for t in (1, 2):
        reward, kind = lane.step(t - 1)
        assert (s["reward%d" % t], s["kind%d" % t], s["pos%d" % t]) == (float(reward), P.CONTINUE, lane.env_pos)
        assert s["obs%d" % t] == lane.obs_features().astype(int).tolist()
    assert np.sum(s["obs1"][21:23]) == 1 and s["obs0"][10] == 1


def test_scalar_env_composes_with_the_mirrors_visible_limit(demo):
    """WithVisibleStepLimit<PartitionGame>, what the CPU-only configuration runs, against the Python lanes under VISIBLE 3"""
    w = demo["wrapped"]
    lane = P.PartitionLane(11, 5, P.Limit(P.LIMIT_VISIBLE, 3))
    assert w["features"] == 24 and np.array_equal(np.array(w["obs0"], np.float32), lane.obs_features())
    for t in (1, 2, 3):
        reward, kind = lane.step(t & 1)
        assert (w["reward%d" % t], w["kind%d" % t]) == (float(reward), kind)
        assert np.array_equal(np.array(w["obs%d" % t], np.float32), lane.obs_features()), t
    assert w["kind3"] == P.INTERRUPT and w["obs3"][23] == 0.0 and w["obs1"][23] == np.float32(2.0 / 3.0)
