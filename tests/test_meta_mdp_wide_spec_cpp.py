"""The HIP-free side of rl_env_create_meta_mdp_wide on the CPU (tests/cpp/meta_mdp_wide_spec_demo.cpp, which includes
relearn_amd/csrc/handle_spec.hpp alone): env_spec_meta_mdp_wide's D, A and constants at the accepted shapes; every refusal
with code and words, in the entry point's own name, and the order of the refusals; equality with env_spec_meta_mdp over
that one's whole range; the wide table of one-launch shapes; rl_rnn_chain_create_wide20's routing; and the shared row
functions of include/rl_normal.h at the bound 16 of the second row class against the bound S, bit for bit.  Built twice:
plainly with -Wall -Wextra -Werror, and with -fsanitize=address,undefined as an executable of its own."""
import json
import os
import struct
import subprocess
import tempfile

import pytest

import meta_mdp_wide_cases as W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLAGS = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", ROOT]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
BUILD_ENV, BUILD_AGENT = 5, 4
ENV_META_MDP = 6


@pytest.fixture(scope="module")
def workdir():
    return tempfile.mkdtemp(prefix="relearn_meta_mdp_wide_spec_")


def build_and_run(workdir, name, extra, env=None):
    exe = os.path.join(workdir, name)
    subprocess.check_call(FLAGS + extra + [os.path.join(HERE, "cpp", "meta_mdp_wide_spec_demo.cpp"), "-o", exe])
    proc = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=200)
    return proc.returncode, proc.stdout.decode(), proc.stderr.decode()


@pytest.fixture(scope="module")
def demo(workdir):
    rc, out, err = build_and_run(workdir, "meta_mdp_wide_spec_demo", ["-O1"])
    assert rc == 0, err[-4000:]
    return json.loads(out)


def test_under_asan_and_ubsan(workdir, demo):
    """a sanitizer-instrumented executable with its own main (no preloaded runtime; leak checking on): no report, and the
    same document"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    rc, out, err = build_and_run(workdir, "meta_mdp_wide_spec_demo_san", SAN, env)
    assert rc == 0, err[-4000:]
    assert "AddressSanitizer" not in err and "LeakSanitizer" not in err and "runtime error:" not in err, err[-4000:]
    assert json.loads(out) == demo


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


ACCEPTED = {
    # name: (S, A, L, E, alpha, reward stddev, floats of a stored row)
    "10x5": (10, 5, 10, 10, 1.0, 1.0, 16),
    "9x2": (9, 2, 1, 1, 2.5, 1.0, 16),
    "10x6": (10, 6, 10, 10, 0.5, 0.0, 16),
    "8x8": (8, 8, (1 << 32) - 1, 10, 1.0, 1.0, 8),
    "9x7": (9, 7, 10, 10, 1.0, 1.0, 16),
    "5x5": (5, 5, 10, 10, 1.0, 1.0, 8),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_spec_decides_dims_and_constants(demo, name):
    S, A, L, E, alpha, sd, row = ACCEPTED[name]
    got = demo["spec"][name]
    assert got["code"] == 0 and got["dims"] == [S + A + 4, A] and got["kind"] == ENV_META_MDP
    assert (got["rows"], got["states"], got["actions"], got["inner_steps"], got["episodes"]) == (S * A, S, A, L, E)
    assert got["chain_size"] == 0 and got["lane_offset"] == 25 and got["tables_unset"] is True
    assert got["row_floats"] == row
    assert got["prior"] == [f64_bits(alpha), f64_bits(1.0), f64_bits(1.0), f64_bits(sd)]


def test_the_case_tables_shapes_are_accepted(demo):
    assert {(10, 5), (9, 2), (10, 6), (8, 8)} == set(W.SHAPES) <= {tuple(int(x) for x in k.split("x")) for k in ACCEPTED}
    assert demo["constants"] == [16, 20, 8, 10]


SIZES = "n_states 2..10 and n_actions 2..8"
REFUSED = {
    "states_1": SIZES, "states_11": SIZES, "actions_1": SIZES, "actions_9": SIZES, "21_features_10x7": "at most 20",
    "21_features_9x8": "at most 20", "inner_0": "max_inner_steps", "inner_2_32": "max_inner_steps",
    "episodes_0": "episodes_per_trial", "episodes_2_32": "episodes_per_trial", "alpha_0": "alpha", "alpha_nan": "alpha",
    "prior_mean_nan": "reward_prior_mean", "prior_stddev_negative": "reward_prior_stddev", "stddev_inf": "reward_stddev",
    "discount_inf": "discount_factor", "latent_limit": "step limit", "visible_limit": "step limit", "no_lanes": "n_lanes",
    # the order of the refusals is behaviour
    "sizes_before_inner": SIZES, "inner_before_episodes": "max_inner_steps", "episodes_before_alpha": "episodes_per_trial",
    "alpha_before_prior_mean": "alpha must", "prior_mean_before_prior_stddev": "reward_prior_mean",
    "prior_stddev_before_stddev": "reward_prior_stddev", "stddev_before_discount": "reward_stddev is",
    "discount_before_limit": "discount_factor", "limit_before_lanes": "step limit",
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_spec_refusals_and_their_order(demo, name):
    got = demo["spec"][name]
    assert got["code"] == BUILD_ENV and REFUSED[name] in got["message"], got
    if name != "no_lanes":  # (the lane count is every env's check, in every env's words)
        assert got["message"].startswith("rl_env_create_meta_mdp_wide: ")


def test_every_spec_case_is_checked(demo):
    assert sorted(demo["spec"]) == sorted(list(ACCEPTED) + list(REFUSED))


def test_equal_to_the_older_spec_over_its_whole_range(demo):
    """S, A in 2..8 with S + A + 4 <= 16: 39 shapes build through both and are equal, config and lanes' struct byte for
    byte; the shapes the wide one adds (S 9..10, or 17..20 features) are refused by the older one"""
    older = sum(1 for S in range(2, 9) for A in range(2, 9) if S + A + 4 <= 16)
    wide = sum(1 for S in range(2, 11) for A in range(2, 9) if S + A + 4 <= 20)
    s = demo["same"]
    assert (s["equal"], s["wide_only"], s["differ"]) == (older, wide - older, 0) and s["neither"] == 13 * 11 - wide
    assert older == 39 and wide - older == 21


def test_wide_fused_shape_table(demo):
    f = demo["fused"]
    assert f["table"] == [[10, 5]] == f["accepted"] == [list(s) for s in W.FUSED]
    assert f["older_table"] == [[2, 2], [3, 2], [4, 3], [5, 5], [8, 4], [4, 8]] and f["older_takes_10x5"] is False


def test_chain_routing_and_refusals(demo):
    c = demo["chains"]
    G, H = 3, 8
    assert c["policy_19_5"] == {"code": 0, "in": 19, "out": 5, "P": G * H * 19 + G * H * H + 2 * G * H + 5 * H + 5, "lane_kernels": True}
    assert c["critic_19_1"]["code"] == 0 and c["critic_19_1"]["lane_kernels"] is True and c["critic_19_1"]["out"] == 1
    assert c["in_20_out_12"]["code"] == 0 and c["in_17"]["code"] == 0
    for name in ("in_21", "out_13_at_19", "out_0_at_19", "hidden_257_at_19"):
        assert c[name]["code"] == BUILD_AGENT and c[name]["message"].startswith("rl_rnn_chain_create_wide20: in_dim 1..20"), c[name]
    # at up to 16 inputs it is the older constructors, bound and words
    assert c["in_0"]["code"] == BUILD_AGENT and c["in_0"]["message"].startswith("supported recurrent chain shapes: in_dim 1..8")
    assert c["out_13_at_14"]["message"].startswith("rl_rnn_chain_create_wide: in_dim 1..16")
    assert c["in_9_out_9_at_8"]["code"] == 0
    assert c["routing"] == [1, 1, 1, 1]


def test_row_functions_at_the_second_row_class_bound(demo):
    r = demo["rows"]
    assert r["same"] is True and r["rule"] is True and r["rows"] >= 300 and r["zero_entries"] > 100 and r["rows_at_9_and_10"] >= 100
