"""The HIP-free side of the meta-MDP lanes on the CPU (tests/cpp/meta_mdp_spec_demo.cpp, which includes
relearn_amd/csrc/handle_spec.hpp alone): env_spec_meta_mdp's refusals with code and words, D, A and the lanes' constants;
the table of one-launch shapes; rollout_path on these lanes; the shared row functions of include/rl_normal.h at the kernels'
loop bound; and the scalar env MetaRandomMdps (host/envs.hpp) against the Python lanes of tests/meta_mdp_ref.py, bit for
bit.  Built twice: plainly with -Wall -Wextra -Werror, and with -fsanitize=address,undefined as an executable of its own."""
import json
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import meta_mdp_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLAGS = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", ROOT]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
BUILD_ENV, INVALID_ARGUMENT, UNSUPPORTED = 5, 1, 10
ENV_META_MDP = 6


@pytest.fixture(scope="module")
def workdir():
    return tempfile.mkdtemp(prefix="relearn_meta_mdp_spec_")


def build_and_run(workdir, name, extra, env=None):
    exe = os.path.join(workdir, name)
    subprocess.check_call(FLAGS + extra + [os.path.join(HERE, "cpp", "meta_mdp_spec_demo.cpp"), "-o", exe])
    proc = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=200)
    return proc.returncode, proc.stdout.decode(), proc.stderr.decode()


@pytest.fixture(scope="module")
def demo(workdir):
    rc, out, err = build_and_run(workdir, "meta_mdp_spec_demo", ["-O1"])
    assert rc == 0, err[-4000:]
    return json.loads(out)


def test_under_asan_and_ubsan(workdir, demo):
    """the scalar env, the shared row functions and the spec as a sanitizer-instrumented executable with its own main (no
    preloaded runtime; leak checking on): no report, and the same document"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    rc, out, err = build_and_run(workdir, "meta_mdp_spec_demo_san", SAN, env)
    assert rc == 0, err[-4000:]
    assert "AddressSanitizer" not in err and "LeakSanitizer" not in err and "runtime error:" not in err, err[-4000:]
    assert json.loads(out) == demo


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


ACCEPTED = {
    # name: (S, A, L, E, alpha, prior mean, prior stddev, reward stddev)
    "default": (5, 5, 10, 10, 1.0, 1.0, 1.0, 1.0),
    "2x2": (2, 2, 1, 1, 1.0, 1.0, 1.0, 1.0),
    "8x4": (8, 4, 10, 10, 0.5, 1.0, 1.0, 0.0),
    "4x8": (4, 8, 10, 10, 2.5, 1.0, 1.0, 1.0),
    "6x6": (6, 6, (1 << 32) - 1, 10, 1.0, 1.0, 1.0, 1.0),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_spec_decides_dims_and_constants(demo, name):
    S, A, L, E, alpha, pm, ps, sd = ACCEPTED[name]
    got = demo["spec"][name]
    assert got["code"] == 0 and got["dims"] == [S + A + 4, A] and got["kind"] == ENV_META_MDP
    assert (got["rows"], got["states"], got["actions"], got["inner_steps"], got["episodes"]) == (S * A, S, A, L, E)
    assert got["chain_size"] == 0 and got["lane_offset"] == 25 and got["tables_unset"] is True
    assert got["prior"] == [f64_bits(alpha), f64_bits(pm), f64_bits(ps), f64_bits(sd)]


REFUSED = {
    "states_1": "n_states 2..8", "states_9": "n_states 2..8", "actions_1": "n_actions 2..8", "actions_9": "n_actions 2..8",
    "17_features": "at most 16", "reference_default_10x5": "at most 16", "inner_0": "max_inner_steps",
    "inner_2_32": "max_inner_steps", "episodes_0": "episodes_per_trial", "episodes_2_32": "episodes_per_trial",
    "alpha_0": "alpha", "alpha_negative": "alpha", "alpha_inf": "alpha", "alpha_nan": "alpha",
    "prior_mean_nan": "reward_prior_mean", "prior_stddev_negative": "reward_prior_stddev",
    "prior_stddev_inf": "reward_prior_stddev", "stddev_negative": "reward_stddev", "stddev_nan": "reward_stddev",
    "discount_inf": "discount_factor", "latent_limit": "step limit", "visible_limit": "step limit", "no_lanes": "n_lanes",
    "sizes_before_alpha": "n_states 2..8",  # the order of the refusals is behaviour: sizes first
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_spec_refusals(demo, name):
    got = demo["spec"][name]
    assert got["code"] == BUILD_ENV and REFUSED[name] in got["message"], got
    if name != "no_lanes":  # (the lane count is every env's check, in every env's words)
        assert got["message"].startswith("rl_env_create_meta_mdp: ")


def test_every_spec_case_is_checked(demo):
    assert sorted(demo["spec"]) == sorted(list(ACCEPTED) + list(REFUSED))


def test_fused_shape_table(demo):
    """data a CPU test reads: the smallest shape, the odd widths, the default, the most features with the widest row, the
    most actions with two head passes — and the closed-loop cases run every one of them"""
    want = [[2, 2], [3, 2], [4, 3], [5, 5], [8, 4], [4, 8]]
    assert demo["fused"]["table"] == want and sorted(demo["fused"]["accepted"]) == sorted(want)
    assert {(c.dist.S, c.dist.A) for c in M.CLOSED} >= {tuple(s) for s in want}


def test_rollout_paths(demo):
    p = demo["paths"]
    assert p["gru_linear_5x5"] == p["lstm_mlp_8x4"] == p["gru_mlp_3x3_outside_the_table"] == "ROLL_STACK"
    assert p["gru_tile_shape_on_2x2"] == "ROLL_STACK"  # never the tile kernels, whatever the widths
    assert p["feed_forward_2x2"] == "ROLL_GENERAL"
    assert p["wrong_width"]["code"] == INVALID_ARGUMENT and "does not match the env" in p["wrong_width"]["message"]
    assert p["two_output_chain_on_five_actions"]["code"] == UNSUPPORTED


def test_row_functions_at_the_kernels_bound(demo):
    assert demo["rows"]["same"] is True and demo["rows"]["rows"] >= 300 and demo["rows"]["zero_entries"] > 100
    assert demo["word_pos"] is True


@pytest.mark.parametrize("index", range(6))
def test_scalar_env_equals_the_python_lanes(demo, index):
    """three trials and a step on streams 0, 25 and 69: rewards, successor codes, observations, the successor
    observation of every trial's end and every trial's tables, bit for bit"""
    c = demo["scalar"]["cases"][index]
    d = M.dist(c["S"], c["A"], c["E"], c["L"], alpha=c["alpha"], reward_stddev=c["reward_stddev"])
    assert c["trial_steps"] == M.trial_steps(d)
    D = d.S + d.A + 4
    for g, got in c["lanes"].items():
        g = int(g)
        lane = M.MetaMdpLane(d, c["seed"], g)
        cum, mean = [lane.cum], [lane.mean]
        reward, flag, obs, term = [], [], [], []
        for t in range(3 * M.trial_steps(d) + 1):
            r, f = lane.step((3 * t + g) % d.A)
            reward.append(r), flag.append(f)
            if f == M.INTERRUPT:
                term.append(lane.obs_features())
                lane.reset()
                cum.append(lane.cum), mean.append(lane.mean)
            obs.append(lane.obs_features())
        bits32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).ravel().tolist()
        ends = len(flag) // M.trial_steps(d)  # three trials and a step (four trials where a trial is one step)
        assert got["flag"] == flag and flag.count(M.INTERRUPT) == ends >= 3
        assert got["reward"] == bits32(reward)
        assert got["obs"] == bits32(obs) and len(got["obs"]) == D * len(flag)
        assert got["term_obs"] == bits32(term)
        assert got["cum"] == bits32(cum) and len(cum) == ends + 1
        assert got["mean"] == np.ascontiguousarray(mean, np.float64).view(np.uint64).ravel().tolist()
    assert demo["scalar"]["refused"] == 4
