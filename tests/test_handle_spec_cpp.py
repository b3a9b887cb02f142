"""The HIP-free half of the env and module constructors (relearn_amd/csrc/handle_spec.hpp) on the CPU.

tests/cpp/handle_spec_demo.cpp includes that header alone and answers the case list of tests/constructor_cases.py.  Its
answers are held to tests/golden/constructor_table.json and tests/golden/rollout_launch_counts.json — the files the GPU
tests record and check on the device — so the words, the order of the refusals, D, A, P and the bytes behind them cannot
drift apart between a machine with a GPU and one without; the initial parameter vectors are held to the oracle bit for
bit.  Built twice: plainly with -Wall -Wextra -Werror, and with -fsanitize=address,undefined as an executable of its own.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import constructor_cases as CC  # noqa: E402
import oracle as O  # noqa: E402

FLAGS = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", ROOT]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.fixture(scope="module")
def workdir():
    d = tempfile.mkdtemp(prefix="relearn_handle_spec_")
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("\n".join(CC.lines()) + "\n")
    return d


def build_and_run(workdir, name, extra, env=None):
    exe = os.path.join(workdir, name)
    subprocess.check_call(FLAGS + extra + [os.path.join(HERE, "cpp", "handle_spec_demo.cpp"), "-o", exe])
    proc = subprocess.run([exe, os.path.join(workdir, "cases.txt")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=200)
    return proc.returncode, proc.stdout.decode(), proc.stderr.decode()


@pytest.fixture(scope="module")
def demo(workdir):
    rc, out, err = build_and_run(workdir, "handle_spec_demo", ["-O1"])
    assert rc == 0, err[-4000:]
    return json.loads(out)


def golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def test_under_asan_and_ubsan(workdir, demo):
    """the same program as a sanitizer-instrumented executable (no preloaded runtime; leak checking on): no report, and
    the same document"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    rc, out, err = build_and_run(workdir, "handle_spec_demo_san", SAN, env)
    assert rc == 0, err[-4000:]
    assert "AddressSanitizer" not in err and "LeakSanitizer" not in err and "runtime error:" not in err, err[-4000:]
    assert json.loads(out) == demo


def test_the_header_is_free_of_hip():
    """what it may include: the standard library, the three public headers and the scalar env mirror"""
    src = open(os.path.join(ROOT, "relearn_amd", "csrc", "handle_spec.hpp")).read()
    quoted = [l.split('"')[1] for l in src.splitlines() if l.startswith("#include \"")]
    assert sorted(quoted) == ["../../include/relearn_hip.h", "../../include/rl_chacha.h", "../../include/rl_detmath.h",
                              "host/envs.hpp"]
    assert "hip/" not in src and "__global__" not in src and "__device__" not in src


ENV_CTORS = ("env", "bandit", "meta", "meta_wide", "mdp")


@pytest.mark.parametrize("name,ctor,nums", CC.CASES, ids=[c[0] for c in CC.CASES])
def test_constructor_table(demo, name, ctor, nums):
    """refusals: code and words of the device's table.  Accepted shapes: its D and A, or its P — and its bytes and
    allocation count follow from what the header decided"""
    got, want = demo["cases"][name], golden("constructor_table.json")[name]
    assert got["code"] == want["code"] and got.get("message") == want.get("message")
    if want["code"] != 0 or ctor.startswith("init_"):
        return
    if ctor.endswith("_as"):  # (kind and MemoryGame shape of the config in front: read by nothing)
        ctor, nums = ctor[:-3], nums[3:]
    if ctor in ENV_CTORS:
        assert got["dims"] == want["dims"]
        n, D = nums[3] if ctor in ("env", "bandit") else nums[2], got["dims"][0]
        # four f64 state columns, nv_pos, steps_remaining, reset_count, actions, flag, reward; obs and term_obs [D][n]
        lanes, allocations = n * (4 * 8 + 1 + 4 + 4 + 1 + 1 + 4) + 2 * n * D * 4, 12
        if ctor == "mdp":  # mean and stddev f64 [S][A], cum f32 [S][A][S]: one allocation
            S, A = nums[3], nums[4]
            lanes, allocations = lanes + S * A * 16 + S * A * S * 4, 13
        assert (want["bytes"], want["allocations"]) == (lanes, allocations)
        assert got["kind"] == {"env": nums[0], "bandit": CC.ENV_BANDIT, "meta": CC.ENV_META, "meta_wide": CC.ENV_META,
                               "mdp": CC.ENV_MDP}[ctor]
    else:
        assert got["params"] == want["params"]
        twin = got["twin_params"]  # the twin's parameters, its gather scratch and its padded tangent
        assert want["bytes"] == 4 * (got["alloc_floats"] + 3 * twin) and want["allocations"] == (4 if twin else 1)


def test_every_case_is_answered(demo):
    assert sorted(demo["cases"]) == sorted(n for n, _, _ in CC.CASES + CC.ROLLOUT_EXTRA)
    assert sorted(demo["rollouts"]) == sorted(CC.ROLLOUT_CASES) and sorted(demo["inits"]) == sorted(CC.INIT_VECTORS)


@pytest.mark.parametrize("name", sorted(CC.ROLLOUT_CASES))
def test_rollout_path(demo, name):
    """rollout_path for every pair of tests/test_gpu_rollout_paths.py: the path the case list names (and the device rolled
    the pair), or the device's refusal"""
    got, want, path = demo["rollouts"][name], golden("rollout_launch_counts.json")[name], CC.ROLLOUT_CASES[name][2]
    if path is None:
        assert got == {"code": want["code"], "message": want["message"]}
    else:
        assert got == path and want["code"] == 0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("name", sorted(CC.INIT_VECTORS))
def test_initial_parameters_are_the_oracles(demo, name):
    v = CC.INIT_VECTORS[name]
    if v[0] == "mlp":
        _, seed, in_dim, hidden, out_dim, bias, kinit, binit = v
        # (without bias vectors: the oracle's Zeros bias draws nothing either, and its entries are dropped)
        want = O.mlp_layers_init(in_dim, hidden, out_dim, seed, kinit, binit if bias else ("Zeros", "FanAvg", 0.0))
        if not bias:
            keep, k = [], 0
            for fi, fo in zip([in_dim] + hidden, hidden + [out_dim]):
                keep.append(want[k:k + fi * fo])
                k += fi * fo + fo
            want = np.concatenate(keep)
    else:
        _, seed, cell, in_dim, H, layers, H2, out_dim, inits = v
        # (a Linear tail is the first layer of an MLP tail whose hidden width is out_dim: Linear(H, out_dim), fan_in H + 1)
        want = O.stack_init_with(O.GruShape(in_dim, H, H2 or out_dim, out_dim, cell), layers, seed, inits)
        if H2 == 0:
            want = want[:want.size - (out_dim * out_dim + out_dim)]
    assert demo["inits"][name] == bits(want)
