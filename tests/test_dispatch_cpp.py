"""The launchers' dispatch primitives (relearn_amd/csrc/dispatch.hpp) and the lane families with their feature ranges
(relearn_amd/csrc/handle_spec.hpp) on the CPU, through tests/cpp/dispatch_demo.cpp, built plainly with -Wall -Wextra
-Werror: a value inside a table reaches `go` once, as that constant; a value outside never does, and the caller hears
`false` — for an env, the family's refusal with code and words."""
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
UNSUPPORTED = 10
# the lane families in EnvLanes' order: name, feature range, refusal
FAMILIES = [
    ("cartpole", 4, 5, "CartPole lanes: 4 or 5 observation features"),
    ("index", 4, 8, "index env lanes: 4..8 observation features"),
    ("meta_bandit", 6, 16, "meta-bandit lanes: 6..16 observation features"),
    ("meta_mdp", 8, 20, "meta-MDP lanes: 8..20 observation features"),
    ("meta_mdp_wide", 15, 20, "meta-MDP lanes of nine or ten states: 15..20 observation features"),
    ("partition", 23, 24, "PartitionGame lanes: 23 or 24 observation features"),
    ("tabular_mdp", 2, 8, "tabular-MDP lanes: 2..8 observation features"),
]
LANES = {name: i for i, (name, *_) in enumerate(FAMILIES)}
# RL_ENV_* (include/relearn_hip.h) -> family; RL_ENV_META_MDP by its state count; 8 is no kind
KIND_FAMILY = {0: "cartpole", 1: "index", 2: "index", 3: "index", 4: "meta_bandit", 5: "tabular_mdp", 7: "partition"}


@pytest.fixture(scope="module")
def demo():
    exe = os.path.join(tempfile.mkdtemp(prefix="relearn_dispatch_"), "demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.dirname(HERE),
                           os.path.join(HERE, "cpp", "dispatch_demo.cpp"), "-o", exe])
    out = {}
    for line in subprocess.check_output([exe], timeout=60).decode().splitlines():
        fields, _, message = line.partition(" |")
        name, *numbers = fields.split()
        out.setdefault(name, []).append((tuple(int(v) for v in numbers), message.strip()))
    return out


def test_with_range_calls_go_once_with_the_value_or_not_at_all(demo):
    want = [((v, 1, v, 1) if 3 <= v <= 7 else (v, 0, -1, 0), "") for v in range(2, 9)]
    assert demo["range"] == want


def test_with_one_of_takes_the_listed_values_alone(demo):
    want = [((v, 1, v, 1) if v in (2, 8, 12) else (v, 0, -1, 0), "") for v in range(1, 14)]
    assert demo["one_of"] == want


def test_with_bool(demo):
    assert demo["bool"] == [((0, 1, 0), ""), ((1, 1, 1), "")]


def test_nested_dispatch_reaches_the_inner_lambda_with_both_constants(demo):
    want = [((s, a, 1, s, a) if 2 <= s <= 4 and a in (2, 5) else (s, a, 0, -1, -1), "")
            for s in range(1, 6) for a in range(1, 7)]
    assert demo["nested"] == want


def test_env_shapes_family_by_family(demo):
    want = []
    for kind in range(9):
        for states in (8, 10):
            family = KIND_FAMILY.get(kind)
            if kind == 6:
                family = "meta_mdp_wide" if states > 8 else "meta_mdp"
            for d in range(26):
                if family is None:
                    want.append(((kind, states, d, UNSUPPORTED, -1, -1), "env kernels: unknown env kind"))
                    continue
                _, lo, hi, refusal = FAMILIES[LANES[family]]
                if lo <= d <= hi:
                    want.append(((kind, states, d, 0, LANES[family], d), ""))
                else:
                    want.append(((kind, states, d, UNSUPPORTED, LANES[family], -1), refusal))
    assert len(want) == 9 * 2 * 26
    got = demo["shape"]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
