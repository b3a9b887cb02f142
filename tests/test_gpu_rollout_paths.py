"""Which launches rl_rollout makes for every pair of env kind and module family, and what it refuses, pinned against a
recorded table (the mechanics of tests/test_gpu_pass_paths.py, at 64 lanes x 4 steps: the tile kernels need a multiple
of 32 lanes).

rl_rollout picks one of five paths — the per-layer kernels, the lane-per-thread recurrent kernels, the recurrent tile
kernels, the fused index-env MLP kernel, the fused CartPole kernel — from the env's kind and widths and the module's
shape.  Per case: the per-class launch counts of one rollout with profiling on and a digest of what it recorded
(actions, flags, rewards, observations).  Then where the rollout left the env, which is where its step counter shows (the
counter has no accessor: it is the word of the lane's streams the next step reads): rl_env_get_state behind the rollout
(index lanes keep their env-stream position in it; meta-bandit lanes refuse the call: null), one rl_env_step of action 0
and what it returned — reward, flag, next observation — and a second rollout behind that.  A path that advanced the
counter twice, or not at all, steps the index lanes on other words of the env stream and draws the second rollout's
actions from other words of the actor streams.  Refusals: status code and message.

    python tests/test_gpu_rollout_paths.py --record [--out FILE]

writes the table (run it on the commit whose sequences are to be pinned; the file is never edited by hand).
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import relearn_amd as ra  # noqa: E402
import constructor_cases as CC  # noqa: E402
from test_gpu_constructor_table import create, destroy, last_error  # noqa: E402
from test_gpu_pass_paths import Case  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_launch_counts.json")
N, T = 64, 4
# beside the pairs of constructor_cases.ROLLOUT_CASES: what rl_rollout refuses before it looks at the pair
HANDLE_CASES = ["refused-trajectory-width", "refused-trajectory-lanes", "refused-two-engines", "refused-null-policy"]
ALL_CASES = sorted(CC.ROLLOUT_CASES) + HANDLE_CASES


def digest_of(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def digest(traj):
    return digest_of(traj.read(f) for f in (ra.TRAJ_ACTION, ra.TRAJ_FLAG, ra.TRAJ_REWARD, ra.TRAJ_OBS, ra.TRAJ_TERM_OBS))


def state_digest(env):
    """rl_env_get_state: the four f64 columns, nv_pos, steps_remaining, reset_count — None where the lanes refuse it"""
    st, nv = np.zeros((4, N), dtype=np.float64), np.zeros(N, dtype=np.int32)
    rem, rc = np.zeros(N, dtype=np.uint64), np.zeros(N, dtype=np.uint64)
    code = ra.lib().rl_env_get_state(env, *[a.ctypes.data_as(C.c_void_p) for a in (st, nv, rem, rc)])
    return digest_of((st, nv, rem, rc)) if code == ra.OK else None


def step_digest(env, D):
    """one rl_env_step of action 0 on every lane: reward, flag, next observation, terminal observation"""
    reward, flag = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.uint8)
    obs, term = np.zeros((D, N), dtype=np.float32), np.zeros((D, N), dtype=np.float32)
    actions = np.zeros(N, dtype=np.uint8)
    assert ra.lib().rl_env_step(env, *[a.ctypes.data_as(C.c_void_p) for a in (actions, reward, flag, obs, term)]) == ra.OK
    return digest_of((reward, flag, obs, term))


def run_case(name):
    L = ra.lib()
    handle_case = name in HANDLE_CASES
    env_case, mod_case, _ = CC.ROLLOUT_CASES["cartpole-mlp-5-128-2" if handle_case else name]
    c = Case(CC.ROLLOUT_VARIANT.get(name, 0))
    eng, cases = c.eng, CC.by_name()
    other = ra.Engine(0) if name == "refused-two-engines" else None
    rc, env, _ = create(other or eng, *cases[env_case], n_lanes=N)
    assert rc == ra.OK, last_error(other or eng)
    rc, pol, _ = create(eng, *cases[mod_case])
    assert rc == ra.OK, last_error(eng)
    assert L.rl_mlp_init(pol, C.c_uint64(17)) == ra.OK
    d = C.c_uint32()
    assert L.rl_env_dims(env, C.byref(d), None) == ra.OK
    traj = ra.Trajectory(eng, N // 2 if name == "refused-trajectory-lanes" else N, T,
                         d.value - 1 if name == "refused-trajectory-width" else d.value)
    rec = {}

    def roll():
        rec["code"] = L.rl_rollout(env, None if name == "refused-null-policy" else pol, traj.h)

    c.call("rollout", roll)
    if rec["code"] != ra.OK:
        rec["message"] = last_error(other or eng)  # (rl_rollout reports to the env's engine)
    else:
        rec["launches"] = c.counts["rollout"]
        rec["first"] = digest(traj)
        rec["state_after"] = state_digest(env)
        rec["step_after"] = step_digest(env, d.value)
        assert L.rl_rollout(env, pol, traj.h) == ra.OK
        rec["second"] = digest(traj)
    traj.close()
    destroy(pol, "module")
    destroy(env, "env")
    c.close()
    if other:
        other.close()
    return rec


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_CASES)
def test_rollout_paths(golden, name):
    got = run_case(name)
    print(name, got)
    assert got == golden[name]
    if name in CC.ROLLOUT_CASES:
        assert (got["code"] == ra.OK) == (CC.ROLLOUT_CASES[name][2] is not None)


def test_the_table_covers_the_case_list(golden):
    """(no GPU) every case has a recorded answer and the file holds no others"""
    assert sorted(golden) == sorted(ALL_CASES)


def record(path):
    table = {name: run_case(name) for name in ALL_CASES}
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(table), path))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="write the table instead of checking it")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    if not args.record:
        ap.error("run under pytest to check; --record writes the table")
    record(args.out)
