"""The recurrent chains' training calls return the bits they returned when tests/golden/seq_bits.json was recorded.

The table was recorded on the PARENT of the commit that folded the GRU and LSTM chains' copied kernels (one tangent kernel
pair templated on the cell in kernels_seq_fvp.hip, one head tail for the two forward cells in kernels_seq.hip, the f32
head backward once in kernels_seq_bwd.hip): that fold changes no sum order, so every hash must survive it, and
every later edit of these kernels that means to keep the arithmetic.  The other GPU tests of the recurrent chains
compare gradients and Fisher-vector products with an f64 evaluation within a tolerance; a reordered addition, a carried
tangent that is not zeroed at an episode end or a block of a ragged chunk that is walked twice can pass them and fails
here.

These kernels have no atomics, and their chunking (seq_ensure: ceil(blocks / 1024) blocks per chunk, at most 64) does
not depend on the device, so the table holds on every device and from run to run (it was recorded twice and the two
recordings were equal).

Calls per case, on a Chain rollout by the same module (setup_update of tests/test_gpu_gru.py / test_gpu_lstm.py), stored as
the sha256 of the returned bytes and their first four words: policy_gradient, critic_gradient and policy_fvp (reg 1e-5,
v = linspace(-1, 1, P)), for cell in {GRU, LSTM} x engine kernel variant in {0: the bf16-pipe training passes of
kernels_seq_train.hip, 1: the f32 kernels of kernels_seq.hip / kernels_seq_bwd.hip}; the tangent kernels run under both.

Shapes (n lanes, T steps, the Chain's max_steps):
  (32, 1, 9)      one (step, tile) block: the carried state is never read
  (32, 2, 1)      every step ends an episode: every carried h_dot / c_dot (and dh / dc) is zeroed
  (96, 7, 3)      three tiles, episodes ending mid-walk
  (2048, 20, 4)   1,280 blocks, two per chunk: the block loop of the tangent `pre` kernel and of the weight-gradient
                  kernels with a second iteration and the barriers between blocks
  (160, 205, 7)   1,025 blocks, two per chunk, 513 chunks with ONE block in the last: the `b1` clamp of those loops.  No
                  smaller shape leaves a ragged last chunk (it needs more than 1,024 blocks and an odd count).
The first three are also compared with the f64 oracle (test_fisher_vector_product_at_edge_shapes and the gradients'
edge-shape tests in tests/test_gpu_gru.py and tests/test_gpu_lstm.py).  The last two are pinned by bits ONLY: one f64 oracle
Fisher-vector product at 32,800 samples takes 15 s (GRU) to 21 s (LSTM) of CPU time, too long for a test — those shapes
are held to "what the parent returned", not re-derived from the oracle.

    python tests/test_gpu_seq_bits.py --record [--out FILE]

writes the table (run it on the commit whose bits are to be pinned).
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import relearn_amd as ra  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_bits.json")

CELLS = {"gru": "GruMlp", "lstm": "LstmMlp"}
SHAPES = [(32, 1, 9), (32, 2, 1), (96, 7, 3), (2048, 20, 4), (160, 205, 7)]
CASES = {"%s-v%d@%dx%dx%d" % (cell, variant, n, T, ms): (cell, variant, n, T, ms)
         for cell in CELLS for variant in (0, 1) for (n, T, ms) in SHAPES}


def bits(*arrays):
    """sha256 of the bytes a call returned and its first four values as hex words"""
    raw = b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)
    first = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint32) for a in arrays])[:4]
    return {"sha256": hashlib.sha256(raw).hexdigest(), "first": ["%08x" % w for w in first]}


def f32(*values):
    return np.array(values, dtype=np.float32)


def run_case(name):
    cell, variant, n, T, max_steps = CASES[name]
    eng = ra.Engine(0)
    eng.set_kernel_variant(variant)
    env = ra.ChainEnv(eng, n, max_steps=max_steps, seed_env=3, seed_actor=4)
    cls = getattr(ra, CELLS[cell])
    pol, cri = cls(eng, 5, 2), cls(eng, 5, 1)
    pol.init(21)
    cri.init(22)
    traj = ra.Trajectory(eng, n, T, 5)
    ra.rollout(env, pol, traj)
    ra.gae(traj, cri, 0.95, 0.9)
    out = {}
    g, loss, ent = ra.policy_gradient(pol, traj)
    out["rl_policy_gradient"] = bits(g, f32(loss, ent))
    g, loss = ra.critic_gradient(cri, traj)
    out["rl_critic_gradient"] = bits(g, f32(loss))
    v = np.linspace(-1.0, 1.0, pol.P).astype(np.float32)
    out["rl_policy_fvp"] = bits(ra.policy_fvp(pol, traj, v, 1e-5))
    eng.close()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_seq_bits(golden, name):
    got, want = run_case(name), golden["cases"][name]
    for call in sorted(got):
        print(name, call, got[call])
    assert got == want, {c: (got.get(c), want.get(c)) for c in set(got) | set(want) if got.get(c) != want.get(c)}


def record(path):
    table = {"cases": {name: run_case(name) for name in CASES}}
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(table["cases"]), path))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="write the table instead of checking it")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    if not args.record:
        ap.error("run under pytest to check; --record writes the table")
    record(args.out)
