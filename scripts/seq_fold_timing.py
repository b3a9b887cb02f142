"""Per-launch device times of the recurrent kernels that the fold of DESIGN 29 touched, at 16,384 lanes x 100 steps with
both cells, from the engine's profile counters (as scripts/gru_config5.py and scripts/lstm_config5.py print them):

  rollout         RL_K_ROLLOUT of rollout()                         k_rollout_gru<ChainOps, Cell>
  seq_forward     RL_K_POLICY_FUSED of seq_forward() of the policy  k_gru_seq_forward<2, Cell> with successor evaluations
  fvp             RL_K_POLICY_FUSED of policy_fvp()                 the training forward + the two tangent kernels
  forward_record  RL_K_POLICY_FUSED of policy_gradient(), variant 1 k_gru_seq_forward<2, Cell> with the activation record
  backward        RL_K_BACKWARD of policy_gradient(), variant 1     k_gru_bptt<2> / k_seq_head_backward<2> + k_lstm_bptt

Each figure is the scope's milliseconds divided by its launches; REPEATS repeats of each, printed with their median and
spread (max - min) as one JSON line.  Run it on the two commits to be compared in the same session (RELEARN_LIB selects
the library):  python scripts/seq_fold_timing.py [lanes [steps [repeats]]]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relearn_amd as ra  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 5

out = {"lanes": N, "horizon": T, "repeats": REPEATS, "lib": ra.LIB_PATH}
for cell, cls in (("gru", ra.GruMlp), ("lstm", ra.LstmMlp)):
    eng = ra.Engine(0)
    env = ra.ChainEnv(eng, N, max_steps=100, seed_env=0, seed_actor=1)
    pol, cri = cls(eng, 5, 2), cls(eng, 5, 1)
    pol.init(2)
    cri.init(3)
    traj = ra.Trajectory(eng, N, T, 5)
    v = np.linspace(-1.0, 1.0, pol.P).astype(np.float32)

    def scope(name, call, variant=0):
        eng.set_kernel_variant(variant)
        eng.profile_read(reset=True)
        call()
        ms, launches = eng.profile_read(reset=True)[name]
        eng.set_kernel_variant(0)
        return ms / launches

    def measure():
        m = {"rollout": scope("rollout", lambda: ra.rollout(env, pol, traj))}
        ra.gae(traj, cri, 0.95, 0.95)
        m["seq_forward"] = scope("policy_fused", lambda: pol.seq_forward(traj))
        m["fvp"] = scope("policy_fused", lambda: ra.policy_fvp(pol, traj, v, 1e-5))
        eng.set_kernel_variant(1)
        eng.profile_read(reset=True)
        ra.policy_gradient(pol, traj)
        prof = eng.profile_read(reset=True)
        eng.set_kernel_variant(0)
        m["forward_record"] = prof["policy_fused"][0] / prof["policy_fused"][1]
        m["backward"] = prof["backward"][0] / prof["backward"][1]
        return m

    eng.profile_enable(True)
    measure()  # warm-up (allocates the activation records)
    runs = [measure() for _ in range(REPEATS)]
    out[cell] = {k: {"ms": [round(r[k], 5) for r in runs], "median": round(float(np.median([r[k] for r in runs])), 5),
                     "spread": round(max(r[k] for r in runs) - min(r[k] for r in runs), 5)} for k in runs[0]}
    eng.close()
print(json.dumps(out))
