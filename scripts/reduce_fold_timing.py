"""Per-launch device times of the launches that the fold of DESIGN 30 touched — the slab reductions, the reduction with
the optimiser's step, the stand-alone step — and of the recurrent chains' row reduction, which that fold tried and left
as it was, from the engine's profile counters (the manner of scripts/seq_fold_timing.py):

  critic_narrow   RL_K_REDUCE of critic_update, 80 steps, Adam, Mlp(5, 128, 1)       k_reduce_opt<ADAM, 16, false>
                  (the benchmark's own loop: 256 slab rows, 57 workgroups)
  critic_wide     the same on Mlp(5, [64, 32], 1)                                     k_reduce_opt<ADAM, 64, false>
  trpo_narrow     RL_K_REDUCE of trpo_update on Mlp(5, 128, 2)                        k_reduce<16>
  gru_reduce      RL_K_REDUCE of policy_gradient + critic_update, 8 steps, GruMlp     k_seq_reduce
  gru_small       RL_K_SMALL of the same                                              k_opt_step<ADAM>
at 65,536 lanes x 128 steps (feed-forward) and 16,384 lanes x 100 steps (recurrent).

Each figure is the scope's milliseconds divided by its launches; REPEATS repeats of each after a warm-up, printed with
their median and spread (max - min) as one JSON line.  Run it on the two commits to be compared in the same session, in
turn (RELEARN_LIB selects the library):  python scripts/reduce_fold_timing.py [repeats [lanes [gru_lanes]]]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relearn_amd as ra  # noqa: E402

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
N_GRU = int(sys.argv[3]) if len(sys.argv) > 3 else 16384

out = {"lanes": N, "gru_lanes": N_GRU, "repeats": REPEATS, "lib": ra.LIB_PATH}


def per_launch(eng, call, *scopes):
    eng.profile_read(reset=True)
    call()
    prof = eng.profile_read(reset=True)
    return [prof[s][0] / prof[s][1] for s in scopes]


# feed-forward modules on a CartPole rollout
eng = ra.Engine(0)
env = ra.CartPoleEnv(eng, N, seed_env=0, seed_actor=1)
pol, cri, wide = ra.Mlp(eng, 5, 128, 2), ra.Mlp(eng, 5, 128, 1), ra.Mlp(eng, 5, [64, 32], 1)
pol.init(2)
cri.init(3)
wide.init(4)
traj = ra.Trajectory(eng, N, 128, 5)
ra.rollout(env, pol, traj)
ra.gae(traj, cri, 0.99, 0.95)
adam = ra.optimizer_config_default(ra.OPTIMIZER_ADAM)
copt, wopt = ra.Optimizer(cri, adam), ra.Optimizer(wide, adam)
p0 = pol.get_params()


def trpo():
    pol.set_params(p0)  # (every repeat solves from the same parameters: the same launches)
    ra.trpo_update(pol, traj)


def feed_forward():
    return {"critic_narrow": per_launch(eng, lambda: ra.critic_update(cri, copt, traj, 80), "reduce")[0],
            "critic_wide": per_launch(eng, lambda: ra.critic_update(wide, wopt, traj, 80), "reduce")[0],
            "trpo_narrow": per_launch(eng, trpo, "reduce")[0]}


eng.profile_enable(True)
feed_forward()  # warm-up
ff = [feed_forward() for _ in range(REPEATS)]
eng.close()

# the recurrent chain on a Chain rollout
eng = ra.Engine(0)
env = ra.ChainEnv(eng, N_GRU, max_steps=100, seed_env=0, seed_actor=1)
gpol, gcri = ra.GruMlp(eng, 5, 2), ra.GruMlp(eng, 5, 1)
gpol.init(2)
gcri.init(3)
traj = ra.Trajectory(eng, N_GRU, 100, 5)
ra.rollout(env, gpol, traj)
ra.gae(traj, gcri, 0.95, 0.95)
gopt = ra.Optimizer(gcri, adam)


def recurrent():
    def both():
        ra.policy_gradient(gpol, traj)
        ra.critic_update(gcri, gopt, traj, 8)
    r, s = per_launch(eng, both, "reduce", "small")
    return {"gru_reduce": r, "gru_small": s}


eng.profile_enable(True)
recurrent()  # warm-up (allocates the activation records)
rec = [recurrent() for _ in range(REPEATS)]
eng.close()

for name in list(ff[0]) + list(rec[0]):
    ms = [r[name] for r in (ff if name in ff[0] else rec)]
    out[name] = {"ms": [round(m, 5) for m in ms], "median": round(float(np.median(ms)), 5),
                 "spread": round(max(ms) - min(ms), 5)}
print(json.dumps(out))
