"""Timings of the recurrent rollouts on meta-bandit lanes (profiles/wide_meta_timing.json): 4,096 lanes x T = 39,
GRU 128.  `old`: two and four arms through the older constructors alone (runs on an older library too: RELEARN_LIB=...);
`new`: also ten arms, one launch against the launch sequence per step, both tails.  One JSON line.

    python scripts/wide_meta_timing.py old|new
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relearn_amd as ra
what = sys.argv[1]
N, T, H, E = 4096, 39, 128, 10
eng = ra.Engine(0)
out = {"lib": os.environ.get("RELEARN_LIB", "this"), "lanes": N, "T": T, "hidden": H}

def timed(env, pol, variant, reps=20):
    traj = ra.Trajectory(eng, N, T, env.D)
    eng.set_kernel_variant(variant)
    eng.sync(); t0 = time.perf_counter()
    ra.rollout(env, pol, traj); eng.sync()
    first = (time.perf_counter() - t0) * 1e3
    ra.rollout(env, pol, traj); eng.sync()
    eng.timer_begin()
    for _ in range(reps): ra.rollout(env, pol, traj)
    ms = eng.timer_end() / reps
    eng.set_kernel_variant(0)
    traj.close()
    return {"ms": ms, "first_call_ms": first}

# two arms, the parent's constructors (DESIGN 37's measurement): the NQ = 2 instantiations
env2 = ra.MetaBanditEnv(eng, N, 2, E, seed_env=0, seed_actor=1)
for tail, mk in (("mlp", lambda: ra.GruMlp(eng, env2.D, 2, H, H)), ("linear", lambda: ra.GruLinear(eng, env2.D, 2, H))):
    pol = mk(); pol.init(2)
    out["two_arms_%s_fused" % tail] = timed(env2, pol, 0)
# four arms through rl_rnn_chain_create: the NQ = 4 rollout and the NQ = 8 step kernels
env4 = ra.MetaBanditEnv(eng, N, 4, E, seed_env=0, seed_actor=1)
pol = ra.RnnChain(eng, "gru", env4.D, H, 4); pol.init(2)
out["four_arms_linear_fused"] = timed(env4, pol, 0)
out["four_arms_linear_stepwise"] = timed(env4, pol, 1, reps=5)
if what == "new":
    env10 = ra.MetaBanditEnvWide(eng, N, 10, E, seed_env=0, seed_actor=1)
    for tail, mh in (("linear", None), ("mlp", H)):
        pol = ra.RnnChainWide(eng, "gru", env10.D, H, 10, mlp_hidden=mh); pol.init(2)
        out["ten_arms_%s_fused" % tail] = timed(env10, pol, 0)
        out["ten_arms_%s_stepwise" % tail] = timed(env10, pol, 1, reps=5)
print(json.dumps(out), flush=True)
