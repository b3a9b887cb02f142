"""Times of the recurrent DQN agent's two launch sequences: one collection at eps = 0 and one update for
GRU-MLP 5 -> 128 -> 128 -> 2 on Chain lanes (latent step limit 100), 4,096 lanes, T = 25 — and, as the yardstick of the
collection, k_stack_rollout's launch for GRU-MLP 6 -> 128 -> 128 -> 2 on two-arm meta-bandit lanes at the same lanes and
T (the one-launch recurrent rollout is built for those lanes; it runs the same module step per env step).

usage: python scripts/recurrent_dqn_timing.py [out.json]
Wall clock around the entry point with the stream drained, median of 20 after 5; nothing here is a test bar."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import relearn_amd as ra  # noqa: E402

LANES, T, REPS, WARMUP = 4096, 25, 20, 5


def timed(engine, f):
    ms = []
    for i in range(WARMUP + REPS):
        engine.sync()
        t0 = time.perf_counter()
        f()
        engine.sync()
        if i >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=REPS)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    engine = ra.Engine(0)
    name, arch, cus = engine.info()
    env = ra.ChainEnv(engine, LANES, max_steps=100, limit=ra.LIMIT_LATENT, seed_env=3, seed_actor=4)
    q = ra.GruMlp(engine, 5, 2)
    q.init(5)
    cfg = ra.dqn_config_default()
    cfg.exploration_kind, cfg.exploration_start = ra.SCHEDULE_CONSTANT, 0.0
    cfg.minibatch_steps, cfg.opt_steps_per_update, cfg.buffer_capacity = 10000, 10, 4 * T
    cfg.discount_factor = 0.95
    for i in range(8):
        cfg.agent_key[i] = 21 + i
    res = dict(device="%s (%s, %d CUs)" % (name, arch, cus), lanes=LANES, T=T, module="GRU-MLP 5-128-128-2")
    for target, key in ((ra.DQN_TARGET_REWARD_TO_GO, "reward_to_go"), (ra.DQN_TARGET_ONE_STEP_TD, "one_step_td")):
        cfg.target = target
        dqn = ra.RecurrentDqn(env, q, ra.Adam(q), cfg)
        if "collect_eps0" not in res:
            res["collect_eps0"] = timed(engine, lambda: dqn.collect(T, want_stats=False))
        else:
            dqn.collect(T, want_stats=False)
        res["update_%s" % key] = dict(timed(engine, dqn.update), minibatch_steps=10000, opt_steps=10)
        dqn.close()
    cfg.exploration_start = 1.0
    dqn = ra.RecurrentDqn(env, q, ra.Adam(q), cfg)
    res["collect_eps1"] = timed(engine, lambda: dqn.collect(T, want_stats=False))
    dqn.close()
    meta = ra.MetaBanditEnv(engine, LANES, n_arms=2, episodes_per_trial=13, seed_env=3, seed_actor=4)
    pol = ra.GruMlp(engine, meta.D, 2)
    pol.init(5)
    traj = ra.Trajectory(engine, LANES, T, meta.D)
    res["k_stack_rollout_meta_6_128_128_2"] = timed(engine, lambda: ra.rollout(meta, pol, traj))
    for k, v in res.items():
        print(k, v)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
