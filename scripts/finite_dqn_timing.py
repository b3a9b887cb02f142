"""Times of one collect + update period of a DQN agent over four actions: MemoryGame(4, 4) lanes (8 observation
features, episodes of 5 steps), 4,096 lanes, horizon 32, 50 optimisation steps on minibatches of 10,000 steps, exploration
rate 0.1, reward-to-go targets — with a feed-forward module of hidden sizes [64, 64] (step-wise collection on the per-layer
kernels) and with a GRU(16) -> ReLU -> MLP([16]) chain (one collection launch, the lane-per-thread update).

usage: python scripts/finite_dqn_timing.py [out.json]
Wall clock around the two entry points with the stream drained, median of 10 after 3; nothing here is a test bar."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import relearn_amd as ra  # noqa: E402

LANES, T, REPS, WARMUP = 4096, 32, 10, 3


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
    res = dict(device="%s (%s, %d CUs)" % (name, arch, cus), lanes=LANES, T=T, env="MemoryGame(4, 4)", opt_steps=50,
               minibatch_steps=10000)
    for key in ("mlp_64_64", "gru_16_mlp_16"):
        env = ra.MemoryEnv(engine, LANES, 4, 4, seed_env=3, seed_actor=4)
        if key == "mlp_64_64":
            q = ra.Mlp(engine, env.D, [64, 64], env.A)
        else:
            q = ra.RnnChain(engine, "gru", env.D, 16, env.A, mlp_hidden=16)
        q.init(5)
        cfg = ra.dqn_config_default()
        cfg.exploration_kind, cfg.exploration_start = ra.SCHEDULE_CONSTANT, 0.1
        cfg.minibatch_steps, cfg.opt_steps_per_update, cfg.buffer_capacity = 10000, 50, 4 * T
        cfg.discount_factor = 1.0
        for i in range(8):
            cfg.agent_key[i] = 21 + i
        dqn = ra.FiniteDqn(env, q, ra.Adam(q), cfg)

        def period():
            dqn.collect(T, want_stats=False)
            dqn.update()
        res[key] = dict(period=timed(engine, period), collect=timed(engine, lambda: dqn.collect(T, want_stats=False)))
        dqn.close()
    for k, v in res.items():
        print(k, v)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
