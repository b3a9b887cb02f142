"""MemoryGame(2, 2) under DQN with a recurrent and with a feed-forward action-value module.

The lane starts in state 0 or 1, walks through two history states whatever it does, and at the answer step earns +1 when
its action names the state it started in, -1 otherwise.  The answer step's observation is the same one-hot whatever the
episode started in: a feed-forward Q-network can only guess (mean episode reward 0), a recurrent one can carry the first
observation to the answer (mean episode reward towards +1, less what exploration costs).

usage: python scripts/dqn_memory_game.py [out.json] [updates] [lanes]
Prints the mean episode reward of every collection (training actor, exploration annealed 1.0 -> 0.05 over the first half
of the run) and writes both curves to out.json.  A demonstration; nothing asserts a threshold on it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import relearn_amd as ra  # noqa: E402


def run(engine, recurrent, updates, lanes, horizon=12):
    env = ra.MemoryEnv(engine, lanes, 2, 2, seed_env=5, seed_actor=6)
    q = ra.GruMlp(engine, env.D, 2, 32, 32) if recurrent else ra.Mlp(engine, env.D, [32, 32], 2)
    q.init(3)
    acfg = ra.adam_config_default()
    acfg.learning_rate = 3e-3
    cfg = ra.dqn_config_default()
    cfg.target = ra.DQN_TARGET_ONE_STEP_TD
    cfg.exploration_kind, cfg.exploration_start, cfg.exploration_end = ra.SCHEDULE_LINEAR_ANNEALED, 1.0, 0.05
    cfg.exploration_period = max(1, updates // 2) * horizon * lanes
    cfg.minibatch_steps, cfg.opt_steps_per_update = 1024, 8
    cfg.buffer_capacity = 4 * horizon
    cfg.discount_factor = 1.0
    for i in range(8):
        cfg.agent_key[i] = 11 + i
    dqn = (ra.RecurrentDqn if recurrent else ra.Dqn)(env, q, ra.Adam(q, acfg), cfg)
    summary = ra.StepsSummary(engine, lanes)
    curve = []
    for u in range(updates):
        st = dqn.collect(horizon)
        summary.push_dqn(dqn)
        s = summary.read()
        summary.clear()
        ust = dqn.update()
        curve.append(dict(update=u, exploration_rate=st.exploration_rate, episodes=int(s.episode_reward.count),
                          mean_episode_reward=s.episode_reward.mean, loss=ust.loss_last))
        print("%-12s update %3d  eps %.3f  mean episode reward %+.3f  loss %.4f" % (
            "gru-mlp" if recurrent else "feed-forward", u, st.exploration_rate, s.episode_reward.mean, ust.loss_last))
    dqn.close()
    return curve


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    updates = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    lanes = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    engine = ra.Engine(0)
    name, arch, cus = engine.info()
    result = dict(env="MemoryGame(2, 2)", lanes=lanes, updates=updates, device="%s (%s, %d CUs)" % (name, arch, cus),
                  gru_mlp=run(engine, True, updates, lanes), feed_forward=run(engine, False, updates, lanes))
    tail = lambda c: sum(r["mean_episode_reward"] for r in c[-10:]) / len(c[-10:])
    result["mean_of_last_10"] = dict(gru_mlp=tail(result["gru_mlp"]), feed_forward=tail(result["feed_forward"]))
    print("mean episode reward over the last 10 collections: gru-mlp %+.3f, feed-forward %+.3f" % (
        result["mean_of_last_10"]["gru_mlp"], result["mean_of_last_10"]["feed_forward"]))
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
