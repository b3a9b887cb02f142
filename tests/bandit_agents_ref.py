"""Python restatement of the bandit baselines on the meta-bandit lanes (test infrastructure, not a test):
`ResettingMetaAgent<TC>` (src/agents/meta.rs:135-199) over `SerialActorAgent` (src/agents/serial.rs:43-95) — a fresh
inner agent per trial, the inner actor in Training mode, every pull updates the inner agent at once — with TC =
RandomAgentConfig (src/agents/random.rs:59-73), TabularQLearningAgentConfig (src/agents/tabular.rs:21-51, 113-133,
159-180, 222-232) or UCB1AgentConfig (src/agents/bandits/ucb.rs:106-160, 209-234), over tests/meta_lanes_ref.py for the env.

One lane's actor stream is one Prng of the oracle's binding — seed_from_u64(seed_actor), set_stream(global lane) —
consumed sequentially.  Python floats are IEEE doubles without contraction: the arithmetic is written out literally,
one operation per statement where the order matters.  Nothing here shares code with the library under test."""
import ctypes as C
import math

import numpy as np

import meta_lanes_ref as M
import oracle as O

L = O.lib()
RANDOM, TABULAR_Q, UCB1 = 0, 1, 2


class RandomInner:
    """RandomAgent: act = IndexSpace::sample = gen_range(0..k) (spaces/index.rs:65-67); no state"""

    def __init__(self, k):
        self.k = k

    def act(self, rng):
        return int(L.oracle_prng_gen_range_u64(rng, 0, self.k))

    def update(self, action, reward):
        pass


class TabularQInner:
    """BaseTabularQLearningAgent over a bandit's single observation"""

    def __init__(self, k, rate, count, value):
        self.k, self.rate = k, rate
        self.counts = [int(count)] * k
        self.values = [float(value)] * k

    def act(self, rng):
        # Training mode: the draw is taken whatever the rate (tabular.rs:222-232)
        if L.oracle_prng_gen_f64(rng) < self.rate:
            return int(L.oracle_prng_gen_range_u64(rng, 0, self.k))
        best = 0  # ndarray-stats argmax: the FIRST maximal value
        for a in range(1, self.k):
            if self.values[a] > self.values[best]:
                best = a
        return best

    def update(self, action, reward):
        # tabular.rs:159-180; a bandit step terminates: no successor value
        self.counts[action] += 1
        w = 1.0 / float(self.counts[action])
        v = self.values[action]
        v = v * (1.0 - w)
        v = v + w * reward
        self.values[action] = v


class Ucb1Inner:
    """BaseUCB1Agent over a bandit's single observation, rewards declared in [0, 1]"""

    def __init__(self, k, rate):
        self.k, self.rate = k, rate
        self.values = [0.5] * k  # one success and one failure per arm (ucb.rs:122-125)
        self.counts = [2] * k
        self.visit = 2 * k

    def act(self, rng):
        log_squared_visit_count = 2.0 * math.log(float(self.visit))
        best, best_v = 0, None
        for a in range(self.k):
            q = log_squared_visit_count / float(self.counts[a])
            ucb = math.sqrt(q) * self.rate
            ucb = ucb + self.values[a]
            if best_v is None or ucb >= best_v:  # the LAST maximal index (utils/iter/cmp.rs:58)
                best, best_v = a, ucb
        return best

    def update(self, action, reward):
        scaled = (reward + (-0.0)) * 1.0  # reward_shift = -min_reward, reward_scale_factor = 1 / width
        self.visit += 1
        self.counts[action] += 1
        d = scaled - self.values[action]
        self.values[action] = self.values[action] + d / float(self.counts[action])


def build_inner(kind, k, rate, count, value):
    if kind == RANDOM:
        return RandomInner(k)
    if kind == TABULAR_Q:
        return TabularQInner(k, rate, count, value)
    return Ucb1Inner(k, rate)


DEFAULTS = {RANDOM: (0.0, 0, 0.0), TABULAR_Q: (0.2, 0, 0.0), UCB1: (0.2, 0, 0.0)}


class BanditAgentLanes:
    """n lanes of ResettingMetaAgent, each with its own actor Prng; drives a meta_lanes_ref.MetaLanes"""

    def __init__(self, n, k, kind, exploration_rate=None, initial_action_count=None, initial_action_value=None,
                 lane_offset=0, seed_actor=1):
        d = DEFAULTS[kind]
        self.n, self.k, self.kind = n, k, kind
        self.args = (kind, k, d[0] if exploration_rate is None else float(exploration_rate),
                     d[1] if initial_action_count is None else int(initial_action_count),
                     d[2] if initial_action_value is None else float(initial_action_value))
        self.rngs = []
        for i in range(n):
            r = O.Prng()
            L.oracle_prng_seed_from_u64(C.byref(r), seed_actor)
            L.oracle_prng_set_stream(C.byref(r), lane_offset + i)
            L.oracle_prng_set_word_pos(C.byref(r), 0)
            self.rngs.append(r)
        self.inner = [build_inner(*self.args) for _ in range(n)]

    def act(self, i, lane):
        """the action for lane i at the env lane's present observation; a pull's update is taken by `observe_pull`"""
        if not lane.inner_done and lane.prev is None and lane.remaining == lane.E:
            self.inner[i] = build_inner(*self.args)  # ResettingMetaAgent::initial_state: the meta episode starts
        if lane.inner_done:
            return 0  # some_element(); nothing is drawn
        return self.inner[i].act(C.byref(self.rngs[i]))

    def rollout(self, env, T):
        """T steps of every lane of `env` (a MetaLanes) -> the planes of MetaLanes.replay and the action plane"""
        D, n = env.D, env.n
        obs = np.zeros((D, T + 1, n), np.float32)
        term = np.zeros((D, T, n), np.float32)
        reward = np.zeros((T, n), np.float32)
        flag = np.zeros((T, n), np.uint8)
        action = np.zeros((T, n), np.uint8)
        obs[:, 0] = env.observe()
        for t in range(T):
            pulls = [not lane.inner_done for lane in env.lanes]
            for i, lane in enumerate(env.lanes):
                action[t, i] = self.act(i, lane)
            reward[t], flag[t], obs[:, t + 1], term[:, t] = env.step(action[t])
            for i in range(n):
                if pulls[i]:  # the update the next observation triggers (meta.rs:166-182)
                    self.inner[i].update(int(action[t, i]), float(reward[t, i]))
        return {"obs": obs, "action": action, "reward": reward, "flag": flag, "term_obs": term}

    def state(self):
        """the agent state AFTER the updates of all pulls so far, as rl_bandit_agent_state_read lays it out"""
        st = {"pos": np.array([L.oracle_prng_word_pos(C.byref(r)) for r in self.rngs], np.uint64)}
        if self.kind != RANDOM:
            st["counts"] = np.array([[a.counts[j] for a in self.inner] for j in range(self.k)], np.uint64)
            st["values"] = np.array([[a.values[j] for a in self.inner] for j in range(self.k)], np.float64)
        if self.kind == UCB1:
            st["visits"] = np.array([a.visit for a in self.inner], np.uint64)
        return st


def ln_table(k, E):
    return np.array([2.0 * math.log(float(2 * k + j)) for j in range(E)], np.float64)
