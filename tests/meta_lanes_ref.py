"""Python restatement of the meta-bandit lanes (test infrastructure, not a test):
`MetaEnv::new(D::new(k)).wrap(TrialEpisodeLimit::new(E))` of src/envs/meta.rs:128-203, 541-617 over Bandit<_>
(src/envs/bandits.rs:58-78), D = UniformBernoulliBandits (bandits.rs:96-106, 170-181), OneHotBandits (bandits.rs:229-243)
or RoundRobinDeterministicBandits (src/envs/testing.rs:108-160).

One lane is one env Prng of the oracle's binding — seed_from_u64(seed_env), set_stream(global lane) — consumed in the
order the reference's calls consume it: sample_environment at a trial's start (k uniform means / one gen_range / nothing),
one gen_bool per pull of a Bernoulli arm.  Nothing here shares code with the library under test."""
import ctypes as C

import numpy as np

import oracle as O

L = O.lib()
CONTINUE, TERMINATE, INTERRUPT = 0, 1, 2
UNIFORM_BERNOULLI, ONE_HOT, ROUND_ROBIN = "uniform_bernoulli", "one_hot", "round_robin"


def features(k, inner_none, prev, done):
    """MetaObservationSpace features (meta.rs:357-363, spaces/option.rs:87-114), k + 4 of them:
    [inner is None] [prev is None] [one-hot(prev action), k] [prev reward] [episode_done]"""
    f = np.zeros(k + 4, np.float32)
    f[0] = 1.0 if inner_none else 0.0
    if prev is None:
        f[1] = 1.0
    else:
        action, reward = prev
        f[2 + action] = 1.0
        f[2 + k] = np.float32(reward)
    f[k + 3] = 1.0 if done else 0.0
    return f


class MetaLane:
    """one lane: (MetaState, remaining episodes) and the lane's env Prng"""

    def __init__(self, k, episodes, distribution, seed_env, global_lane):
        self.k, self.E, self.dist = k, episodes, distribution
        self.rng = O.Prng()
        L.oracle_prng_seed_from_u64(C.byref(self.rng), seed_env)
        L.oracle_prng_set_stream(C.byref(self.rng), global_lane)
        L.oracle_prng_set_word_pos(C.byref(self.rng), 0)
        self.trials = 0
        self.reset()

    def reset(self):
        """Wrapped<_, TrialEpisodeLimit>::initial_state -> MetaEnv::initial_state: sample_environment, then the bandit's
        initial_state (no draw)"""
        r = C.byref(self.rng)
        if self.dist == UNIFORM_BERNOULLI:
            self.arms = [L.oracle_prng_uniform_f64_inclusive(r, 0.0, 1.0) for _ in range(self.k)]
        elif self.dist == ONE_HOT:
            good = int(L.oracle_prng_gen_range_u64(r, 0, self.k))
            self.arms = [1.0 if a == good else 0.0 for a in range(self.k)]
        else:
            self.arms = [1.0 if a == self.trials % self.k else 0.0 for a in range(self.k)]
        self.trials += 1
        self.inner_done = False  # inner_successor: Continue(()) / Terminate
        self.prev = None         # prev_step_obs
        self.remaining = self.E

    def observation(self):
        """(inner is None, prev, episode_done)"""
        return (self.inner_done, self.prev, self.inner_done)

    def obs_features(self):
        return features(self.k, *self.observation())

    def step(self, action):
        """-> (reward, successor kind); on Interrupt the lane holds the successor state (observe it, then reset())"""
        if self.inner_done:  # a new inner episode; the action is ignored
            self.inner_done, self.prev = False, None
            return 0.0, CONTINUE
        if self.dist == UNIFORM_BERNOULLI:
            reward = 1.0 if L.oracle_prng_gen_bool(C.byref(self.rng), self.arms[action]) else 0.0
        else:
            reward = self.arms[action]  # Deterministic: no draw
        self.prev = (int(action), reward)
        self.inner_done = True
        self.remaining -= 1
        return reward, (INTERRUPT if self.remaining == 0 else CONTINUE)


class MetaLanes:
    """n lanes stepped the way the library's env handle steps them: a lane whose step is not Continue records its
    successor observation and starts a new trial"""

    def __init__(self, n, k=2, episodes=10, distribution=UNIFORM_BERNOULLI, lane_offset=0, seed_env=0):
        self.n, self.k, self.D = n, k, k + 4
        self.lanes = [MetaLane(k, episodes, distribution, seed_env, lane_offset + i) for i in range(n)]

    def reset(self):
        for lane in self.lanes:
            lane.reset()

    def observe(self):
        return np.stack([lane.obs_features() for lane in self.lanes], axis=1)  # [D][n]

    def step(self, actions):
        """-> reward [n] f32, flag [n] u8, next observation [D][n], interrupt successor [D][n] (zero where not cut)"""
        reward = np.zeros(self.n, np.float32)
        flag = np.zeros(self.n, np.uint8)
        term = np.zeros((self.D, self.n), np.float32)
        for i, lane in enumerate(self.lanes):
            r, f = lane.step(int(actions[i]))
            reward[i], flag[i] = r, f
            if f == INTERRUPT:
                term[:, i] = lane.obs_features()
            if f != CONTINUE:
                lane.reset()
        return reward, flag, self.observe(), term

    def replay(self, actions):
        """actions [T][n] -> a trajectory's planes: obs [D][T+1][n], reward, flag [T][n], term_obs [D][T][n]"""
        T = actions.shape[0]
        obs = np.zeros((self.D, T + 1, self.n), np.float32)
        term = np.zeros((self.D, T, self.n), np.float32)
        reward = np.zeros((T, self.n), np.float32)
        flag = np.zeros((T, self.n), np.uint8)
        obs[:, 0] = self.observe()
        for t in range(T):
            reward[t], flag[t], obs[:, t + 1], term[:, t] = self.step(actions[t])
        return {"obs": obs, "reward": reward, "flag": flag, "term_obs": term}
