"""ReplayBuffer restated in Python, for the DQN tests on envs the oracle's own store cannot be filled from (its
collection is CartPole's).  Reference: src/agents/buffers/replay.rs:11-127 (the step deque, the episode-end deque,
whole-episode eviction, WriteExperienceError::Full) and relearn_amd/csrc/replay.hpp (the same bookkeeping as ring words
plus a bounded episode table).  tests/test_dqn_ring_ref_cpu.py validates it against the oracle's store.

A lane's steps are tagged with the lane's absolute step number (total_step_count before the write), as the oracle's
store tags them; the step data is kept append-only under that tag, so evicted steps stay readable by tag."""
import numpy as np

CONTINUE, TERMINATE, INTERRUPT = 0, 1, 2


class Full(Exception):
    """WriteExperienceError::Full: the buffer holds one unfinished episode and nothing to evict"""


class ReplayRing:
    """one lane's ReplayBuffer bookkeeping"""

    def __init__(self, capacity, episode_capacity=None):
        self.capacity = capacity
        self.episode_capacity = episode_capacity or capacity
        self.steps = []         # tags of the stored steps, oldest first (VecDeque<PartialStep>)
        self.episode_ends = []  # one past the end of each stored episode, in total_step_count terms
        self.index_offset = 0   # total_step_count index of the first stored step
        self.total_step_count = 0
        self.evicted_episodes = 0  # episodes dropped so far: the ring index the device's ep_head counts

    def _drop_oldest_episode(self):
        ep_end = self.episode_ends.pop(0)
        assert ep_end > self.index_offset, "episodes always have at least 1 step"
        del self.steps[:ep_end - self.index_offset]
        self.index_offset = ep_end
        self.evicted_episodes += 1

    def write_step(self, episode_done):
        """replay.rs:89-115; returns the step's tag"""
        if len(self.steps) == self.capacity:
            if not self.episode_ends:
                raise Full()
            self._drop_oldest_episode()
        tag = self.total_step_count
        self.steps.append(tag)
        self.total_step_count += 1
        if episode_done:
            if len(self.episode_ends) == self.episode_capacity:  # replay.hpp: the bounded table drops its oldest episode
                self._drop_oldest_episode()
            self.episode_ends.append(self.total_step_count)
        return tag

    def num_steps(self):
        return len(self.steps)

    def num_episodes(self):
        return len(self.episode_ends)

    def episode_lens(self):
        ends = np.array([self.index_offset] + self.episode_ends, dtype=np.int64)
        return np.diff(ends)

    def episode(self, idx):
        """Episodes::get (replay.rs:154-165): (tag of the first step, length)"""
        end = self.episode_ends[idx]
        start = self.index_offset if idx == 0 else self.episode_ends[idx - 1]
        return start, end - start

    def words(self):
        """the device's ring words (replay.hpp LaneRing): head, count, ep_head, ep_count, total"""
        return self.index_offset, len(self.steps), self.evicted_episodes, len(self.episode_ends), self.total_step_count


class RingStore:
    """one ReplayRing per lane and the step data by (lane, tag)"""

    def __init__(self, n_lanes, capacity, obs_dim, episode_capacity=None):
        self.n, self.C, self.D = n_lanes, capacity, obs_dim
        self.E = episode_capacity or capacity
        self.rings = [ReplayRing(capacity, episode_capacity) for _ in range(n_lanes)]
        self.data = [[] for _ in range(n_lanes)]  # per lane: (obs, action, reward, flag, next_obs) by tag

    def write(self, lane, obs, action, reward, flag, next_obs=None):
        tag = self.rings[lane].write_step(flag != CONTINUE)
        assert tag == len(self.data[lane])
        nx = np.zeros(self.D, dtype=np.float32) if next_obs is None else np.array(next_obs, dtype=np.float32)
        self.data[lane].append((np.array(obs, dtype=np.float32), int(action), np.float32(reward), int(flag), nx))
        return tag

    def write_collection(self, obs, action, reward, flag, next_obs):
        """a collection's planes: obs / next_obs [T][D][n] (next_obs read where the flag is INTERRUPT), the rest [T][n]"""
        T = len(action)
        for i in range(self.n):
            for t in range(T):
                fl = int(flag[t][i])
                self.write(i, obs[t][:, i], action[t][i], reward[t][i], fl, next_obs[t][:, i] if fl == INTERRUPT else None)

    def lane_info(self, lane):
        r = self.rings[lane]
        return r.num_steps(), r.num_episodes(), r.total_step_count

    def lane_dump(self, lane):
        r = self.rings[lane]
        return np.array(r.steps, dtype=np.int32), r.episode_lens().astype(np.uint64)

    def step_data(self, lane, tag):
        return self.data[lane][tag]

    def check_device(self, dqn, ra):
        """every ring word and every stored step of a device store (`dqn`: relearn_amd.Dqn) against this one"""
        head, count = dqn.replay_read(ra.REPLAY_HEAD), dqn.replay_read(ra.REPLAY_COUNT)
        eph, epc = dqn.replay_read(ra.REPLAY_EP_HEAD), dqn.replay_read(ra.REPLAY_EP_COUNT)
        total, ep_end = dqn.replay_read(ra.REPLAY_TOTAL), dqn.replay_read(ra.REPLAY_EP_END)
        obs, nobs = dqn.replay_read(ra.REPLAY_OBS), dqn.replay_read(ra.REPLAY_NEXT_OBS)
        act, rew, flag = (dqn.replay_read(f) for f in (ra.REPLAY_ACTION, ra.REPLAY_REWARD, ra.REPLAY_FLAG))
        assert (dqn.C, dqn.E, dqn.n) == (self.C, self.E, self.n)
        for i in range(self.n):
            r = self.rings[i]
            assert (int(head[i]), int(count[i]), int(eph[i]), int(epc[i]), int(total[i])) == r.words(), i
            ends = [int(ep_end[(int(eph[i]) + k) % self.E, i]) for k in range(int(epc[i]))]
            assert ends == r.episode_ends, i
            for tag in r.steps:
                o, a, rw, fl, nx = self.data[i][tag]
                slot = tag % self.C
                assert np.array_equal(obs[:, slot, i], o), (i, tag)
                assert (act[slot, i], flag[slot, i]) == (a, fl) and rew[slot, i] == rw, (i, tag)
                if fl == INTERRUPT:
                    assert np.array_equal(nobs[:, slot, i], nx), (i, tag)
