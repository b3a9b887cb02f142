"""Python restatement of the PartitionGame lanes (test infrastructure, not a test): `PartitionGame` of
src/envs/partition.rs:86-130 under the step-limit wrappers of wrappers/step_limit.rs, as include/relearn_hip.h states it
(rl_env_create_partition).

One lane is one env Prng of the oracle's binding — seed_from_u64(seed_env), set_stream(global lane) — consumed in the order
the reference's calls consume it: initial_state takes gen_range(0..10) (oracle_prng_gen_range_u64: whole u64s) and then
ten gen::<bool>(), a step takes ten more.  gen::<bool>() is one next_u32 whose sign bit is the value; [bool; 10] is ten of
them in index order.  `env_pos` is where the stream stands (oracle_prng_word_pos): the lanes' tests hold it even.

The closed loop (`rollout`) is built as tests/meta_mdp_ref.py's is: logits from the oracle's teacher-forced C forward over
the prefix, the action from oracle_log_softmax_f32 / oracle_categorical_sample_u at word period * T + t of the lane's actor
stream, the env from the lanes here.  Nothing here shares code with the library under test."""
import collections
import ctypes as C

import numpy as np

import oracle as O
import seq_multi_ref as R

L = O.lib()
CONTINUE, TERMINATE, INTERRUPT = 0, 1, 2
LIMIT_NONE, LIMIT_LATENT, LIMIT_VISIBLE = 0, 1, 2
NUM_FEATURES = 10  # partition.rs:11
LEFT, RIGHT = 0, 1  # Classification, and the action indices ClassifyLeft / ClassifyRight
F32 = np.float32
DISCOUNT_FACTOR = 0.999

Limit = collections.namedtuple("Limit", "kind max_steps")
NO_LIMIT = Limit(LIMIT_NONE, 0)


def obs_dim(limit):
    return 2 * NUM_FEATURES + 3 + (1 if limit.kind == LIMIT_VISIBLE else 0)


def make_rng(seed, stream):
    rng = O.Prng()
    L.oracle_prng_seed_from_u64(C.byref(rng), seed)
    L.oracle_prng_set_stream(C.byref(rng), stream)
    L.oracle_prng_set_word_pos(C.byref(rng), 0)
    return rng


def gen_bool(rng):
    """rand 0.8.5 Standard for bool: (rng.next_u32() as i32) < 0"""
    return (int(L.oracle_prng_next_u32(C.byref(rng))) >> 31) & 1 == 1


def gen_element(rng):
    """Standard for [bool; 10]: ten gen::<bool>() in index order"""
    return tuple(gen_bool(rng) for _ in range(NUM_FEATURES))


def features(element, feedback, limit, remaining):
    """[element, 10] [feedback is None] [previous element, 10] [one-hot label: Left, Right] [+ remaining / max_steps]"""
    f = np.zeros(obs_dim(limit), F32)
    f[:NUM_FEATURES] = element
    if feedback is None:
        f[NUM_FEATURES] = 1.0
    else:
        prev, label = feedback
        f[NUM_FEATURES + 1:2 * NUM_FEATURES + 1] = prev
        f[2 * NUM_FEATURES + 1 + label] = 1.0
    if limit.kind == LIMIT_VISIBLE:
        f[-1] = F32(float(remaining) / float(limit.max_steps))  # f64 quotient, then `as f32`
    return f


class PartitionLane:
    def __init__(self, seed_env, global_lane, limit=NO_LIMIT):
        self.limit = limit
        self.rng = make_rng(seed_env, global_lane)
        self.resets = 0
        self.reset()

    @property
    def env_pos(self):
        return int(L.oracle_prng_word_pos(C.byref(self.rng)))

    def reset(self):
        """PartitionGame::initial_state: the axis, then the element; feedback None"""
        self.axis = int(L.oracle_prng_gen_range_u64(C.byref(self.rng), 0, NUM_FEATURES))
        self.element = gen_element(self.rng)
        self.feedback = None
        self.remaining = self.limit.max_steps
        self.resets += 1

    def obs_features(self):
        return features(self.element, self.feedback, self.limit, self.remaining)

    def step(self, action):
        """-> (reward f32, successor kind); on Interrupt the lane holds the successor state (observe it, then reset())"""
        label = RIGHT if self.element[self.axis] else LEFT
        reward = F32(1.0) if int(action) == label else F32(-1.0)
        self.feedback = (self.element, label)
        self.element = gen_element(self.rng)
        if self.limit.kind != LIMIT_NONE:
            self.remaining -= 1
            if self.remaining == 0:
                return reward, INTERRUPT
        return reward, CONTINUE


class PartitionLanes:
    """n lanes stepped the way the library's env handle steps them"""

    def __init__(self, n, limit=NO_LIMIT, lane_offset=0, seed_env=0):
        self.n, self.limit, self.D = n, limit, obs_dim(limit)
        self.lanes = [PartitionLane(seed_env, lane_offset + i, limit) for i in range(n)]

    def reset(self):
        for lane in self.lanes:
            lane.reset()

    def observe(self):
        return np.stack([lane.obs_features() for lane in self.lanes], axis=1)  # [D][n]

    def step(self, actions):
        """-> reward [n] f32, flag [n] u8, next observation [D][n], interrupt successor [D][n] (zero where not cut)"""
        reward = np.zeros(self.n, F32)
        flag = np.zeros(self.n, np.uint8)
        term = np.zeros((self.D, self.n), F32)
        for i, lane in enumerate(self.lanes):
            r, f = lane.step(int(actions[i]))
            reward[i], flag[i] = r, f
            if f == INTERRUPT:
                term[:, i] = lane.obs_features()
                lane.reset()
        return reward, flag, self.observe(), term


Reference = collections.namedtuple("Reference", "periods margin observe")


def rollout(net, limit, n, T_, seed_env, seed_actor, params, lane_offset=0, periods=2):
    assert net.D == obs_dim(limit) and net.A == 2
    shape, full = R.shape_of(net), R.to_oracle(net, np.ascontiguousarray(params, dtype=np.float32))
    lanes = PartitionLanes(n, limit, lane_offset=lane_offset, seed_env=seed_env)
    rngs = []
    for i in range(n):
        r = O.Prng()
        L.oracle_prng_seed_from_u64(C.byref(r), seed_actor)
        L.oracle_prng_set_stream(C.byref(r), lane_offset + i)
        rngs.append(r)
    lp = np.zeros(2, F32)
    margin = np.inf
    out = []
    for period in range(periods):
        obs = np.zeros((net.D, T_ + 1, n), F32)
        term = np.zeros((net.D, T_, n), F32)
        action = np.zeros((T_, n), np.uint8)
        reward = np.zeros((T_, n), F32)
        flag = np.zeros((T_, n), np.uint8)
        obs[:, 0] = lanes.observe()
        for t in range(T_):
            prefix = {"obs": np.ascontiguousarray(obs[:, :t + 2]), "flag": np.ascontiguousarray(flag[:t + 1]),
                      "term_obs": np.ascontiguousarray(term[:, :t + 1])}
            z = O.stack_seq_forward(shape, net.L, full, prefix, want_succ=False)[0][:, t]  # [2][n]
            for i in range(n):
                L.oracle_prng_set_word_pos(C.byref(rngs[i]), period * T_ + t)
                w = L.oracle_prng_next_u32(C.byref(rngs[i]))
                u = F32(w >> 8) * F32(1.0 / (1 << 24))
                zi = np.ascontiguousarray(z[:, i])
                L.oracle_log_softmax_f32(O.f32p(zi), 2, O.f32p(lp), 0)
                action[t, i] = L.oracle_categorical_sample_u(O.f32p(lp), 2, C.c_float(u), 0)
                cum = np.cumsum(np.exp(R.log_softmax(zi.astype(np.float64))))[:-1]
                margin = min(margin, np.abs(np.float64(u) - cum).min())
            reward[t], flag[t], obs[:, t + 1], term[:, t] = lanes.step(action[t])
        out.append({"obs": obs, "action": action, "reward": reward, "flag": flag, "term_obs": term})
    return Reference(out, float(margin), lanes.observe())
