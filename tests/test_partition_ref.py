"""CPU checks of the PartitionGame lanes' reference (tests/partition_ref.py) against facts that follow from
src/envs/partition.rs, and of the case tables of tests/partition_cases.py that the GPU tests run: the feature layout at
None and Some, the reward's sign against element[axis], the feedback, the axis within an episode, the stream position
(even, ten words per step), elements that straddle a ChaCha block, the episode length under each limit kind, the lane-range
property, every sampled action's margin, and the binding's new surface.  No device."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import partition_cases as W
import partition_ref as P
import relearn_amd as ra

L = O.lib()


def test_feature_layout_at_none_and_some():
    """[element, 10] [feedback is None] [previous element, 10] [one-hot label: Left, Right] [+ remaining]"""
    assert P.obs_dim(P.NO_LIMIT) == 23 == P.obs_dim(W.LATENT3) and P.obs_dim(W.VISIBLE3) == 24
    lane = P.PartitionLane(5, 0, W.VISIBLE3)
    f0, e0 = lane.obs_features(), lane.element
    assert f0.shape == (24,) and f0.dtype == np.float32
    assert np.array_equal(f0[:10], np.array(e0, np.float32)) and f0[10] == 1.0
    assert np.all(f0[11:23] == 0.0)  # the 12 entries behind a None marker are zero
    assert f0[23] == np.float32(1.0)  # 3 of 3 steps remain
    label = int(e0[lane.axis])
    r, succ = lane.step(label)
    f1 = lane.obs_features()
    assert r == 1.0 and succ == P.CONTINUE
    assert np.array_equal(f1[:10], np.array(lane.element, np.float32)) and f1[10] == 0.0
    assert np.array_equal(f1[11:21], np.array(e0, np.float32))  # the previous element
    assert f1[21 + label] == 1.0 and f1[21 + (1 - label)] == 0.0
    assert f1[23] == np.float32(2.0 / 3.0)
    assert set(np.unique(f1[:23])) <= {0.0, 1.0}
    assert P.PartitionLane(5, 0).obs_features().shape == (23,)


def test_reward_sign_feedback_and_axis():
    rs = np.random.default_rng(0)
    for g in range(40):
        lane = P.PartitionLane(9, g, P.Limit(P.LIMIT_LATENT, 6))
        axis = lane.axis
        assert 0 <= axis < 10
        for t in range(6):
            e, a = lane.element, int(rs.integers(0, 2))
            r, succ = lane.step(a)
            assert r == (1.0 if a == int(e[axis]) else -1.0)
            assert lane.feedback == (e, int(e[axis]))  # the previous element and its label
            assert lane.axis == axis  # never changes within an episode
            assert succ == (P.INTERRUPT if t == 5 else P.CONTINUE)
        lane.reset()
        assert lane.feedback is None
    axes = {P.PartitionLane(9, g).axis for g in range(200)}
    assert axes == set(range(10))


def test_bool_is_the_sign_bit_and_elements_follow_the_stream_in_index_order():
    lane = P.PartitionLane(3, 7)
    start = lane.env_pos - 10  # the element's ten words
    rng = P.make_rng(3, 7)
    L.oracle_prng_set_word_pos(C.byref(rng), start)
    words = [int(L.oracle_prng_next_u32(C.byref(rng))) for _ in range(20)]
    assert lane.element == tuple(w >= 1 << 31 for w in words[:10])
    lane.step(0)
    assert lane.element == tuple(w >= 1 << 31 for w in words[10:])


def test_env_pos_is_even_and_advances_by_ten_per_step():
    for g in range(64):
        lane = P.PartitionLane(11, g, W.LATENT3)
        first = lane.env_pos
        assert first % 2 == 0 and first >= 12 and (first - 10) % 2 == 0  # whole u64s for the axis, ten words
        for t in range(2):
            before = lane.env_pos
            lane.step(0)
            assert lane.env_pos == before + 10
        before = lane.env_pos
        _, succ = lane.step(0)
        assert succ == P.INTERRUPT and lane.env_pos == before + 10
        lane.reset()
        assert lane.env_pos % 2 == 0 and lane.env_pos >= before + 22
    # gen_range(0..10) rejects: not every lane takes one u64 for its axis
    firsts = {P.PartitionLane(11, g).env_pos for g in range(64)}
    assert 12 in firsts and len(firsts) > 1


def test_an_element_that_straddles_a_block_edge():
    """a lane whose first step draws words 12..21: block 0 gives six bits, block 1 four"""
    lane = next(l for l in (P.PartitionLane(11, g) for g in range(64)) if l.env_pos == 12)
    rng = P.make_rng(11, next(g for g in range(64) if P.PartitionLane(11, g).env_pos == 12))
    L.oracle_prng_set_word_pos(C.byref(rng), 12)
    words = [int(L.oracle_prng_next_u32(C.byref(rng))) for _ in range(10)]
    lane.step(1)
    assert lane.element == tuple(w >> 31 == 1 for w in words)
    assert (12 & 15) > 6 and lane.env_pos == 22


@pytest.mark.parametrize("limit,length", [(W.VISIBLE3, 3), (W.LATENT3, 3), (P.Limit(P.LIMIT_VISIBLE, 1), 1),
                                          (P.NO_LIMIT, None)])
def test_episode_length_under_each_limit_kind(limit, length):
    lanes = P.PartitionLanes(8, limit, seed_env=2)
    for t in range(12):
        _, flag, obs, term = lanes.step(np.zeros(8, np.uint8))
        cut = length is not None and (t + 1) % length == 0
        assert np.all(flag == (P.INTERRUPT if cut else P.CONTINUE)), t  # the env never terminates by itself
        if cut:
            assert np.all(obs[10] == 1.0) and np.all(term[10] == 0.0)  # None after the reset, Some in the successor
            if limit.kind == P.LIMIT_VISIBLE:
                assert np.all(term[23] == 0.0) and np.all(obs[23] == 1.0)
        else:
            assert np.all(term == 0.0)
    assert all(lane.resets == (1 if length is None else 1 + 12 // length) for lane in lanes.lanes)


@pytest.mark.parametrize("c", W.DRIVEN, ids=W.driven_id)
def test_driven_cases_hold_their_own_conditions(c):
    ref = W.driven_reference(c)
    D = P.obs_dim(c.limit)
    assert ref.observe0.shape == (D, c.n) and len(ref.steps) == W.DRIVEN_STEPS == 14
    print("%s: %d element draws of %d straddle a block" % (W.driven_id(c), ref.straddles, c.n * W.DRIVEN_STEPS))
    assert ref.straddles >= c.n  # in every case, many times
    flags = np.stack([s[1] for s in ref.steps])
    if c.limit.kind == P.LIMIT_NONE:
        assert np.all(flags == P.CONTINUE)
    else:
        assert np.array_equal(flags[:, 0], np.array([0, 0, 2] * 4 + [0, 0], np.uint8)) and np.all(flags == flags[:, :1])
    rewards = np.stack([s[0] for s in ref.steps])
    assert set(np.unique(rewards)) == {-1.0, 1.0}
    # feedback not cleared at a reset would show: after an Interrupt the None marker is set and the 12 entries are zero,
    # while the successor observation carries Some
    for (_, flag, obs, term) in ref.steps:
        cut = flag == P.INTERRUPT
        assert np.all(obs[10, cut] == 1.0) and np.all(obs[11:23, cut] == 0.0)
        assert np.all(term[10, cut] == 0.0) and np.all(term[21:23, cut].sum(0) == 1.0)
        assert np.all(obs[10, ~cut] == 0.0)
    # an element taken from its first block alone would show: the bits the second block gives are not all zero
    obs_all = np.stack([s[2] for s in ref.steps])
    assert obs_all[:, :10].mean() > 0.4 and obs_all[:, :10].mean() < 0.6


def test_lane_range_property():
    """offset 137 gives lanes 137..199 of the 200-lane run (and one lane more)"""
    whole, part = W.DRIVEN[0], W.DRIVEN[3]
    assert whole.limit == part.limit and whole.seed == part.seed and part.offset + part.n == 201
    a, b = W.driven_reference(whole), W.driven_reference(part)
    m = whole.n - part.offset
    assert np.array_equal(a.observe0[:, part.offset:], b.observe0[:, :m])
    for sa, sb, aa, ab in zip(a.steps, b.steps, a.actions, b.actions):
        assert np.array_equal(aa[part.offset:], ab[:m])
        for x, y in zip(sa, sb):
            assert np.array_equal(x[..., part.offset:], y[..., :m])


@pytest.mark.parametrize("c", W.CLOSED, ids=W.closed_id)
def test_closed_cases_hold_their_own_conditions(c):
    ref = W.closed_reference(c)
    print("%s: smallest margin of a sampled action %.3g (bar %.3g)" % (W.closed_id(c), ref.margin, W.MIN_MARGIN))
    assert ref.margin > W.MIN_MARGIN
    assert c.net.D == P.obs_dim(c.limit) and c.net.A == 2 and len(ref.periods) == W.PERIODS
    for p in ref.periods:
        assert sorted(np.unique(p["action"])) == [0, 1]
        assert (p["flag"] == P.INTERRUPT).any() == (c.limit.kind != P.LIMIT_NONE)
        assert p["obs"].shape == (c.net.D, c.T + 1, c.n)
    # T = 7 against episodes of 3 steps: an episode runs across the two collections
    if c.limit.kind != P.LIMIT_NONE:
        assert np.all(ref.periods[1]["flag"][1] == P.INTERRUPT) and np.all(ref.periods[0]["flag"][2] == P.INTERRUPT)


def test_binding_names_and_abi_exports():
    for name in ("rl_env_create_partition", "rl_rnn_chain_create_wide24", "rl_traj_create_wide24"):
        assert name in ra.ABI_SYMBOLS and hasattr(ra.lib(), name)  # declared, and exported by the built library
    assert ra.ENV_PARTITION == 7 and ra.PartitionEnv.DISCOUNT_FACTOR == P.DISCOUNT_FACTOR == 0.999
    assert ra.RnnChainWide24.CREATE == "rl_rnn_chain_create_wide24" and issubclass(ra.RnnChainWide24, ra.RnnChain)
    assert ra.TrajectoryWide24.CREATE == "rl_traj_create_wide24" and issubclass(ra.TrajectoryWide24, ra.Trajectory)
    assert ra.lib().rl_abi_version() == 6  # additive entry points: the version stays
