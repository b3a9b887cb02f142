"""tests/dqn_ring_ref.py, the Python restatement of ReplayBuffer that the index-env DQN tests compare the device's
store with, against the oracle's own store (oracle/dqn.c over oracle_replay, which the reference's replay tests pin).
The oracle's store can only be filled by its CartPole collection, so that is what drives both: every step the oracle
wrote is fed to the restatement, and bookkeeping and contents are compared for every lane after every collection."""
import numpy as np
import pytest

import oracle as O
from dqn_ring_ref import Full, ReplayRing, RingStore

KEY = [0x9E3779B9, 0x7F4A7C15, 3, 4, 5, 6, 7, 0xFFFFFFFF]


def feed(store, osim, fed):
    """the steps the oracle's lanes wrote since the last call (its step data is append-only by absolute step number)"""
    for i in range(store.n):
        _, _, total = osim.lane_info(i)
        for k in range(fed[i], total):
            o, a, r, nx, no = osim.step_data(i, k)
            assert store.write(i, o, a, r, nx, no if nx == O.INTERRUPT else None) == k
        fed[i] = total


def compare(store, osim):
    evicted = 0
    for i in range(store.n):
        assert store.lane_info(i) == osim.lane_info(i), i
        tags, lens = store.lane_dump(i)
        tags_o, lens_o = osim.lane_dump(i)
        assert np.array_equal(tags, tags_o) and np.array_equal(lens, lens_o), i
        evicted += int(tags[0] > 0) if len(tags) else 0
        for k in tags:
            o, a, r, nx, no = osim.step_data(i, int(k))
            so, sa, sr, snx, sno = store.step_data(i, int(k))
            assert np.array_equal(so, o) and (sa, snx) == (a, nx) and sr == r, (i, k)
            if nx == O.INTERRUPT:
                assert np.array_equal(sno, no), (i, k)
        # Episodes::get over the restatement walks the same episodes as the dump
        r = store.rings[i]
        starts = [r.episode(e) for e in range(r.num_episodes())]
        assert [ln for _, ln in starts] == list(lens) and (not starts or starts[0][0] == tags[0])
    return evicted


@pytest.mark.parametrize("limit", [O.LIMIT_VISIBLE, O.LIMIT_NONE], ids=["5-features", "4-features"])
def test_restated_ring_follows_the_oracle_store_through_evictions(limit):
    # capacity 48 and max_steps 23: evictions from the second collection on (tests/test_gpu_dqn.py)
    n, cap = 40, 48
    for eps, T in [(1.0, 30), (0.5, 45), (0.0, 31)]:
        sim = O.LaneSim(n, max_steps=23, limit=limit, seed_env=21, seed_actor=34)
        qs = O.MlpShape(sim.D, 32, 2)
        osim = O.DqnSim(sim, qs, O.mlp_init(qs, 77), cap, KEY, 100)
        store, fed, evicted = RingStore(n, cap, sim.D), [0] * n, 0
        for rep in range(4):
            flags, full = osim.collect(T, eps)
            assert not full
            feed(store, osim, fed)
            evicted = compare(store, osim)
        assert evicted > n // 2  # most lanes have dropped whole episodes by the end


def test_restated_ring_reports_full_like_the_oracle():
    sim = O.LaneSim(8, max_steps=500, seed_env=21, seed_actor=34)
    qs = O.MlpShape(5, 32, 2)
    osim = O.DqnSim(sim, qs, O.mlp_init(qs, 77), 6, KEY, 100)
    assert osim.collect(30, 0.0)[1]  # an episode outgrows six steps
    ring = ReplayRing(6)
    for _ in range(6):
        ring.write_step(False)
    with pytest.raises(Full):
        ring.write_step(False)


def test_bounded_episode_table_drops_its_oldest_episode():
    """replay.hpp's addition to the reference's deque: with E episode slots, the E + 1st complete episode evicts the
    oldest one although steps are left"""
    ring = ReplayRing(10, episode_capacity=2)
    for k in range(3):
        ring.write_step(False)
        ring.write_step(True)
    assert ring.words() == (2, 4, 1, 2, 6) and ring.episode_ends == [4, 6]
