"""The meta-bandit lanes' Python restatement (tests/meta_lanes_ref.py) against the reference's own expectations, and the
new C-ABI surface as far as it shows without a GPU.  CPU only.

The fixture tests/golden/meta_env_fixtures.json is the step sequence of the reference's `meta_env_expected_steps`
(src/envs/meta.rs:642-769) as data."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import meta_lanes_ref as M
import relearn_amd as ra

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "meta_env_fixtures.json")))
KIND = {"continue": M.CONTINUE, "terminate": M.TERMINATE, "interrupt": M.INTERRUPT}


def fixture_obs(o):
    prev = None if o["prev"] is None else (o["prev"]["action"], o["prev"]["reward"])
    return (o["inner_none"], prev, o["done"])


def test_restatement_reproduces_the_reference_step_sequence():
    env = FIXTURE["env"]
    lane = M.MetaLane(env["n_arms"], env["episodes_per_trial"], env["distribution"], seed_env=0, global_lane=0)
    assert lane.observation() == fixture_obs(FIXTURE["initial_observation"])
    kinds = []
    for t, s in enumerate(FIXTURE["steps"]):
        reward, succ = lane.step(s["action"])
        assert reward == s["reward"] and succ == KIND[s["successor"]], t
        assert lane.observation() == fixture_obs(s["observation"]), t
        kinds.append(succ)
        if succ != M.CONTINUE:
            lane.reset()
            assert lane.observation() == fixture_obs(FIXTURE["initial_observation"])
    assert kinds.count(M.INTERRUPT) == 1 and M.TERMINATE not in kinds


@pytest.mark.parametrize("k", [2, 3, 4])
def test_feature_vectors_of_the_fixture_observations(k):
    """the observation shapes of the fixture (a fresh inner episode and the three pulls it holds) and a pull of the last
    arm, written out by hand: [inner None] [prev None] [one-hot(action), k] [reward] [done]"""
    z = [0.0] * (k - 2)
    want = {
        (False, None, False): [0, 1, 0, 0] + z + [0, 0],        # a fresh inner episode
        (True, (0, 1.0), True): [1, 0, 1, 0] + z + [1, 1],      # pulled arm 0, reward 1
        (True, (1, 0.0), True): [1, 0, 0, 1] + z + [0, 1],      # pulled arm 1, reward 0
        (True, (0, 0.0), True): [1, 0, 1, 0] + z + [0, 1],      # pulled arm 0, reward 0
        (True, (k - 1, 1.0), True): [1, 0] + [0] * (k - 1) + [1] + [1, 1],  # the last arm, reward 1
    }
    seen = {fixture_obs(s["observation"]) for s in FIXTURE["steps"]} | {fixture_obs(FIXTURE["initial_observation"])}
    assert seen <= set(want) and len(seen) == 4
    for obs, f in want.items():
        got = M.features(k, *obs)
        assert got.dtype == np.float32 and got.shape == (k + 4,)
        assert got.tolist() == [float(x) for x in f], obs


@pytest.mark.parametrize("dist", [M.UNIFORM_BERNOULLI, M.ONE_HOT, M.ROUND_ROBIN])
@pytest.mark.parametrize("E", [1, 3, 4])
def test_a_trial_is_2E_minus_1_steps_and_ends_in_interrupt(E, dist):
    lanes = M.MetaLanes(6, k=3, episodes=E, distribution=dist, lane_offset=2, seed_env=5)
    rs = np.random.default_rng(E)
    T = 3 * (2 * E - 1)
    out = lanes.replay(rs.integers(0, 3, (T, 6)).astype(np.uint8))
    want = np.zeros(T, np.uint8)
    want[2 * E - 2::2 * E - 1] = M.INTERRUPT
    assert np.array_equal(out["flag"], np.repeat(want[:, None], 6, axis=1))
    # the Interrupt's successor: inner None, prev Some, done; the observation after it: a fresh trial
    cut = out["flag"] == M.INTERRUPT
    assert np.all(out["term_obs"][0][cut] == 1.0) and np.all(out["term_obs"][1][cut] == 0.0)
    assert np.all(out["term_obs"][:, ~cut] == 0.0)
    assert np.all(out["obs"][1, 1:][cut] == 1.0) and np.all(out["obs"][0, 1:][cut] == 0.0)
    # restart steps earn nothing
    if E > 1:
        assert np.all(out["reward"][1:2 * E - 2:2] == 0.0)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_one_hot_trials_have_exactly_one_arm_at_one(k):
    lanes = M.MetaLanes(40, k=k, episodes=2, distribution=M.ONE_HOT, seed_env=3)
    goods = set()
    for _ in range(4):
        for lane in lanes.lanes:
            assert sorted(lane.arms) == [0.0] * (k - 1) + [1.0]
            goods.add(lane.arms.index(1.0))
        lanes.reset()
    assert goods == set(range(k))


def test_uniform_bernoulli_means_and_round_robin_arms():
    lanes = M.MetaLanes(50, k=4, episodes=2, distribution=M.UNIFORM_BERNOULLI, seed_env=1)
    means = np.array([lane.arms for lane in lanes.lanes])
    assert means.shape == (50, 4) and np.all((means >= 0.0) & (means <= 1.0)) and 0.35 < means.mean() < 0.65
    rr = M.MetaLane(3, 1, M.ROUND_ROBIN, 0, 7)
    for j in range(7):  # the good arm of a lane's j-th trial is j mod k
        assert rr.arms.index(1.0) == j % 3
        rr.reset()


def test_the_library_exports_the_meta_bandit_entry_points():
    lib = ra.lib()
    assert hasattr(lib, "rl_env_create_meta_bandit") and hasattr(lib, "rl_meta_bandit_config_default")
    assert "rl_env_create_meta_bandit" in ra.ABI_SYMBOLS and "rl_meta_bandit_config_default" in ra.ABI_SYMBOLS
    assert ra.ENV_META_BANDIT == 4


def test_config_default_is_the_reference_default():
    """UniformBernoulliBandits::default (bandits.rs:140-144), TrialEpisodeLimit::default (meta.rs:557-564)"""
    m = ra.meta_bandit_config_default()
    assert (m.n_arms, m.distribution, m.episodes_per_trial) == (2, ra.BANDITS_UNIFORM_BERNOULLI, 10)
    assert C.sizeof(ra.MetaBanditConfig) == 16
    assert ra.lib().rl_meta_bandit_config_default(None) == ra.ERR_INVALID_ARGUMENT
