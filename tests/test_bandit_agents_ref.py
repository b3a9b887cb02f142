"""The restatement of the bandit baselines (tests/bandit_agents_ref.py) held to facts that do not come from it: the
reference's own test of ResettingMetaAgent (src/agents/meta.rs:238-264), the pull sequences the two tie rules give on
one-hot arms, the oracle's tabular Q-learning agent step by step, the number of words each actor draws — and the
library's new entry points as far as they go without a GPU.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import bandit_agents_ref as B
import meta_lanes_ref as M
import oracle as O
import relearn_amd as ra

L = O.lib()


def trials_of(planes):
    """per lane: the completed trials as lists of (action, reward) of their pulls, in order"""
    T, n = planes["flag"].shape
    done = []
    for i in range(n):
        cur = []
        for t in range(T):
            if planes["obs"][0, t, i] == 0.0:  # [inner observation is None] clear: this step is a pull
                cur.append((int(planes["action"][t, i]), float(planes["reward"][t, i])))
            if planes["flag"][t, i] == M.INTERRUPT:
                done.append((i, cur))
                cur = []
    return done


def one_hot_run(kind, n_lanes, T, **agent):
    k, E = 3, 20
    env = M.MetaLanes(n_lanes, k, E, M.ONE_HOT, seed_env=221)
    agents = B.BanditAgentLanes(n_lanes, k, kind, **agent)
    return env, agents, agents.rollout(env, T)


def test_the_references_own_test_ucb1_on_one_hot_bandits():
    """meta.rs:238-264: OneHot(3), 20 episodes per trial, UCB1 0.2, 1,000 steps: mean reward of completed trials
    > 0.7 * (20 - 3) = 11.9.  Worked out by hand from the last-maximal-index rule: the first pull is arm 2; a miss
    lowers that arm's bound below the untouched ones and the next pull is the last of those, a hit raises the arm's
    mean and it stays — so a trial pulls (2, 2, ...), (2, 1, 1, ...) or (2, 1, 0, 0, ...) and earns at least 18"""
    env, agents, planes = one_hot_run(B.UCB1, 1, 1000)
    done = trials_of(planes)
    assert len(done) == 1000 // 39
    rewards = [sum(r for _, r in pulls) for _, pulls in done]
    assert np.mean(rewards) > 11.9
    assert min(rewards) >= 18
    seen = set()
    for _, pulls in done:
        good = [a for a, r in pulls if r == 1.0][0]
        want = {2: [2] * 20, 1: [2] + [1] * 19, 0: [2, 1] + [0] * 18}[good]
        assert [a for a, _ in pulls] == want
        seen.add(good)
    assert seen == {0, 1, 2}
    assert np.all(agents.state()["pos"] == 0)  # UCB1 draws nothing


def test_greedy_on_one_hot_bandits_first_maximal_index():
    """Greedy = TabularQ (0.0, 2, 0.5): all values tie at 0.5 and the FIRST is pulled; a miss lowers it to 1/3, a hit
    raises it to 2/3 — (0, 0, ...), (0, 1, 1, ...) or (0, 1, 2, 2, ...)"""
    env, agents, planes = one_hot_run(B.TABULAR_Q, 4, 39 * 6, exploration_rate=0.0, initial_action_count=2,
                                      initial_action_value=0.5)
    done = trials_of(planes)
    assert len(done) == 24
    seen = set()
    for _, pulls in done:
        good = [a for a, r in pulls if r == 1.0][0]
        want = {0: [0] * 20, 1: [0] + [1] * 19, 2: [0, 1] + [2] * 18}[good]
        assert [a for a, _ in pulls] == want
        seen.add(good)
    assert seen == {0, 1, 2}
    # one gen::<f64>() per pull, also at rate 0: 20 pulls x 2 words per trial
    assert np.all(agents.state()["pos"] == 6 * 40)


@pytest.mark.parametrize("rate", [0.0, 0.2, 1.0])
def test_tabular_q_against_the_oracles_agent(rate):
    """the default priors (0, 0.0), one observation, four actions, 200 steps against oracle_tabular_q_act /
    oracle_tabular_q_step_update: the same actions, values and counts bit for bit, the same Prng position"""
    k, steps = 4, 200
    q = C.c_void_p(L.oracle_tabular_q_new(1, k, 1.0, rate))
    mine = B.TabularQInner(k, rate, 0, 0.0)
    r_o, r_m, r_reward = O.Prng(), O.Prng(), O.Prng()
    for r, seed in ((r_o, 5), (r_m, 5), (r_reward, 6)):
        L.oracle_prng_seed_from_u64(C.byref(r), seed)
        L.oracle_prng_set_stream(C.byref(r), 3)
        L.oracle_prng_set_word_pos(C.byref(r), 0)
    vals, cnts = np.zeros((1, k)), np.zeros((1, k), np.uint64)
    actions = set()
    for t in range(steps):
        a_o = L.oracle_tabular_q_act(q, C.c_uint64(0), C.c_int(1), C.byref(r_o))
        a_m = mine.act(C.byref(r_m))
        assert a_o == a_m, t
        assert L.oracle_prng_word_pos(C.byref(r_o)) == L.oracle_prng_word_pos(C.byref(r_m)), t
        reward = 1.0 if L.oracle_prng_gen_bool(C.byref(r_reward), 0.2 + 0.2 * a_m) else 0.0
        L.oracle_tabular_q_step_update(q, 0, a_o, reward, O.TERMINATE, 0)
        mine.update(a_m, reward)
        L.oracle_tabular_q_read(q, O.f64p(vals), O.u64p(cnts))
        assert np.array_equal(vals[0], np.array(mine.values)) and list(cnts[0]) == mine.counts, t
        actions.add(a_m)
    L.oracle_tabular_q_free(q)
    if rate > 0.0:
        assert actions == set(range(k))  # (the comparison saw explored actions and their updates)
    assert L.oracle_prng_word_pos(C.byref(r_m)) >= 2 * steps
    if rate == 0.0:
        assert L.oracle_prng_word_pos(C.byref(r_m)) == 2 * steps


@pytest.mark.parametrize("kind, k, rate", [(B.UCB1, 3, None), (B.RANDOM, 2, None), (B.RANDOM, 4, None),
                                            (B.TABULAR_Q, 3, 0.0), (B.TABULAR_Q, 3, 0.2), (B.TABULAR_Q, 3, 1.0)])
def test_words_drawn_per_trial(kind, k, rate):
    """every restart step records action 0 and draws nothing; per trial of E pulls UCB1 draws no word, TABULAR_Q at
    least 2 E and exactly 2 E at rate 0.  RANDOM draws two words per ATTEMPT of gen_range: rand 0.8.5's sample_single
    accepts a u64 v when the low half of v * k is <= (k << leading_zeros(k)) - 1, which at k = 2 or 4 is 2^63 - 1 —
    half of all draws are rejected, so "exactly 2 E" does not hold even at a power of two.  The exact count is worked
    out here from the raw u64s of the lane's stream with that rule in Python integers: the words up to the E-th
    accepted attempt."""
    n, E, trials = 5, 6, 3
    raw = []
    for i in range(n):  # the lanes' actor streams, read from word 0 by a Prng of their own
        r = O.Prng()
        L.oracle_prng_seed_from_u64(C.byref(r), 10)
        L.oracle_prng_set_stream(C.byref(r), i)
        L.oracle_prng_set_word_pos(C.byref(r), 0)
        raw.append(r)
    zone = (k << (64 - k.bit_length())) - 1

    def words_of_pulls(i, pulls):
        words = 0
        while pulls > 0:
            v = int(L.oracle_prng_next_u64(C.byref(raw[i])))
            words += 2
            if (v * k) % (1 << 64) <= zone:
                pulls -= 1
        return words

    env = M.MetaLanes(n, k, E, M.UNIFORM_BERNOULLI, seed_env=9)
    agents = B.BanditAgentLanes(n, k, kind, exploration_rate=rate, seed_actor=10)
    before = agents.state()["pos"].astype(np.int64)
    for trial in range(trials):
        planes = agents.rollout(env, 2 * E - 1)
        assert np.all(planes["flag"][-1] == M.INTERRUPT)
        assert np.all(planes["action"][1::2] == 0)  # the restart steps
        assert np.all(planes["obs"][0, 1:-1:2] == 1.0)  # ... which are the steps that see a finished inner episode
        after = agents.state()["pos"].astype(np.int64)
        drawn = after - before
        before = after
        if kind == B.UCB1:
            assert np.all(drawn == 0)
        elif kind == B.RANDOM:
            assert list(drawn) == [words_of_pulls(i, E) for i in range(n)]
            assert np.all(drawn >= 2 * E) and np.all(drawn % 2 == 0)
        elif rate == 0.0:
            assert np.all(drawn == 2 * E)
        else:
            assert np.all(drawn >= 2 * E) and np.all(drawn % 2 == 0)
            if rate == 1.0:
                assert np.all(drawn >= 4 * E)  # every pull draws the f64 and then explores


# ------------------------------------------------------------------------------------------------ the library, no GPU
NEW_SYMBOLS = ["rl_bandit_agent_config_default", "rl_bandit_agent_create", "rl_bandit_agent_destroy",
               "rl_bandit_agent_rollout", "rl_bandit_agent_state_read"]


def test_library_exports_and_defaults():
    ra.build()
    lib = ra.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in ra.ABI_SYMBOLS, s
    assert (ra.BANDIT_AGENT_RANDOM, ra.BANDIT_AGENT_TABULAR_Q, ra.BANDIT_AGENT_UCB1) == (0, 1, 2)
    t = ra.bandit_agent_config_default(ra.BANDIT_AGENT_TABULAR_Q)  # TabularQLearningAgentConfig::default
    assert (t.kind, t.reserved, t.exploration_rate, t.initial_action_count, t.initial_action_value) == (1, 0, 0.2, 0, 0.0)
    u = ra.bandit_agent_config_default("ucb1")  # UCB1AgentConfig::default
    assert (u.kind, u.reserved, u.exploration_rate) == (2, 0, 0.2)
    r = ra.bandit_agent_config_default(ra.BANDIT_AGENT_RANDOM)
    assert (r.kind, r.reserved) == (0, 0)
    assert lib.rl_bandit_agent_config_default(C.c_int32(ra.BANDIT_AGENT_UCB1), None) == ra.ERR_INVALID_ARGUMENT
    cfg = ra.BanditAgentConfig()
    for bad in (-1, 3, 99):
        assert lib.rl_bandit_agent_config_default(C.c_int32(bad), C.byref(cfg)) == ra.ERR_INVALID_ARGUMENT
        assert b"unknown kind" in lib.rl_last_error(None)
    # NULL handles are refused before anything touches a device
    h = C.c_void_p()
    assert lib.rl_bandit_agent_create(None, C.byref(cfg), C.byref(h)) == ra.ERR_INVALID_ARGUMENT
    assert lib.rl_bandit_agent_rollout(None, None, None) == ra.ERR_INVALID_ARGUMENT
    assert lib.rl_bandit_agent_state_read(None, C.c_int32(0), None, C.c_uint64(0)) == ra.ERR_INVALID_ARGUMENT
    assert lib.rl_bandit_agent_destroy(None) == ra.OK
