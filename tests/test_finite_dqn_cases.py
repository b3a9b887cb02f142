"""tests/finite_dqn_cases.py and tests/finite_dqn_ref.py — the case table of DQN over 3 to 8 actions and its restatement —
checked on the CPU, so that tests/test_gpu_finite_dqn.py leaves no step out of a comparison.  CPU only.

(a) for every collection case the gap between the largest and the second-largest action value is at least MARGIN (the bar
    and the reason of tests/test_gpu_dqn_index_envs.py): feed-forward modules on the f64 network at every observation the
    env can emit, and every case on every greedy step of the restated closed loops at eps = 0.5 and 0;
(b) over the table every action index of every A is a greedy action at least once and an explored one at least once;
(c) the restated gen_range(0..A) is the oracle's, uses every value of every A of the table within 10,000 draws, and at
    A = 2 consumes exactly the words of the two-action restatement (oracle_prng_gen_range_u64(0, 2), as
    tests/test_gpu_dqn_index_envs.py and tests/recurrent_dqn_ref.py draw it);
(d) the restated k-armed bandit lanes are the oracle's at two arms;
(e) the collections end mid-episode where the table says so."""
import ctypes as C

import numpy as np
import pytest

import finite_dqn_cases as FC
import finite_dqn_ref as F
import oracle as O
import recurrent_dqn_ref as R


@pytest.mark.parametrize("case", FC.COLLECT_CASES, ids=FC.case_id)
def test_margin_at_every_greedy_step(case):
    e = FC.ENVS[case.env]
    if not FC.is_recurrent(case):
        from test_gpu_general_mlp import forward64, unflatten
        hidden, act = FC.FF_MODULES[case.module]
        z, _ = forward64(unflatten(F.case_params(case), e.D, hidden, e.A), F.possible_observations(case.env), act,
                         "Identity")
        assert z.shape[1] == e.A and F.top_gap(z.T).min() >= FC.MARGIN
    loops = F.case_loops(case)
    for eps, loop in loops.items():
        assert loop.margin >= FC.MARGIN, (eps, loop.margin)
        # the first collection's 9 steps end mid-episode on every lane of a MemoryGame; the bandit's never do
        assert loop.cuts[0] == (0 if e.kind == "bandit" else case.n), loop.cuts
        assert (loop.cuts[1] > 0) == ((e.warm + sum(FC.HORIZONS)) % e.ep_len != 0)
    assert loops[0.0].explored.sum() == 0 and loops[0.0].greedy.sum() == case.n * sum(FC.HORIZONS)
    assert min(loops[0.5].explored.sum(), loops[0.5].greedy.sum()) > 0.3 * case.n * sum(FC.HORIZONS)


def test_every_action_is_greedy_and_explored_somewhere():
    counts = {}
    for case in FC.COLLECT_CASES:
        A = FC.ENVS[case.env].A
        g, x = counts.setdefault(A, (np.zeros(A, dtype=np.int64), np.zeros(A, dtype=np.int64)))
        for loop in F.case_loops(case).values():
            g += loop.greedy
            x += loop.explored
    assert sorted(counts) == [3, 4, 5, 7, 8]
    for A, (g, x) in counts.items():
        assert g.min() > 0, (A, g)
        assert x.min() > 0, (A, x)


def fresh(stream=3):
    return R.actor_streams(stream + 1, FC.SEEDS["seed_actor"])[stream]


@pytest.mark.parametrize("A", [2, 3, 4, 5, 6, 7, 8])
def test_gen_range_is_the_oracles(A):
    L = O.lib()
    mine, theirs = fresh(), fresh()
    got = [F.gen_range(mine, A) for _ in range(10000)]
    want = [L.oracle_prng_gen_range_u64(C.byref(theirs), 0, A) for _ in range(10000)]
    assert got == want and sorted(set(got)) == list(range(A))
    assert L.oracle_prng_word_pos(C.byref(mine)) == L.oracle_prng_word_pos(C.byref(theirs))
    # (sample_single's zone is the conservative one: a draw is rejected with probability 1 - A / 2^ceil(log2(A + 1)), so
    # the positions are far beyond two words per draw and the retry loop is exercised at every A)
    assert L.oracle_prng_word_pos(C.byref(mine)) > 22000


def test_two_action_draws_consume_the_same_words():
    """DqnActor::act at A = 2, draw by draw beside the existing restatement: the same decisions, actions and positions"""
    L = O.lib()
    mine, theirs = fresh(5), fresh(5)
    for _ in range(2000):
        a, b = L.oracle_prng_gen_bool(C.byref(mine), 0.5), L.oracle_prng_gen_bool(C.byref(theirs), 0.5)
        assert a == b
        if a:
            assert F.gen_range(mine, 2) == L.oracle_prng_gen_range_u64(C.byref(theirs), 0, 2)
        assert L.oracle_prng_word_pos(C.byref(mine)) == L.oracle_prng_word_pos(C.byref(theirs))


def test_restated_bandit_lanes_are_the_oracles_at_two_arms():
    values, n = (0.25, 1.5), 7
    mine, theirs = F.KBanditLanes(n, values), O.BanditLaneSim(n, values, **FC.SEEDS)
    rng = np.random.default_rng(1)
    assert mine.D == theirs.D and np.array_equal(mine.observe(), theirs.observe())
    for _ in range(5):
        a = rng.integers(0, 2, size=n).astype(np.uint8)
        for x, y in zip(mine.step(a), theirs.step(a)):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        for x, y in zip(mine.get_state(), theirs.get_state()):
            assert np.array_equal(x, y)


def test_table_shapes():
    """what the table is meant to cover"""
    assert {FC.ENVS[c.env].A for c in FC.COLLECT_CASES} == {3, 4, 5, 7, 8}
    assert {FC.ENVS[c.env].D for c in FC.COLLECT_CASES} == {4, 5, 8}
    assert {c.n for c in FC.REC_CASES} == {200, 64} and {c.n for c in FC.FF_CASES} == {200}
    assert {c.module for c in FC.FF_CASES} == set(FC.FF_MODULES) and {c.module for c in FC.REC_CASES} == set(FC.REC_MODULES)
    for name, e in FC.ENVS.items():
        sim = F.make_sim(name, 3)
        assert sim.D == e.D and F.possible_observations(name).shape[1] == e.D
        if e.kind == "memory":
            assert e.D == e.k + e.h + (1 if e.limit else 0) and e.A == e.k
            assert e.ep_len == (min(e.limit, e.h + 1) if e.limit else e.h + 1)
    for c in FC.MINIBATCH_CASES + FC.STEP_CASES:
        assert c in FC.COLLECT_CASES


def test_target_restatements():
    assert np.allclose(F.reward_to_go([1.0, 2.0, 4.0], 0.5), [3.0, 4.0, 4.0])
    flags = np.array([O.CONTINUE, O.INTERRUPT, O.TERMINATE])
    assert np.allclose(F.td_targets(np.array([1.0, 2.0, 3.0]), [1.0, 1.0, 1.0], flags, 0.5), [1.5, 2.0, 1.0])
