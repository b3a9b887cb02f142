"""CPU checks of the meta-MDP lanes' reference (tests/meta_mdp_ref.py, imported unchanged: it takes any size) at the shapes
rl_env_create_meta_mdp_wide adds, and of the case tables of tests/meta_mdp_wide_cases.py that the GPU tests run:
lane g's first tables equal the host sampler rl_random_mdps_sample at stream = global lane through the library, at 10 x 5
and 9 x 2 and alpha 1, 0.5 and 2.5; the trial length; the 19-feature layout; the lane-range property; the tables' own
conditions, every sampled action's margin above MIN_MARGIN among them (printed); the binding's new surface; and the
bound on the env stream position, which grows faster on these lanes.  No device."""
import ctypes as C

import numpy as np
import pytest

import meta_mdp_ref as M
import meta_mdp_wide_cases as W
import relearn_amd as ra
import tabular_mdp_ref as T


@pytest.mark.parametrize("alpha", [1.0, 0.5, 2.5])
@pytest.mark.parametrize("S,A", [(10, 5), (9, 2)])
def test_first_tables_equal_the_host_sampler(S, A, alpha):
    d = M.dist(S, A, 2, 2, alpha=alpha, prior_mean=0.5, prior_stddev=2.0)
    cfg = ra.random_mdps_config_default()
    cfg.num_states, cfg.num_actions = S, A
    cfg.transition_prior_dirichlet_alpha, cfg.reward_prior_mean, cfg.reward_prior_stddev = alpha, 0.5, 2.0
    for g in (0, 25, 69):
        lane = M.MetaMdpLane(d, 77, g)
        tr, mean = ra.sample_random_mdp(cfg, seed=77, stream=g)
        assert np.array_equal(lane.cum, T.cumulative(tr)) and np.array_equal(lane.mean, mean), g
        assert lane.cum.shape == (S, A, S) and np.all(lane.cum[:, :, -1] == 1.0) and np.all(np.diff(lane.cum, axis=2) >= 0)


def test_trial_length_and_the_19_feature_layout():
    """[inner is None] [one-hot(state), 10] [prev is None] [one-hot(prev action), 5] [prev reward] [episode_done]"""
    S, A = 10, 5
    d = M.dist(S, A, 2, 2, reward_stddev=0.5)
    lanes = M.MetaMdpLanes(40, d, seed_env=9)
    D = S + A + 4
    assert D == 19 == lanes.D and M.trial_steps(d) == 5 and M.trial_steps(M.dist(S, A, 10, 10)) == 109
    start = np.zeros(D, np.float32)
    start[1] = 1.0       # state 0
    start[1 + S] = 1.0   # prev is None; the A + 1 entries behind the marker are zero
    assert np.array_equal(lanes.observe(), np.repeat(start[:, None], 40, axis=1))
    acts = (np.arange(40) % A).astype(np.uint8)
    r1, f1, o1, _ = lanes.step(acts)
    assert np.all(f1 == M.CONTINUE) and np.all(o1[0] == 0) and np.all(o1[D - 1] == 0) and np.all(o1[1 + S] == 0)
    assert np.array_equal(o1[2 + S:2 + S + A].argmax(0), acts) and np.array_equal(o1[D - 2], r1)
    assert np.all(o1[1:1 + S].sum(0) == 1) and o1[1:1 + S].argmax(0).max() >= 8  # a state the 8-float row has no place for
    r2, f2, o2, _ = lanes.step(acts)  # the inner limit's Interrupt(state): the one-hot stays, episode_done shows
    assert np.all(f2 == M.CONTINUE) and np.all(o2[D - 1] == 1) and np.all(o2[1:1 + S].sum(0) == 1)
    r3, f3, o3, _ = lanes.step(acts)  # the restart
    assert np.all(r3 == 0) and np.array_equal(o3, np.repeat(start[:, None], 40, axis=1))
    lanes.step(acts)
    r5, f5, o5, term = lanes.step(acts)
    assert np.all(f5 == M.INTERRUPT) and np.all(term[D - 1] == 1) and np.array_equal(term[D - 2], r5)
    assert np.array_equal(o5, np.repeat(start[:, None], 40, axis=1))


def test_lane_range_property():
    """offset 25 gives lanes 25..69 of a 70-lane run"""
    c = W.DRIVEN[0]
    ref = W.driven_reference(c)
    tail = M.MetaMdpLanes(W.N_LANES - W.OFFSET, c.dist, lane_offset=W.OFFSET, seed_env=c.seed)
    assert np.array_equal(tail.observe(), ref.observe0[:, W.OFFSET:])
    assert np.array_equal(tail.tables()[0], ref.tables0[0][W.OFFSET:])
    for a, (reward, flag, obs, term, tables) in zip(ref.actions, ref.steps):
        r, f, o, t = tail.step(a[W.OFFSET:])
        assert np.array_equal(r, reward[W.OFFSET:]) and np.array_equal(f, flag[W.OFFSET:])
        assert np.array_equal(o, obs[:, W.OFFSET:]) and np.array_equal(t, term[:, W.OFFSET:])
        assert np.array_equal(tail.tables()[0], tables[0][W.OFFSET:])


@pytest.mark.parametrize("c", W.DRIVEN, ids=W.driven_id)
def test_driven_cases_hold_their_own_conditions(c):
    d = c.dist
    assert 2 <= d.S <= 10 and 2 <= d.A <= 8 and d.S + d.A + 4 <= 20 and (d.S > 8 or d.S + d.A + 4 > 16)
    ref = W.driven_reference(c)
    assert len(ref.steps) == W.TRIALS * M.trial_steps(d) + 1
    flags = np.array([s[1] for s in ref.steps])
    assert (flags == M.INTERRUPT).sum(0).min() >= W.TRIALS and not (flags == M.TERMINATE).any()
    assert sorted(np.unique(np.array(ref.actions))) == list(range(d.A))
    tables = [ref.tables0] + [s[4] for s in ref.steps]
    for t in range(len(ref.steps)):  # the tables change exactly where a trial ends, in every lane
        changed = np.any(tables[t + 1][1] != tables[t][1], axis=(1, 2))
        assert np.array_equal(changed, flags[t] == M.INTERRUPT), t
    # every state is reached — the ninth and tenth among them (where a trial ends the successor shows in term_obs alone)
    states = np.array([np.where(s[1] == M.INTERRUPT, s[3][1:1 + d.S].argmax(0), s[2][1:1 + d.S].argmax(0))
                       for s in ref.steps])
    assert len(np.unique(states)) == d.S


def test_cases_cover_the_issue():
    assert set(W.SHAPES) == {(10, 5), (9, 2), (10, 6), (8, 8)}
    assert {(c.dist.S, c.dist.A) for c in W.DRIVEN} == set(W.SHAPES)
    assert {c.dist.alpha for c in W.DRIVEN} == {1.0, 0.5, 2.5} and any(c.dist.reward_stddev == 0.0 for c in W.DRIVEN)
    assert (W.N_LANES, W.OFFSET) == (70, 25) and W.TRIALS >= 3
    at_default = [c for c in W.CLOSED if (c.dist.S, c.dist.A) == (10, 5)]
    assert {(c.net.cell, c.net.H2 == 0) for c in at_default} == {("gru", True), ("gru", False), ("lstm", True), ("lstm", False)}
    assert {(c.n, c.offset) for c in at_default} == {(70, 0), (45, 25)} and all(c.net.H == 8 and c.T == 7 for c in W.CLOSED)
    assert {(c.dist.S, c.dist.A) for c in W.CLOSED} == {(10, 5), (9, 2), (10, 6)} and W.FUSED == [(10, 5)]


@pytest.mark.parametrize("c", W.CLOSED, ids=W.closed_id)
def test_closed_loop_cases_hold_their_own_conditions(c):
    """no sample is excused: every sampled action's uniform is further than MIN_MARGIN from every cumulative boundary"""
    ref = W.closed_reference(c)
    print("%s: smallest margin %.3g" % (W.closed_id(c), ref.margin))
    assert ref.margin > M.MIN_MARGIN == 1e-5
    d = c.dist
    assert (c.net.D, c.net.A) == (d.S + d.A + 4, d.A)
    length = M.trial_steps(d)
    assert c.T % length != 0  # a trial runs across the two collections
    want = M.expected_interrupts(c)
    assert want[0] and want[1]
    for p, planes in enumerate(ref.periods):
        cut = planes["flag"] == M.INTERRUPT
        assert np.array_equal(cut, np.repeat(np.isin(np.arange(c.T), want[p])[:, None], c.n, axis=1)), p
    action = np.concatenate([p["action"] for p in ref.periods])
    assert sorted(np.unique(action)) == list(range(d.A))
    states = np.concatenate([p["obs"][1:1 + d.S].argmax(0).ravel() for p in ref.periods])
    assert states.max() >= 8  # the states beyond the 8-float row are visited


def test_env_stream_position_round_trips_through_its_f64_plane():
    """env_pos lives in an f64 plane: exact below 2^53 words.  A 10 x 5 trial at alpha 1 reads 500 Gamma draws of 2 words,
    50 normals of 4 words per attempt and, per live step, 2 words and a normal: measured here over many trials, then bounded.
    The worst case of a trial, every sampler at its attempt limit (64 attempts; a Marsaglia-Tsang attempt is a normal of at
    most 64 attempts of 4 words, and 2 words; below alpha 1 two more words): 550 * (64 * 258 + 2) + 100 * 258 < 9.2e6 words,
    so 2^53 words outlast 9.7e8 worst-case trials, and 4e12 trials at the measured rate."""
    d = M.dist(10, 5, 10, 10)
    lane = M.MetaMdpLane(d, 5, 3)
    rs = np.random.default_rng(0)
    trials = 40
    for _ in range(trials):
        for _t in range(M.trial_steps(d)):
            _r, f = lane.step(int(rs.integers(0, 5)))
        assert f == M.INTERRUPT
        lane.reset()
    pos = word_pos(lane.rng)
    per_trial = pos / (trials + 1)
    print("env stream: %d words after %d trials, %.0f per trial" % (pos, trials + 1, per_trial))
    assert pos % 2 == 0 and float(pos) == pos and int(np.float64(pos)) == pos
    assert 1500 < per_trial < 3000  # about 2,000 words per trial: 2^53 / 3000 > 3e12 trials
    assert 550 * (64 * 258 + 2) + 100 * 258 < 9.2e6 and (1 << 53) / 9.2e6 > 9.7e8


def word_pos(rng):
    """the next unread word of an oracle Prng, found by search: the generator set to a position draws what `rng` draws"""
    import oracle as O
    L = O.lib()
    probe = O.Prng()
    C.memmove(C.byref(probe), C.byref(rng), C.sizeof(O.Prng))
    want = [L.oracle_prng_next_u32(C.byref(probe)) for _ in range(4)]
    for pos in range(0, 400000, 2):
        L.oracle_prng_set_word_pos(C.byref(probe), pos)
        if L.oracle_prng_next_u32(C.byref(probe)) == want[0]:
            L.oracle_prng_set_word_pos(C.byref(probe), pos)
            if [L.oracle_prng_next_u32(C.byref(probe)) for _ in range(4)] == want:
                return pos
    raise AssertionError("position not found")


def test_binding_declares_the_new_surface():
    for name in ("rl_env_create_meta_mdp_wide", "rl_rnn_chain_create_wide20", "rl_traj_create_wide"):
        assert name in ra.ABI_SYMBOLS and hasattr(ra.lib(), name)
    assert issubclass(ra.MetaMdpEnvWide, ra.MetaMdpEnv) and ra.MetaMdpEnvWide.CREATE == "rl_env_create_meta_mdp_wide"
    assert ra.RnnChainWide20.CREATE == "rl_rnn_chain_create_wide20" and ra.TrajectoryWide.CREATE == "rl_traj_create_wide"
    assert ra.lib().rl_abi_version() == 6
    m = ra.meta_mdp_config_default()  # the older default stays: five states
    assert (m.n_states, m.n_actions) == (5, 5)
