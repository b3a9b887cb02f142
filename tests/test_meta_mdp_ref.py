"""CPU checks of the meta-MDP lanes' reference (tests/meta_mdp_ref.py) and of the cases the GPU tests run against it:
a lane's first tables equal the host sampler rl_random_mdps_sample at stream = global lane (through the library, bit for
bit); the trial length; the feature layout at an inner Interrupt and at a restart; the lane-range property; and the case
tables' own conditions, the margin of every sampled action among them.  No device."""
import numpy as np
import pytest

import meta_mdp_ref as M
import relearn_amd as ra
import tabular_mdp_ref as T


@pytest.mark.parametrize("alpha", [1.0, 0.5, 2.5])
@pytest.mark.parametrize("S,A", [(2, 2), (5, 5), (8, 4), (4, 8)])
def test_first_tables_equal_the_host_sampler(S, A, alpha):
    """lanes are keyed by seed_from_u64(seed_env) and stream = global lane: at stream position 0 lane g's first trial is
    rl_random_mdps_sample(cfg, seed_env, stream = g)"""
    d = M.dist(S, A, 2, 2, alpha=alpha, prior_mean=0.5, prior_stddev=2.0)
    cfg = ra.random_mdps_config_default()
    cfg.num_states, cfg.num_actions = S, A
    cfg.transition_prior_dirichlet_alpha, cfg.reward_prior_mean, cfg.reward_prior_stddev = alpha, 0.5, 2.0
    for g in (0, 1, 25, 69):
        lane = M.MetaMdpLane(d, 77, g)
        tr, mean = ra.sample_random_mdp(cfg, seed=77, stream=g)
        assert np.array_equal(lane.cum, T.cumulative(tr)) and np.array_equal(lane.mean, mean), g
        assert np.all(lane.cum[:, :, -1] == 1.0) and np.all(np.diff(lane.cum, axis=2) >= 0)
    # the second trial continues the stream: it is not the first trial of any of these streams
    lane = M.MetaMdpLane(d, 77, 0)
    first = lane.cum.copy()
    lane.reset()
    assert not np.array_equal(lane.cum, first)


@pytest.mark.parametrize("E,L", [(1, 1), (2, 3), (3, 4), (5, 1)])
def test_trial_length_and_flags(E, L):
    d = M.dist(3, 2, E, L)
    lanes = M.MetaMdpLanes(4, d, seed_env=5)
    length = M.trial_steps(d)
    assert length == E * (L + 1) - 1
    flags = np.array([lanes.step(np.zeros(4, np.uint8))[1] for _ in range(3 * length)])
    want = np.where((np.arange(3 * length) + 1) % length == 0, M.INTERRUPT, M.CONTINUE)
    assert np.array_equal(flags, np.repeat(want[:, None], 4, axis=1))
    assert [lane.trials for lane in lanes.lanes] == [4] * 4


def test_feature_layout_at_an_inner_interrupt_and_at_a_restart():
    """[inner is None] [one-hot(state), S] [prev is None] [one-hot(prev action), A] [prev reward] [episode_done]"""
    S, A = 3, 2
    d = M.dist(S, A, 2, 2, reward_stddev=0.5)
    lanes = M.MetaMdpLanes(40, d, seed_env=9)
    D = S + A + 4
    start = np.zeros(D, np.float32)
    start[1] = 1.0      # state 0
    start[1 + S] = 1.0  # prev is None; the A + 1 entries behind the marker are zero
    assert np.array_equal(lanes.observe(), np.repeat(start[:, None], 40, axis=1))
    acts = (np.arange(40) % A).astype(np.uint8)
    r1, f1, o1, _ = lanes.step(acts)  # inner step 1 of 2
    assert np.all(f1 == M.CONTINUE) and np.all(o1[0] == 0) and np.all(o1[D - 1] == 0) and np.all(o1[1 + S] == 0)
    assert np.array_equal(o1[2 + S:2 + S + A].argmax(0), acts) and np.array_equal(o1[D - 2], r1)
    assert np.all(o1[1:1 + S].sum(0) == 1)
    r2, f2, o2, _ = lanes.step(acts)  # inner step 2 of 2: the limit's Interrupt(state) — the state's one-hot stays
    assert np.all(f2 == M.CONTINUE) and np.all(o2[0] == 0) and np.all(o2[D - 1] == 1)
    assert np.all(o2[1:1 + S].sum(0) == 1) and len(set(o2[1:1 + S].argmax(0))) > 1
    assert np.array_equal(o2[D - 2], r2) and np.all(o2[1 + S] == 0)
    r3, f3, o3, _ = lanes.step(1 - acts)  # the restart: action ignored, reward 0, prev None, state 0, nothing drawn
    assert np.all(r3 == 0) and np.all(f3 == M.CONTINUE) and np.array_equal(o3, np.repeat(start[:, None], 40, axis=1))
    lanes.step(acts)
    r5, f5, o5, term = lanes.step(acts)  # the trial's last step: an Interrupt, term_obs shows the done inner episode
    assert np.all(f5 == M.INTERRUPT) and np.all(term[D - 1] == 1) and np.array_equal(term[D - 2], r5)
    assert np.all(term[1:1 + S].sum(0) == 1) and np.array_equal(o5, np.repeat(start[:, None], 40, axis=1))


def test_lane_range_property():
    """offset 25 gives lanes 25..69 of a 70-lane run"""
    c = M.DRIVEN[1]
    ref = M.driven_reference(c)
    tail = M.MetaMdpLanes(M.N_LANES - M.OFFSET, c.dist, lane_offset=M.OFFSET, seed_env=c.seed)
    assert np.array_equal(tail.observe(), ref.observe0[:, M.OFFSET:])
    assert np.array_equal(tail.tables()[0], ref.tables0[0][M.OFFSET:])
    for a, (reward, flag, obs, term, tables) in zip(ref.actions, ref.steps):
        r, f, o, t = tail.step(a[M.OFFSET:])
        assert np.array_equal(r, reward[M.OFFSET:]) and np.array_equal(f, flag[M.OFFSET:])
        assert np.array_equal(o, obs[:, M.OFFSET:]) and np.array_equal(t, term[:, M.OFFSET:])
        assert np.array_equal(tail.tables()[1], tables[1][M.OFFSET:])


@pytest.mark.parametrize("c", M.DRIVEN, ids=M.driven_id)
def test_driven_cases_hold_their_own_conditions(c):
    d = c.dist
    assert 2 <= d.S <= 8 and 2 <= d.A <= 8 and d.S + d.A + 4 <= 16
    ref = M.driven_reference(c)
    assert len(ref.steps) >= M.TRIALS * M.trial_steps(d) + 1
    flags = np.array([s[1] for s in ref.steps])
    assert (flags == M.INTERRUPT).sum(0).min() >= M.TRIALS and not (flags == M.TERMINATE).any()
    assert sorted(np.unique(np.array(ref.actions))) == list(range(d.A))
    tables = [ref.tables0] + [s[4] for s in ref.steps]
    for t in range(len(ref.steps)):  # the tables change exactly where a trial ends, in every lane
        changed = np.any(tables[t + 1][1] != tables[t][1], axis=(1, 2))
        assert np.array_equal(changed, flags[t] == M.INTERRUPT), t
    rewards = np.array([s[0] for s in ref.steps])
    live = rewards != 0
    if d.reward_stddev == 0.0:  # rewards are table entries: the mean of the row stepped from
        means = np.stack([tb[1] for tb in tables[:-1]])  # [t][n][S][A]
        assert np.all(np.isin(rewards[live], means.astype(np.float32)))
    assert live.mean() > 0.4
    # every state is reached (where a trial ends the successor state shows in term_obs alone)
    states = np.array([np.where(s[1] == M.INTERRUPT, s[3][1:1 + d.S].argmax(0), s[2][1:1 + d.S].argmax(0))
                       for s in ref.steps])
    assert len(np.unique(states)) == d.S


def test_driven_cases_cover_the_issue():
    shapes = [(c.dist.S, c.dist.A, c.dist.E, c.dist.L) for c in M.DRIVEN]
    for want in [(2, 2, 1, 1), (3, 2, 2, 3), (5, 5, 3, 4), (8, 4, 2, 2), (4, 8, 2, 2)]:
        assert want in shapes
    by = {(c.dist.S, c.dist.A): c.dist for c in M.DRIVEN if c.dist.reward_stddev != 0}
    assert by[(5, 5)].alpha == 1.0 and by[(5, 5)].reward_stddev == 1.0
    assert by[(8, 4)].alpha == 0.5 and by[(4, 8)].alpha == 2.5
    assert any(c.dist.reward_stddev == 0.0 for c in M.DRIVEN)
    assert (M.N_LANES, M.OFFSET) == (70, 25) and M.TRIALS >= 3


@pytest.mark.parametrize("c", M.CLOSED, ids=M.closed_id)
def test_closed_loop_cases_hold_their_own_conditions(c):
    """no sample is excused: every sampled action's uniform is further than MIN_MARGIN from every cumulative boundary"""
    ref = M.closed_reference(c)
    print("%s: margin %.3g" % (M.closed_id(c), ref.margin))
    assert ref.margin > M.MIN_MARGIN
    d = c.dist
    length = M.trial_steps(d)
    assert c.T % length != 0  # a trial runs across the two collections
    want = M.expected_interrupts(c)
    assert any(want) and want[1] and (want[1][0] + 1 + c.T) % length == 0
    for p, planes in enumerate(ref.periods):
        cut = planes["flag"] == M.INTERRUPT
        assert np.array_equal(cut, np.repeat(np.isin(np.arange(c.T), want[p])[:, None], c.n, axis=1)), p
        assert not (planes["flag"] == M.TERMINATE).any()
        assert np.all(planes["obs"][0] == 0)
    action = np.concatenate([p["action"] for p in ref.periods])
    if c.n >= 45:
        assert sorted(np.unique(action)) == list(range(d.A))


def test_closed_loop_cases_cover_the_issue():
    shapes = {(c.dist.S, c.dist.A) for c in M.CLOSED}
    assert shapes == {(2, 2), (3, 2), (4, 3), (5, 5), (8, 4), (4, 8), (3, 3)}
    assert {c.net.cell for c in M.CLOSED} == {"gru", "lstm"} and {c.net.H2 == 0 for c in M.CLOSED} == {True, False}
    assert {1, 64, 65, 130} <= {c.n for c in M.CLOSED} and any(c.offset for c in M.CLOSED)


def test_dynamic_programming_over_read_back_tables():
    """the optimum of a lane is at least the uniform policy's value, and both are E times one inner episode's"""
    d = M.dist(4, 3, 3, 5)
    lane = M.MetaMdpLane(d, 3, 0)
    opt, uni = M.optimal_and_uniform_values(lane.cum, lane.mean, d)
    assert opt > uni
    one = M.optimal_and_uniform_values(lane.cum, lane.mean, d._replace(E=1))
    assert abs(opt - 3 * one[0]) < 1e-12 and abs(uni - 3 * one[1]) < 1e-12


def test_binding_declares_the_new_surface():
    import ctypes as C
    assert ra.ENV_META_MDP == 6
    for name in ("rl_meta_mdp_config_default", "rl_env_create_meta_mdp", "rl_env_meta_mdp_read_tables"):
        assert name in ra.ABI_SYMBOLS and hasattr(ra.lib(), name)
    m = ra.meta_mdp_config_default()
    assert (m.n_states, m.n_actions, m.alpha, m.reward_prior_mean, m.reward_prior_stddev, m.reward_stddev,
            m.discount_factor, m.max_inner_steps, m.episodes_per_trial) == (5, 5, 1.0, 1.0, 1.0, 1.0, 1.0, 10, 10)
    assert C.sizeof(ra.MetaMdpConfig) == 64
    assert ra.lib().rl_meta_mdp_config_default(None) == ra.ERR_INVALID_ARGUMENT
    assert ra.lib().rl_abi_version() == 6
