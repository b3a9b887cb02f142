"""rl_gae, rl_reward_to_go and the value targets of rl_values_opt_update on every critic path, bit for bit against the
oracle, on the histories of tests/advantage_cases.py: episode ends placed at t = T-1 (each successor code), t = 0 and
either side of the scans' 16-step batch boundary; T below, at and just over one batch; a patterned lane in a second and
a third 64-thread workgroup; term_obs poisoned wherever no Interrupt stands.

  fused      ra.Mlp(engine, 5 | 4, 128, 1): k_mlp_forward_rows, k_gae_scan<5> / <4> (and its rtg_only branch),
             k_value_targets_td<5> / <4>, k_value_targets_rtg — held to oracle_lanes_gae / oracle_lanes_one_step_targets
  general    launch_gen_values (k_gen_any_interrupt, k_gen_chain_rows at kernel variant 0, the per-layer k_gen_dense with
             its skip argument at variant 1, k_gen_successor_values), then k_seq_gae / k_seq_value_targets_td — held to
             oracle_mlp_layers_forward -> successors -> oracle_seq_gae / oracle_seq_one_step_targets
  recurrent  the teacher-forced forward's outputs (bit-exact against the oracle elsewhere) -> k_seq_gae /
             k_seq_value_targets_td — held to the oracle's array-fed scans on those outputs

Slot T of RL_TRAJ_VALUES is V(obs[T]) of every lane for feed-forward critics, whatever ended step T-1; for recurrent
critics it is what step T-1 bootstrapped from (include/relearn_hip.h).

The tile kernels of the default GruMlp / LstmMlp take lane counts that are multiples of 32 (seq_ensure refuses others), so
those modules run at (32, 1) and (96, 17) — one workgroup of the scan half full, and a second one — and the shapes (1, 1)
and (65, 17) themselves on two-layer chains, whose lane-per-thread kernels take any lane count and feed the same scans."""
import numpy as np
import pytest

import advantage_cases as ac
import oracle as O
import relearn_amd as ra

pytestmark = pytest.mark.gpu

SHAPE_IDS = [ac.shape_id(s) for s in ac.SHAPES]
VARIANTS = pytest.mark.parametrize("variant", [0, 1], ids=["kernels-best", "kernels-v1"])


def planes(traj, *fields):
    out = [traj.read(f) for f in fields]
    for a in out:
        assert not np.isnan(a).any()  # no poison in a compared plane
    return out


def td_update(critic, traj, target, discount, p0):
    """one optimisation step of rl_values_opt_update from the parameters p0 (the targets come from the critic as it
    stands before the step)"""
    critic.set_params(p0)
    cfg = ra.values_opt_config_default()
    cfg.opt_steps_per_update, cfg.target, cfg.discount_factor = 1, target, discount
    st, losses = ra.values_opt_update(critic, ra.Adam(critic), traj, cfg, want_losses=True)
    assert st.steps == 1 and np.isfinite(losses).all()
    critic.set_params(p0)


def loaded(engine, hist):
    D, T1, n = hist["obs"].shape
    traj = ra.Trajectory(engine, n, T1 - 1, D)
    traj.write_all(hist)
    return traj


# ---------------------------------------------------------------- fused critics
_fused = {}


def fused_expectation(D, shape, pattern_set, cp):
    key = (D, shape, pattern_set)
    if key not in _fused:
        cs, h = O.MlpShape(D, 128, 1), ac.history(D, shape, pattern_set)
        values, adv, rtg = O.lanes_gae(cs, cp, h, ac.GAMMA, ac.LAMBDA)
        _fused[key] = dict(params=cp.copy(), values=values, adv=adv, rtg=rtg,
                           td=O.lanes_one_step_targets(cs, cp, h, np.float32(ac.TD_GAMMA)),
                           rtg_td=O.lanes_gae(cs, cp, h, ac.TD_GAMMA, ac.LAMBDA)[2])
    assert np.array_equal(_fused[key]["params"], cp)
    return _fused[key]


@VARIANTS
@pytest.mark.parametrize("shape", ac.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("D", [5, 4])
def test_fused_critic(engine, D, shape, variant):
    n, T = shape
    engine.set_kernel_variant(variant)
    try:
        critic = ra.Mlp(engine, D, 128, 1)
        critic.init(3)
        p0 = critic.get_params()
        for pattern_set in ("base", "no_interrupt"):
            h = ac.history(D, shape, pattern_set)
            e = fused_expectation(D, shape, pattern_set, p0)
            traj = loaded(engine, h)
            ra.gae(traj, critic, ac.GAMMA, ac.LAMBDA)
            values, adv, rtg = planes(traj, ra.TRAJ_VALUES, ra.TRAJ_ADVANTAGES, ra.TRAJ_RETURNS)
            assert np.array_equal(values[:T], e["values"][:T])
            assert np.array_equal(values[T], e["values"][T])  # slot T: V(obs[T]) of every lane
            assert np.array_equal(adv, e["adv"]) and np.array_equal(rtg, e["rtg"])
            # RewardToGo targets: at rl_gae's discount the return plane itself, at another a scan of their own
            td_update(critic, traj, ra.VALUE_TARGET_REWARD_TO_GO, ac.GAMMA, p0)
            assert np.array_equal(planes(traj, ra.TRAJ_TARGETS)[0], e["rtg"])
            td_update(critic, traj, ra.VALUE_TARGET_REWARD_TO_GO, ac.TD_GAMMA, p0)
            assert np.array_equal(planes(traj, ra.TRAJ_TARGETS)[0], e["rtg_td"])
            assert np.array_equal(e["rtg_td"], ac.returns_f32(h, ac.TD_GAMMA))
            # One-step TD: targets and the refreshed value plane, slot T included
            traj.write(ra.TRAJ_VALUES, np.full((T + 1, n), 7.0, np.float32))
            td_update(critic, traj, ra.VALUE_TARGET_ONE_STEP_TD, ac.TD_GAMMA, p0)
            tgt, values = planes(traj, ra.TRAJ_TARGETS, ra.TRAJ_VALUES)
            assert np.array_equal(tgt, e["td"]) and np.array_equal(values, e["values"])
            # the RewardToGo critic (k_gae_scan's rtg_only branch): the "advantage" is the return
            ra.reward_to_go(traj, ac.GAMMA)
            adv, rtg = planes(traj, ra.TRAJ_ADVANTAGES, ra.TRAJ_RETURNS)
            assert np.array_equal(adv, e["rtg"]) and np.array_equal(rtg, e["rtg"])
    finally:
        engine.set_kernel_variant(0)


# ---------------------------------------------------------------- general critics
_general = {}


def make_general(engine, spec):
    D, hidden, act, bias = spec
    critic = ra.Mlp(engine, D, hidden, 1, act, "Identity", bias=bias)
    critic.init(22)
    assert critic.P == ac.general_num_params(spec)
    return critic, critic.get_params()


def general_expectation(spec, shape, pattern_set, p0):
    key = (ac.general_id(spec), shape, pattern_set)
    if key not in _general:
        h = ac.history(spec[0], shape, pattern_set)
        e = ac.general_expectation(spec, p0, h)
        e["params"], e["rtg_td"] = p0.copy(), ac.returns_f32(h, ac.TD_GAMMA)
        _general[key] = e
    assert np.array_equal(_general[key]["params"], p0)
    return _general[key]


def general_calls(critic, p0, traj, T):
    """the calls of one case on a loaded trajectory -> every plane they leave"""
    got = {}
    ra.gae(traj, critic, ac.GAMMA, ac.LAMBDA)
    got["values"], got["adv"], got["rtg"] = planes(traj, ra.TRAJ_VALUES, ra.TRAJ_ADVANTAGES, ra.TRAJ_RETURNS)
    # RewardToGo targets at rl_gae's own discount: the array-fed scan's return plane is not vouched for (rtg_scan_valid
    # stays false), so they are scanned again — and equal it; then at another discount
    td_update(critic, traj, ra.VALUE_TARGET_REWARD_TO_GO, ac.GAMMA, p0)
    got["tgt_rtg"] = planes(traj, ra.TRAJ_TARGETS)[0]
    td_update(critic, traj, ra.VALUE_TARGET_REWARD_TO_GO, ac.TD_GAMMA, p0)
    got["tgt_rtg_td"] = planes(traj, ra.TRAJ_TARGETS)[0]
    traj.write(ra.TRAJ_VALUES, np.full((T + 1, traj.n), 7.0, np.float32))
    td_update(critic, traj, ra.VALUE_TARGET_ONE_STEP_TD, ac.TD_GAMMA, p0)
    got["td"], got["td_values"] = planes(traj, ra.TRAJ_TARGETS, ra.TRAJ_VALUES)
    return got


def check_general(got, e, T):
    assert np.array_equal(got["values"][:T], e["values"][:T])
    assert np.array_equal(got["adv"], e["adv"]) and np.array_equal(got["rtg"], e["rtg"])
    assert np.array_equal(got["tgt_rtg"], e["rtg"]) and np.array_equal(got["tgt_rtg_td"], e["rtg_td"])
    assert np.array_equal(got["td"], e["td"]) and np.array_equal(got["td_values"][:T], e["values"][:T])


@VARIANTS
@pytest.mark.parametrize("shape", ac.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("spec", ac.GENERAL, ids=ac.general_id)
def test_general_critic(engine, spec, shape, variant):
    T = shape[1]
    engine.set_kernel_variant(variant)
    try:
        critic, p0 = make_general(engine, spec)
        e = general_expectation(spec, shape, "base", p0)
        traj = loaded(engine, ac.history(spec[0], shape, "base"))
        check_general(general_calls(critic, p0, traj, T), e, T)
    finally:
        engine.set_kernel_variant(0)


@VARIANTS
@pytest.mark.parametrize("shape", ac.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("spec", ac.GENERAL, ids=ac.general_id)
def test_general_critic_slot_T_is_the_value_of_the_last_observation(engine, spec, shape, variant):
    """RL_TRAJ_VALUES[T] = V(obs[T]) for every lane after rl_gae and after the One-step-TD update — the lanes whose last
    step terminated or was interrupted included, where the scan bootstraps from 0 or V(term_obs[T-1])"""
    n, T = shape
    engine.set_kernel_variant(variant)
    try:
        critic, p0 = make_general(engine, spec)
        e = general_expectation(spec, shape, "base", p0)
        traj = loaded(engine, ac.history(spec[0], shape, "base"))
        ra.gae(traj, critic, ac.GAMMA, ac.LAMBDA)
        assert np.array_equal(planes(traj, ra.TRAJ_VALUES)[0][T], e["values"][T])
        traj.write(ra.TRAJ_VALUES, np.full((T + 1, n), 7.0, np.float32))
        td_update(critic, traj, ra.VALUE_TARGET_ONE_STEP_TD, ac.TD_GAMMA, p0)
        assert np.array_equal(planes(traj, ra.TRAJ_VALUES)[0][T], e["values"][T])
    finally:
        engine.set_kernel_variant(0)


@VARIANTS
@pytest.mark.parametrize("shape", [(3, 2), (65, 17)], ids=ac.shape_id)
@pytest.mark.parametrize("spec", ac.GENERAL, ids=ac.general_id)
def test_general_critic_sequences_on_one_trajectory(engine, spec, shape, variant):
    """a history with Interrupts, then one with none, then one Interrupt in the last sample, then one in the first, all on
    ONE trajectory object: every plane after each call equals what a fresh trajectory gives for that history (a skip flag
    that is not reset, an inverted skip sense, a V(term_obs) left over from the call before)"""
    T = shape[1]
    engine.set_kernel_variant(variant)
    try:
        critic, p0 = make_general(engine, spec)
        reused = ra.Trajectory(engine, shape[0], T, spec[0])
        for pattern_set in ac.PATTERN_SETS:
            h = ac.history(spec[0], shape, pattern_set)
            reused.write_all(h)
            got = general_calls(critic, p0, reused, T)
            fresh = loaded(engine, h)
            want = general_calls(critic, p0, fresh, T)
            for k in want:
                assert np.array_equal(got[k], want[k]), (pattern_set, k)
    finally:
        engine.set_kernel_variant(0)


# ---------------------------------------------------------------- recurrent critics
RECURRENT = [("gru", {}, (32, 1)), ("gru", {}, (96, 17)), ("lstm", {}, (32, 1)), ("lstm", {}, (96, 17)),
             ("gru", dict(num_layers=2), (1, 1)), ("gru", dict(num_layers=2), (65, 17)),
             ("lstm", dict(num_layers=2), (1, 1)), ("lstm", dict(num_layers=2), (65, 17))]


@pytest.mark.parametrize("cell,kw,shape", RECURRENT,
                         ids=["%s%s-%s" % (c, "-l2" if kw else "", ac.shape_id(s)) for c, kw, s in RECURRENT])
def test_recurrent_critic(engine, cell, kw, shape):
    n, T = shape
    make = ra.GruMlp if cell == "gru" else ra.LstmMlp
    critic = make(engine, 5, 1, 16, 12, **kw) if kw else make(engine, 5, 1)
    critic.init(22)
    p0 = critic.get_params()
    h = ac.make_history(5, n, T, "base", seed=11)
    flag = h["flag"]
    assert (flag[T - 1] == O.INTERRUPT).any() if n > 2 else True
    traj = loaded(engine, h)
    v_d, s_d = critic.seq_forward(traj)
    v, s = v_d[0], s_d[0]
    used = (flag == O.INTERRUPT)
    used[T - 1] |= flag[T - 1] == O.CONTINUE
    assert np.isfinite(v).all() and np.isfinite(s[used]).all()
    assert not s[~used].any()  # the forward's side of the contract: 0 wherever the scan must not bootstrap
    adv_o, rtg_o = O.seq_gae(v, np.where(used, s, np.float32(0)), h, ac.GAMMA, ac.LAMBDA)
    td_o = O.seq_one_step_targets(v, np.where(used, s, np.float32(0)), h, np.float32(ac.TD_GAMMA))
    # slot T: what step T-1 bootstrapped from — 0 after Terminate, V(successor) otherwise (include/relearn_hip.h)
    slot_T = np.where(flag[T - 1] == O.TERMINATE, np.float32(0), s[T - 1])
    ra.gae(traj, critic, ac.GAMMA, ac.LAMBDA)
    values, adv, rtg = planes(traj, ra.TRAJ_VALUES, ra.TRAJ_ADVANTAGES, ra.TRAJ_RETURNS)
    assert np.array_equal(values[:T], v) and np.array_equal(values[T], slot_T)
    assert np.array_equal(adv, adv_o) and np.array_equal(rtg, rtg_o)
    td_update(critic, traj, ra.VALUE_TARGET_REWARD_TO_GO, ac.TD_GAMMA, p0)
    assert np.array_equal(planes(traj, ra.TRAJ_TARGETS)[0], ac.returns_f32(h, ac.TD_GAMMA))
    traj.write(ra.TRAJ_VALUES, np.full((T + 1, n), 7.0, np.float32))
    td_update(critic, traj, ra.VALUE_TARGET_ONE_STEP_TD, ac.TD_GAMMA, p0)
    tgt, values = planes(traj, ra.TRAJ_TARGETS, ra.TRAJ_VALUES)
    assert np.array_equal(tgt, td_o)
    assert np.array_equal(values[:T], v) and np.array_equal(values[T], slot_T)
