"""The case table of tests/advantage_cases.py, checked with the oracle alone: every history holds the episode ends it is
there for (a condition, not a measurement), the NumPy restatements of the scans equal the oracle's bit for bit, and the
f32 scan stays inside a first-order rounding bound of the f64 definition."""
import numpy as np
import pytest

import advantage_cases as ac
import oracle as O

CASES = [(s, p) for s in ac.SHAPES for p in ac.PATTERN_SETS]
IDS = ["%s-%s" % (ac.shape_id(s), p) for s, p in CASES]


def lanes_with(shape, pattern):
    n, T = shape
    return [i for i in range(n) if ac.PATTERNS[i % len(ac.PATTERNS)] == pattern and ac.pattern_of(i, T) == pattern]


def test_shapes_are_the_ones_the_scans_change_behaviour_at():
    assert ac.SHAPES == [(1, 1), (3, 2), (65, 15), (63, 16), (65, 17), (130, 33)]
    Ts = [T for _, T in ac.SHAPES]
    assert any(T < ac.BATCH for T in Ts) and ac.BATCH in Ts and ac.BATCH + 1 in Ts and 2 * ac.BATCH + 1 in Ts
    # a patterned (not all-Continue) lane in a second and in a third 64-thread workgroup
    assert ac.pattern_of(64, 15) != "continue" and ac.pattern_of(129, 33) != "continue" and 129 // 64 == 2
    assert len(ac.PATTERNS) == 9 and len(set(ac.PATTERNS)) == 9


@pytest.mark.parametrize("shape,pattern_set", CASES, ids=IDS)
def test_every_history_holds_what_it_claims(shape, pattern_set):
    n, T = shape
    for D in (1, 5, 8):
        h = ac.history(D, shape, pattern_set)
        flag, term = h["flag"], h["term_obs"]
        assert h["obs"].shape == (D, T + 1, n) and term.shape == (D, T, n) and flag.shape == (T, n)
        assert h["obs"].dtype == h["reward"].dtype == term.dtype == np.float32 and flag.dtype == h["action"].dtype == np.uint8
        assert np.isfinite(h["obs"]).all() and np.isfinite(h["reward"]).all() and flag.max() <= O.INTERRUPT
        # term_obs: poisoned exactly where no Interrupt stands
        intr = flag == O.INTERRUPT
        assert np.isnan(term[:, ~intr]).all() and np.isfinite(term[:, intr]).all()
        if pattern_set == "no_interrupt":
            assert not intr.any()
        elif pattern_set == "only_last_sample":
            assert np.argwhere(intr).tolist() == [[T - 1, n - 1]]
        elif pattern_set == "only_first_sample":
            assert np.argwhere(intr).tolist() == [[0, 0]]
        if pattern_set != "base":
            base = ac.history(D, shape, "base")["flag"]
            assert np.array_equal(flag != O.CONTINUE, (base != O.CONTINUE) | intr)  # the ends stay where they were
            continue
        # the placed ends, lane by lane
        for i in range(n):
            p, f = ac.pattern_of(i, T), flag[:, i]
            others = np.ones(T, dtype=bool)
            if p == "continue":
                assert not f.any()
            elif p in ("term_last", "intr_last"):
                others[T - 1] = False
                assert f[T - 1] == (O.TERMINATE if p == "term_last" else O.INTERRUPT) and not f[others].any()
            elif p in ("term_first", "intr_first"):
                others[0] = False
                assert f[0] == (O.TERMINATE if p == "term_first" else O.INTERRUPT) and not f[others].any()
            elif p == "every_step":
                assert (f[0::2] == O.TERMINATE).all() and (f[1::2] == O.INTERRUPT).all()
            elif p in ("term_batch_edge", "intr_batch_edge"):
                k = O.TERMINATE if p == "term_batch_edge" else O.INTERRUPT
                others[[T - 16, T - 17]] = False
                assert T >= 18 and f[T - 16] == k and f[T - 17] == k and not f[others].any()
        # ... and together, where n and T allow
        if n >= len(ac.PATTERNS):
            assert {int(c) for c in flag[T - 1]} == {O.CONTINUE, O.TERMINATE, O.INTERRUPT}
            assert {O.TERMINATE, O.INTERRUPT} <= {int(c) for c in flag[0]}
            assert lanes_with(shape, "continue") and not flag[:, lanes_with(shape, "continue")].any()
            assert any((flag[:, i] == O.CONTINUE).all() for i in range(n))
            # a patterned lane in the last workgroup of the 64-thread scans
            assert (n - 1) // 64 == 0 or flag[:, 64 * ((n - 1) // 64):].any()
        elif n == 3:
            assert flag[T - 1].tolist() == [O.CONTINUE, O.TERMINATE, O.INTERRUPT]
        if T >= 18:
            for k, p in ((O.TERMINATE, "term_batch_edge"), (O.INTERRUPT, "intr_batch_edge")):
                lanes = lanes_with(shape, p)
                assert lanes and (flag[T - 16, lanes] == k).all() and (flag[T - 17, lanes] == k).all()
        else:
            assert not lanes_with(shape, "term_batch_edge") and not lanes_with(shape, "intr_batch_edge")


def random_values(hist, seed):
    rng = np.random.default_rng(seed)
    T, n = hist["flag"].shape
    return rng.normal(size=(T, n)).astype(np.float32), rng.normal(size=(T, n)).astype(np.float32)


@pytest.mark.parametrize("shape,pattern_set", CASES, ids=IDS)
def test_restatements_equal_the_array_fed_oracle_bit_for_bit(shape, pattern_set):
    h = ac.history(5, shape, pattern_set)
    values, succ = random_values(h, 3)
    for gamma, lam in ((ac.GAMMA, ac.LAMBDA), (ac.TD_GAMMA, 0.95), (1.0, 1.0)):
        adv, rtg = ac.scan_f32(values, succ, h, gamma, lam)
        adv_o, rtg_o = O.seq_gae(values, succ, h, gamma, lam)
        assert np.array_equal(adv, adv_o) and np.array_equal(rtg, rtg_o)
        assert np.array_equal(ac.td_f32(values, succ, h, gamma), O.seq_one_step_targets(values, succ, h, np.float32(gamma)))
        assert np.array_equal(ac.returns_f32(h, gamma), rtg_o)


def test_successors_is_the_selection_rule():
    h = ac.history(5, (65, 17), "base")
    T, n = h["flag"].shape
    v_term, v_last = np.full((T, n), np.nan, np.float32), np.arange(1, n + 1, dtype=np.float32)
    v_term[h["flag"] == O.INTERRUPT] = -2.0
    succ = ac.successors(h, v_term, v_last)
    for t in range(T):
        for i in range(n):
            f = h["flag"][t, i]
            want = -2.0 if f == O.INTERRUPT else (v_last[i] if f == O.CONTINUE and t == T - 1 else 0.0)
            assert succ[t, i] == want, (t, i)


@pytest.mark.parametrize("D", [5, 4])
@pytest.mark.parametrize("shape", ac.SHAPES, ids=ac.shape_id)
def test_fused_shapes_through_the_lanes_route(D, shape):
    """the 5-128-1 / 4-128-1 critics are held to oracle_lanes_gae: its own values and the successor selection from them,
    fed to the restated scan, reproduce its advantages, returns and One-step-TD targets"""
    n, T = shape
    cs = O.MlpShape(D, 128, 1)
    cp = O.mlp_init(cs, 3)
    for pattern_set in ac.PATTERN_SETS:
        h = ac.history(D, shape, pattern_set)
        values, adv_o, rtg_o = O.lanes_gae(cs, cp, h, ac.GAMMA, ac.LAMBDA)
        x = np.nan_to_num(h["term_obs"].reshape(D, T * n).T, nan=0.0)
        v_term = O.mlp_forward_batch(cs, cp, x)[:, 0].reshape(T, n)
        succ = ac.successors(h, v_term, values[T])
        adv, rtg = ac.scan_f32(values, succ, h, ac.GAMMA, ac.LAMBDA)
        assert np.array_equal(adv, adv_o) and np.array_equal(rtg, rtg_o)
        assert not np.isnan(adv_o).any() and not np.isnan(values).any()
        td_o = O.lanes_one_step_targets(cs, cp, h, np.float32(ac.TD_GAMMA))
        assert np.array_equal(ac.td_f32(values, succ, h, ac.TD_GAMMA), td_o) and not np.isnan(td_o).any()
        assert np.array_equal(ac.returns_f32(h, ac.TD_GAMMA), O.lanes_gae(cs, cp, h, ac.TD_GAMMA, ac.LAMBDA)[2])


@pytest.mark.parametrize("spec", ac.GENERAL, ids=ac.general_id)
def test_general_expectation_holds_no_poison(spec):
    """the expectation of a general critic, built as the device test builds it (oracle-initialised parameters here):
    V(term_obs) is poison wherever no Interrupt stands and none of it reaches a plane; the Interrupts do"""
    D, hidden, act, bias = spec
    p = O.mlp_layers_init(D, hidden, 1, 5)
    if not bias:  # the kernels only
        p = np.concatenate([p[k:k + fi * fo] for (fi, fo), k in zip(
            ac.layer_dims(D, hidden, 1), np.cumsum([0] + [fi * fo + fo for fi, fo in ac.layer_dims(D, hidden, 1)]))])
    assert p.size == ac.general_num_params(spec)
    for shape in ac.SHAPES:
        h = ac.history(D, shape, "base")
        e = ac.general_expectation(spec, p, h)
        intr = h["flag"] == O.INTERRUPT
        assert np.isfinite(e["v_term"][intr]).all()
        if act != "Relu" and (~intr).any():  # (max(NaN, 0) = 0: behind a ReLU the poison comes out as one constant)
            assert np.isnan(e["v_term"][~intr]).all()
        for k in ("values", "succ", "adv", "rtg", "td"):
            assert np.isfinite(e[k]).all(), k
        assert np.array_equal(ac.scan_f32(e["values"], e["succ"], h, ac.GAMMA, ac.LAMBDA)[0], e["adv"])
        if intr.any():  # the Interrupts matter: without V(term_obs) the planes differ
            zeroed = ac.successors(h, np.zeros_like(e["v_term"]), e["values"][-1])
            assert not np.array_equal(O.seq_gae(e["values"][:-1], zeroed, h, ac.GAMMA, ac.LAMBDA)[0], e["adv"])


@pytest.mark.parametrize("shape,pattern_set", CASES, ids=IDS)
def test_f32_scan_against_the_f64_definition(shape, pattern_set):
    """|a32 - a64| <= k 2^-24 S per sample: k = three roundings per remaining step of the segment (the product with the
    rounded lam*gamma, its addition, and lam*gamma's own rounding once per power) plus three (dn, tmp, delta); S = the sum
    of the absolute values of the terms of that sample's sum"""
    h = ac.history(5, shape, pattern_set)
    values, succ = random_values(h, 4)
    adv32, rtg32 = ac.scan_f32(values, succ, h, ac.GAMMA, ac.LAMBDA)
    adv64, rtg64, steps, s_adv, s_rtg = ac.scan_f64(values, succ, h, ac.GAMMA, ac.LAMBDA)
    k = 3.0 * steps + 3.0
    u = 2.0 ** -24
    ra_, rr_ = np.abs(adv32 - adv64) / (k * u * s_adv), np.abs(rtg32 - rtg64) / (k * u * s_rtg)
    print("%s %s: worst |a32 - a64| / bound %.3g, returns %.3g" % (ac.shape_id(shape), pattern_set, ra_.max(), rr_.max()))
    assert (ra_ <= 1.0).all() and (rr_ <= 1.0).all()
