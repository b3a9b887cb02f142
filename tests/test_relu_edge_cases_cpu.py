"""The conditions the table of tests/relu_edge_cases.py claims, recomputed here independently of the library: exact signs
from fractions.Fraction, the order-free condition from a restatement of the kernels' piece splits, the margin of the
margin cases, a dead sample's exact forward, and which cases the numeric range guard must accept."""
from fractions import Fraction

import numpy as np
import pytest

import relu_edge_cases as R

F32 = np.float32
SETS = list(R.SETS.values())
ALL = [(s, d) for s in SETS for d in s.designs]
IDS = ["%s / %s" % (s.name, d.name) for s, d in ALL]


def test_the_splits_are_exact_and_their_pieces_are_bf16():
    rng = np.random.default_rng(0)
    values = list((rng.standard_normal(200) * 10.0 ** rng.integers(-12, 9, size=200)).astype(np.float32))
    values += [v for s in SETS for v in s.x if np.abs(v) >= 2.0 ** -100]
    for v in values:
        for split in (R.split3, R.split3t):
            p = split(v)
            assert sum((R.frac(q) for q in p), Fraction(0)) == R.frac(v), (split.__name__, v, p)
            assert all(R.is_bf16(q) for q in p), (split.__name__, v, p)
        # truncation: pieces have the value's sign; rounding may give pieces of either sign
        assert all(q == 0 or np.sign(q) == np.sign(v) for q in R.split3t(v))
    # bf16 rounding is to nearest, ties to even
    assert R.bf16_round(F32(1.0 + 2.0 ** -8)) == 1.0 and R.bf16_round(F32(1.0 + 3 * 2.0 ** -8)) == F32(1.0 + 2.0 ** -6)
    assert R.split3(F32(1.0 - 2.0 ** -22))[1] < 0


def test_quantum():
    assert R.quantum([Fraction(3, 4), Fraction(6)]) == Fraction(1, 4)
    assert R.quantum([Fraction(0)]) is None and R.quantum([Fraction(-8), Fraction(24)]) == 8


@pytest.mark.parametrize("s, d", ALL, ids=IDS)
def test_the_recorded_sign_is_the_exact_sign(s, d):
    pre = R.exact_pre(s.x, d)
    if d.family == "zero":
        assert pre == 0 and d.expect == 0
    elif d.family == "worst":
        assert d.expect is None and pre > 0
    else:
        assert pre != 0 and d.expect == (1 if pre > 0 else 0)
    # the f64 oracle's own evaluation (products exact in f64, five f64 additions) has that sign too
    pre64 = np.float64(d.b)
    for k in range(R.D):
        pre64 = pre64 + np.float64(d.w[k]) * np.float64(s.x[k])
    assert (pre64 > 0) == (pre > 0)


@pytest.mark.parametrize("s, d", ALL, ids=IDS)
def test_order_free_designs_cannot_round_in_any_order(s, d):
    if not d.order_free:
        assert d.family in ("margin", "worst", "subnormal")
        return
    assert R.is_order_free(s.x, d)
    q, total = R.order_free_quantum(s.x, d)
    pre = R.exact_pre(s.x, d) * Fraction(2) ** R.FWD_SCALE_LOG2
    if q is not None:
        assert (pre / q).denominator == 1 and total < 2 ** 24 * q
        # a non-zero scaled pre-activation is at least 1: the clamped conversion gives 0 or 1, never a fraction
        assert pre == 0 or abs(pre) >= 1


def test_the_smallest_cases_are_the_smallest_the_condition_allows():
    """halving the distance from zero would break the order-free condition: sum|piece products| >= 2^23 x that distance"""
    seen = 0
    for s, d in ALL:
        if d.family == "smallest" or (d.family == "largest" and "2^31" in d.name):
            pre = abs(R.exact_pre(s.x, d)) * Fraction(2) ** R.FWD_SCALE_LOG2
            _, total = R.order_free_quantum(s.x, d)
            if d.family == "smallest":
                assert total >= 2 ** 23 * pre / 2, (s.name, d.name)
            seen += 1
    assert seen >= 12


def test_the_lower_edge_cases_sit_on_the_guards_lower_edge():
    for name in ("lower-weight", "lower-bias"):
        s = R.SETS[name]
        W1, b1 = R.layer1(s)
        xmin = min(abs(float(v)) for v in s.x if v != 0)
        for d in s.designs:
            if d.family == "plain":
                continue
            largest = max(max(abs(float(w)) for w in d.w) * xmin, abs(float(d.b)))
            assert largest == 0.0 or 2.0 ** -46 <= largest <= 2.0 ** -46 * (1 + 2.0 ** -21), (name, d.name, largest)
    s = R.SETS["upper"]
    tops = [abs(R.exact_pre(s.x, d)) for d in s.designs]
    assert max(tops) == 2 ** 31 - 2 ** 8 and Fraction(2 ** 30 + 2 ** 29) in tops and Fraction(2 ** 30 - 2 ** 29) in tops


def test_the_margin_cases_have_the_margin_and_use_every_piece_pair():
    s = R.SETS["margin"]
    assert all(int(np.asarray(v).view(np.uint32)) & 1 for v in s.x)
    sides, pair_signs = set(), [set() for _ in range(9)]
    for d in s.designs:
        assert all(int(np.asarray(w).view(np.uint32)) & 1 for w in d.w[:4])
        terms = R.exact_terms(s.x, d)
        pre, size = sum(terms, Fraction(0)), sum((abs(t) for t in terms), Fraction(0))
        # |pre| = 2^-20 sum|terms| up to the rounding of the one tuned weight; an f32 summation of six exact products in any
        # order errs by less than 5 x 2^-24 sum|terms| < 2^-21 sum|terms| (five additions, each within 2^-24 of a partial
        # sum that is at most sum|terms| (1 + 2^-24)^5), so the margin left is more than 2^-20 (7/8 - 1/2) sum|terms|
        edge = Fraction(R.RELU_EDGE)
        assert edge * Fraction(7, 8) <= abs(pre) / size <= edge * Fraction(9, 8), (d.name, float(abs(pre) / size))
        assert d.expect == (1 if pre > 0 else 0) and d.b < 0
        sides.add(d.expect)
        for term in R.piece_products(s.x, d)[:R.D]:
            for i, v in enumerate(term):
                if v != 0:
                    pair_signs[i].add(v > 0)
        # negative pieces of a positive weight: the rounding split
        sides.add(("neg", any(np.sign(p) == -np.sign(w) for w in d.w for p in R.split3(R.scaled_weight(w)) if p != 0)))
    assert sides >= {0, 1, ("neg", True)}
    assert all(sg == {True, False} for sg in pair_signs), pair_signs
    assert len(s.designs) >= 32


def test_the_worst_case_is_2_to_the_minus_46_of_its_terms():
    s = R.SETS["lower-weight"]
    (d,) = [d for d in s.designs if d.family == "worst"]
    terms = R.exact_terms(s.x, d)
    assert sum(terms, Fraction(0)) == Fraction(2) ** -92  # 16 in the scaled accumulator: a mask of 1 when nothing is lost
    assert sorted(abs(t) for t in terms)[-2:] == [Fraction(2) ** -46 * (1 + Fraction(2) ** -22),
                                                  Fraction(2) ** -46 * (1 + Fraction(2) ** -23) ** 2]
    assert not R.is_order_free(s.x, d)


def test_the_subnormal_observation_is_subnormal():
    s = R.SETS["subnormal-obs"]
    assert all(v == 0 or abs(float(v)) < 2.0 ** -126 for v in s.x) and min(abs(float(v)) for v in s.x if v != 0) == 2.0 ** -149
    for d in s.designs:
        assert d.expect == (1 if d.b > 0 else 0)


@pytest.mark.parametrize("s", SETS, ids=[s.name for s in SETS])
def test_layouts_and_output_weights(s):
    W1, b1 = R.layer1(s)
    assert s.copies == bool((b1 > 0).any())  # a dead sample (pre = b1) must have no unit on
    masks = R.expected_masks(s)
    assert (masks == 1).sum() >= 20 and (masks == 0).sum() >= 20  # one module carries both sides many times
    # every design sits on both lane halves' sample rows of several hidden tiles
    for i, d in enumerate(s.designs):
        units = [j for j in range(R.H) if j % len(s.designs) == i]
        assert len({j // 32 for j in units}) >= 2 or len(s.designs) > 32, d.name
    for out_dim, seed in ((2, 2), (1, 3)):
        for moved in (False, True):
            w2 = R.w2_grid(s, out_dim, seed, moved)
            grid = np.ldexp(w2.astype(np.float64), 10 - s.w2_log2)
            assert np.array_equal(grid, np.round(grid)) and 56 <= np.abs(grid).min() and np.abs(grid).max() <= 136
            if not s.copies:
                for a in range(out_dim):
                    q, total = R.dead_forward_quantum(s, w2[a])
                    assert q is None or total < 2 ** 24 * q, (s.name, out_dim, a)
        assert np.mean(R.w2_grid(s, out_dim, seed, True) != R.w2_grid(s, out_dim, seed)) == 1.0


def planes_of(s):
    """every observation the guard's range words see: the designed sample and zeros"""
    return np.concatenate([np.asarray(s.x, dtype=np.float32), np.zeros(5, dtype=np.float32)])


@pytest.mark.parametrize("s", SETS, ids=[s.name for s in SETS])
def test_the_guard_accepts_every_set(s):
    W1, b1 = R.layer1(s)
    assert not R.guard_refuses(W1, b1, planes_of(s))


@pytest.mark.parametrize("g", list(R.GUARD_CASES.values()), ids=list(R.GUARD_CASES))
def test_the_guards_boundary(g):
    s = R.guard_set(g)
    W1, b1 = R.layer1(s)
    assert R.guard_refuses(W1, b1, planes_of(s)) == g.refused
    # the stated bound in exact arithmetic (dyadic operands: the guard's own f32 sums are exact)
    xmax = max(abs(R.frac(v)) for v in g.x)
    xmin = min(abs(R.frac(v)) for v in g.x if v != 0)
    wsum = sum((abs(R.frac(w)) for w in g.w), Fraction(0))
    upper = wsum * xmax + abs(R.frac(g.b))
    largest = max(max(abs(R.frac(w)) for w in g.w) * xmin, abs(R.frac(g.b)))
    assert g.refused == (not (upper < 2 ** 31) or not (wsum < 2 ** 31) or not (largest >= Fraction(2) ** -46))
    # and the boundary is met exactly or missed by one unit in the last place
    if "upper" in g.name:
        assert upper in (Fraction(2 ** 31), Fraction(2 ** 31 - 2 ** 7))
    elif "weights" in g.name:
        assert wsum in (Fraction(2 ** 31), Fraction(2 ** 31 - 2 ** 7)) and upper < 1
    else:
        assert largest in (Fraction(2) ** -46, Fraction(2) ** -46 * (1 - Fraction(2) ** -24))


def test_a_guard_that_compared_with_other_powers_of_two_would_differ():
    """the boundary cases tell 2^31 from 2^32 and 2^-46 from 2^-47: restated with the other constant the verdicts change"""
    refused = [g.refused for g in R.GUARD_CASES.values()]
    assert refused.count(True) == 5 and refused.count(False) == 5
