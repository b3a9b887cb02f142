"""The closed-loop rollout reference (tests/meta_rollout_ref.py) against itself, without a device: its env side replays
through MetaLanes, it is deterministic, a lane range of a run equals the run of that range at a lane offset, every
sampled action is decided by a margin far above f32 rounding, and every case's data holds what the case is there for."""
import numpy as np
import pytest

import meta_lanes_ref as M
import meta_rollout_ref as R

MIN_MARGIN = 1e-5  # of |u - p(action 0)|: more than a hundred f32 ulps of a probability (2^-24 = 6e-8 below 1)
SPLIT = 25


@pytest.mark.parametrize("case", R.GRID, ids=R.case_id)
def test_reference(case):
    ref = R.reference(case)
    assert len(ref.periods) == R.PERIODS
    lanes = M.MetaLanes(case.n, R.ARMS, case.E, case.arms, lane_offset=case.offset, seed_env=case.seed + 1)
    for p, planes in enumerate(ref.periods):
        assert planes["obs"].shape == (R.D, case.T + 1, case.n) and planes["action"].shape == (case.T, case.n)
        want = lanes.replay(planes["action"])
        for key in ("obs", "reward", "flag", "term_obs"):
            assert np.array_equal(planes[key], want[key]), (p, key)
    assert np.array_equal(ref.observe, lanes.observe())
    for got, want in zip(ref.driven, lanes.step(R.driven_actions(case.n))):
        assert np.array_equal(got, want)
    print("smallest |u - p0| = %.3g" % ref.margin)
    assert ref.margin >= MIN_MARGIN
    R.check_data(case, ref.periods)


@pytest.mark.parametrize("case", R.GRID, ids=R.case_id)
def test_reference_is_deterministic(case):
    again = R.reference.__wrapped__(case)
    ref = R.reference(case)
    assert again.margin == ref.margin
    for a, b in zip(again.periods, ref.periods):
        for key in R.PLANES:
            assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(again.observe, ref.observe)
    assert all(np.array_equal(a, b) for a, b in zip(again.driven, ref.driven))


def lane_range_equal(whole, part, first):
    for a, b in zip(whole.periods, part.periods):
        for key in R.PLANES:
            assert np.array_equal(a[key][..., first:], b[key]), key
    # (the driven step is not compared: its actions alternate from the range's first lane, and 25 is odd)
    assert np.array_equal(whole.observe[:, first:], part.observe)


@pytest.mark.parametrize("case", [c for c in R.GRID if c.n > SPLIT], ids=R.case_id)
def test_lane_range_at_an_offset(case):
    """lanes 25.. of the n-lane run equal the offset-25 run of n - 25 lanes (70 and 45 at most cases); the case with a
    lane offset of its own is lanes 25..69 of its 70-lane run at offset 0"""
    if case.offset:
        whole, part, first = R.reference(case, n=case.n + case.offset, offset=0), R.reference(case), case.offset
    else:
        whole, part, first = R.reference(case), R.reference(case, n=case.n - SPLIT, offset=SPLIT), SPLIT
    lane_range_equal(whole, part, first)
    assert part.margin >= whole.margin
