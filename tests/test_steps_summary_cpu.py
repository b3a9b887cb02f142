"""StepsSummary on the host (CPU only): rl_steps_summary_merge — `impl Add for StepsSummary` (src/simulation/summary.rs,
src/utils/stats.rs:184-209) — against the numpy restatement over random splits, empty sides included; the C++ program
of the GPU test compiles."""
import math
import os
import subprocess
import tempfile

import numpy as np

import relearn_amd as ra
from steps_summary_ref import close, mean_variance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("step_reward", "episode_reward", "episode_length")


def stats_of(parts):
    s = ra.StepsSummaryStats()
    for f, v in zip(FIELDS, parts):
        m, srs, c = mean_variance(v)
        getattr(s, f).mean, getattr(s, f).squared_residual_sum, getattr(s, f).count = m, srs, c
    return s


def test_merge_matches_numpy_over_random_splits():
    ra.build()
    rng = np.random.default_rng(7)
    for trial in range(200):
        vals = [rng.normal(rng.uniform(-5, 5), rng.uniform(0.1, 1e3), rng.integers(0, 300)) for _ in FIELDS]
        if trial % 5 == 0:
            vals[0][: len(vals[0]) // 3] = 1e6  # large values beside small ones
        cuts = [int(rng.integers(0, len(v) + 1)) for v in vals]
        if trial % 7 == 0:
            cuts = [0] * 3  # left side empty
        if trial % 11 == 0:
            cuts = [len(v) for v in vals]  # right side empty
        a = stats_of([v[:k] for v, k in zip(vals, cuts)])
        b = stats_of([v[k:] for v, k in zip(vals, cuts)])
        got = ra.steps_summary_merge(a, b)
        for f, v in zip(FIELDS, vals):
            close(getattr(got, f), mean_variance(v), f)


def test_empty_side_returns_the_other_side_unchanged():
    ra.build()
    a = stats_of([np.array([1.0, 2.0, 4.0]), np.array([3.0]), np.array([])])
    e = ra.StepsSummaryStats()
    for got in (ra.steps_summary_merge(a, e), ra.steps_summary_merge(e, a)):
        for f in FIELDS:
            x, y = getattr(got, f), getattr(a, f)
            assert (x.mean, x.squared_residual_sum, x.count) == (y.mean, y.squared_residual_sum, y.count)
    both = ra.steps_summary_merge(e, e)  # the reference computes 0 / 0 here; documented deviation
    for f in FIELDS:
        x = getattr(both, f)
        assert x.count == 0 and x.mean == 0.0 and x.squared_residual_sum == 0.0
        assert not math.isnan(x.mean) and x.stddev() is None
    assert a.episode_reward.stddev() == 0.0 and abs(a.step_reward.stddev() - math.sqrt(14 / 9)) < 1e-15


def test_merge_of_constant_values_keeps_sigma_zero():
    ra.build()
    a, b = stats_of([np.ones(37)] * 3), stats_of([np.ones(91)] * 3)
    got = ra.steps_summary_merge(a, b)
    assert got.step_reward.mean == 1.0 and got.step_reward.squared_residual_sum == 0.0 and got.step_reward.count == 128


def test_steps_summary_demo_compiles():
    ra.build()
    out = os.path.join(tempfile.mkdtemp(), "steps_summary_demo")
    libdir = os.path.join(ROOT, "relearn_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", ROOT,
                           os.path.join(ROOT, "tests", "cpp", "steps_summary_demo.cpp"), "-o", out, "-L", libdir,
                           "-lrelearn_hip", "-Wl,-rpath," + libdir])
    assert os.path.exists(out)
