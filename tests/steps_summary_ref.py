"""numpy restatement of the reference's step statistics for the StepsSummary tests: OnlineStepsSummary::push
(src/simulation/summary.rs:198-214) over time-major reward / flag planes, OnlineMeanVariance (src/utils/stats.rs:11-15,
119-203: population variance, Chan's merge).  Shared by tests/test_steps_summary_cpu.py and
tests/test_gpu_steps_summary.py."""
import numpy as np


def mean_variance(values):
    """(mean, squared residual sum, count) of a 1-D array, two-pass in float64"""
    v = np.asarray(values, dtype=np.float64)
    if v.size == 0:
        return 0.0, 0.0, 0
    m = v.mean()
    return float(m), float(((v - m) ** 2).sum()), int(v.size)


def episodes(rewards, flags):
    """episodes that END inside [T][n] planes concatenated over time (lanes persist): (returns, lengths, end step),
    each episode summed on its own (no cumulative-sum cancellation)"""
    r = np.ascontiguousarray(np.asarray(rewards, dtype=np.float64).T)  # [n][T]
    end = np.ascontiguousarray(np.asarray(flags).T != 0)
    n, L = r.shape
    flat_r, flat_end = r.reshape(-1), end.reshape(-1)
    start = np.zeros(n * L, dtype=bool)
    start[1:] = flat_end[:-1]
    start[::L] = True
    starts = np.flatnonzero(start)
    sums = np.add.reduceat(flat_r, starts)
    stops = np.append(starts[1:], n * L)
    lengths = stops - starts
    is_ep = flat_end[stops - 1]
    return sums[is_ep], lengths[is_ep].astype(np.float64), (stops - 1)[is_ep] % L


def period_summaries(rewards, flags):
    """lists of [T][n] planes, one per push with a clear (new period) after each: the completed StepsSummary of every
    period as dicts {step_reward, episode_reward, episode_length} of (mean, srs, count)"""
    T = rewards[0].shape[0]
    R, F = np.concatenate(rewards, axis=0), np.concatenate(flags, axis=0)
    ret, length, end_t = episodes(R, F)
    out = []
    for p in range(len(rewards)):
        sel = (end_t // T) == p
        out.append(dict(step_reward=mean_variance(np.asarray(rewards[p], dtype=np.float64).reshape(-1)),
                        episode_reward=mean_variance(ret[sel]), episode_length=mean_variance(length[sel])))
    return out


def close(got, want, name=""):
    """got: a MeanVariance ctypes struct; want: (mean, srs, count).  Counts exact, means within 1e-12 relative,
    squared residual sums within 1e-10 relative (exactly 0 where numpy gives 0)"""
    m, s, c = want
    assert got.count == c, (name, got.count, c)
    if c == 0:
        return
    assert abs(got.mean - m) <= 1e-12 * abs(m) or got.mean == m, (name, got.mean, m)
    if s == 0.0:
        assert got.squared_residual_sum == 0.0, (name, got.squared_residual_sum)
    else:
        assert abs(got.squared_residual_sum - s) <= 1e-10 * abs(s), (name, got.squared_residual_sum, s)
