"""Case tables of the PartitionGame lanes (test infrastructure, not a test): the seeds, lane counts and limits that
tests/test_partition_ref.py holds to its own conditions on the CPU and tests/test_gpu_partition*.py run on the device
against tests/partition_ref.py.  The references are computed once per process and left unchanged.

Shapes: 64 lanes and 200 (off the block size of every env kernel), a horizon of 7 steps, the limits VISIBLE 3, LATENT 3
and none — an Interrupt and a reset fall inside every horizon under a limit — and a lane offset above 0, which shows that
the streams are keyed by the global lane.  gen_range(0..10) rejects three draws in eight, so the lanes' stream positions
drift apart at once and elements straddle ChaCha blocks in every case (tests/test_partition_ref.py counts them)."""
import collections
import functools

import numpy as np

import partition_ref as P
import seq_multi_ref as R

HORIZON = 7
VISIBLE3, LATENT3 = P.Limit(P.LIMIT_VISIBLE, 3), P.Limit(P.LIMIT_LATENT, 3)
MIN_MARGIN = R.MIN_MARGIN  # the project's: 1e-5

# ---------------------------------------------------------------- driven steps
Driven = collections.namedtuple("Driven", "limit n offset seed")
DRIVEN = [
    Driven(VISIBLE3, 200, 0, 71),
    Driven(LATENT3, 64, 0, 72),
    Driven(P.NO_LIMIT, 200, 0, 73),
    Driven(VISIBLE3, 64, 137, 71),  # the lanes 137..200 of the first case: global-lane keying
]
DRIVEN_STEPS = 2 * HORIZON
DrivenRef = collections.namedtuple("DrivenRef", "observe0 actions steps straddles")
"""steps: per step (reward, flag, obs, term_obs); straddles: element draws whose ten words span two ChaCha blocks"""


def limit_id(limit):
    return {P.LIMIT_NONE: "none", P.LIMIT_LATENT: "latent%d", P.LIMIT_VISIBLE: "visible%d"}[limit.kind] % (
        () if limit.kind == P.LIMIT_NONE else (limit.max_steps,))


def driven_id(c):
    return "%s-n%d-off%d-seed%d" % (limit_id(c.limit), c.n, c.offset, c.seed)


def straddling(lanes):
    """lanes whose next element (ten words from env_pos) runs into the next block"""
    return sum(1 for lane in lanes.lanes if (lane.env_pos & 15) > 6)


@functools.lru_cache(maxsize=None)
def driven_reference(c):
    lanes = P.PartitionLanes(c.n, c.limit, lane_offset=c.offset, seed_env=c.seed)
    # (the actions are drawn for global lanes 0..255, so that an offset case repeats its part of the whole)
    rs = np.random.default_rng(2000 + c.seed)
    observe0 = lanes.observe()
    actions, steps, straddles = [], [], 0
    for _ in range(DRIVEN_STEPS):
        a = rs.integers(0, 2, 256).astype(np.uint8)[c.offset:c.offset + c.n]
        actions.append(a)
        straddles += straddling(lanes)  # (a step's draw; the reset's after an Interrupt is not counted)
        steps.append(lanes.step(a))
    return DrivenRef(observe0, actions, steps, straddles)


# ---------------------------------------------------------------- closed-loop rollouts
Closed = collections.namedtuple("Closed", "net limit n T offset seed")
# Net(cell, D, H, layers, mlp_hidden (0: a Linear tail), bias, outputs); seed: the module's init seed, seed_env = seed + 1,
# seed_actor = seed + 2, chosen on the CPU (tests/test_partition_ref.py) so that every sampled action is decided by more
# than MIN_MARGIN.  D = 24 is the one launch, D = 23 the launch sequence per step; both cells and both tails at each.
CLOSED = [
    Closed(R.Net("gru", 24, 9, 1, 6, True, 2), VISIBLE3, 200, HORIZON, 0, 801),
    Closed(R.Net("lstm", 24, 8, 1, 0, True, 2), VISIBLE3, 64, HORIZON, 0, 811),
    Closed(R.Net("gru", 24, 8, 1, 0, True, 2), VISIBLE3, 64, HORIZON, 31, 821),
    Closed(R.Net("lstm", 24, 7, 2, 5, False, 2), VISIBLE3, 64, HORIZON, 0, 831),
    Closed(R.Net("gru", 23, 8, 1, 0, True, 2), LATENT3, 200, HORIZON, 0, 841),
    Closed(R.Net("lstm", 23, 9, 1, 6, True, 2), P.NO_LIMIT, 64, HORIZON, 5, 851),
]
PERIODS = 2


def closed_id(c):
    return "%s-%s-n%d-T%d-off%d" % (R.net_id(c.net), limit_id(c.limit), c.n, c.T, c.offset)


def closed_params(c):
    import oracle as O
    inits = list(O.RNN_DEFAULT_INITS)
    if c.net.bias:
        inits[2] = R.BIAS_INIT
    return R.init(c.net, c.seed, tuple(inits))


@functools.lru_cache(maxsize=None)
def closed_reference(c):
    return P.rollout(c.net, c.limit, c.n, c.T, c.seed + 1, c.seed + 2, closed_params(c), lane_offset=c.offset,
                     periods=PERIODS)
