"""The tile walk of the general-MLP fused kernels, restated in plain Python from the text of `launch_gen_mfma`,
`k_gen_mfma` and `k_gen_pair` (relearn_amd/csrc/kernels_gen_mfma.hip): which walker of which workgroup walks which
32-sample tiles in which order for a sample count B and a compute-unit count, how many slab rows the launch leaves,
which of a walker's f32 -> f64 flushes store and which add — and, from that, the sample counts at which the walk changes
behaviour (`cases`).  tests/test_gen_walk_model.py checks the model against itself; tests/test_gpu_gen_tile_walk.py
runs the kernels at the counts of `cases` and probes the tiles `probe_tiles` names.  These kernels share no walk code
with the fused 5-128 family (tests/tile_walk_model.py), only the tile size and the rule that factors B into n x T.

Two forms on ONE grid, nwg = min(ceil(n_tiles / 4), compute units) workgroups of 4 walkers:
  WAVE  k_gen_mfma: a walker is a wave.  Wave w (its number in the grid) walks tiles w, w + 4 nwg, ... while they exist
        and fetches one tile ahead (a tile past the end reads sample B - 1 under an all-false mask).  A wave with no tile
        leaves before it touches its row: the launch counts n_tiles rows when 4 nwg >= n_tiles, else 4 nwg.  Every pass
        of a one-hidden-layer module of 65 - 128 units, and the evaluation pass of every module.
  PAIR  k_gen_pair: a walker is a pair of waves.  EVERY pair runs iters = ceil(n_tiles / (4 nwg)) iterations (the
        exchanges between its waves are workgroup barriers), on zeros where pair + it 4 nwg is no tile; 4 nwg rows
        always.  The gradient, PPO, Fisher-vector and critic passes of modules whose layers have at most 64 units.
Both flush their f32 accumulators into the f64 row after every GM_FLUSH = 64 tiles (the pair form: iterations, idle
ones included) since the last flush and after the walker's last one; a row's first flush stores, every later one adds.
"""
from collections import namedtuple

from tile_walk_model import shape_for

TILE = 32
WALKERS = 4  # GWAVES waves / GP_PAIRS pairs of a workgroup
GM_FLUSH = 64
WAVE, PAIR = "wave", "pair"
FORMS = (WAVE, PAIR)


def n_tiles(B):
    return (B + TILE - 1) // TILE


def grid(B, cus):
    """launch_gen_mfma: one workgroup per four tiles, at most one per compute unit"""
    return min((n_tiles(B) + WALKERS - 1) // WALKERS, cus)


def n_walkers(B, cus):
    return WALKERS * grid(B, cus)


def iterations(B, cus):
    """k_gen_pair's `iters`; in the wave form the tile count of the busiest wave"""
    W = n_walkers(B, cus)
    return (n_tiles(B) + W - 1) // W


def walk(B, cus, form):
    """{walker: [tile or None, ...]} in the order walked, every walker of the grid present.  None is an idle iteration
    of a pair; a wave has none (its list ends with its last tile, and is empty if it has no tile)."""
    W, tiles = n_walkers(B, cus), n_tiles(B)
    out = {}
    for w in range(W):
        if form == WAVE:
            out[w] = list(range(w, tiles, W))
        else:
            out[w] = [w + it * W if w + it * W < tiles else None for it in range(iterations(B, cus))]
    return out


def fetches(B, cus, form):
    """{walker: [tile index handed to gm_load_tile, ...]}: the walker's first tile, then one tile ahead per iteration.
    An index >= n_tiles is fetched under an all-false mask from sample B - 1."""
    W = n_walkers(B, cus)
    out = {}
    for w, tiles in walk(B, cus, form).items():
        out[w] = [w + k * W for k in range(len(tiles) + 1)] if tiles else []
    return out


def owner_of(B, cus, tile):
    """the walker that walks `tile`"""
    assert 0 <= tile < n_tiles(B)
    return tile % n_walkers(B, cus)


def rows(B, cus, form):
    """t->last_rows of launch_gen_mfma"""
    W = n_walkers(B, cus)
    return W if form == PAIR or W < n_tiles(B) else n_tiles(B)


def writers(B, cus, form):
    """the walkers that write a slab row"""
    return [w for w, tiles in walk(B, cus, form).items() if tiles]


def flush_pattern(count):
    """the in-loop flushes of a walker that runs `count` iterations (a pair: idle ones included), as
    [("store" | "add", iterations folded by it), ...]: after every GM_FLUSH-th iteration since the last flush and after
    the last iteration; the first stores, every later one adds.  There is no flush outside the loop."""
    out, done = [], 0
    while done < count:
        k = min(GM_FLUSH, count - done)
        out.append(("add" if out else "store", k))
        done += k
    return out


# ------------------------------------------------------------------------------------------------ the case table
Case = namedtuple("Case", "name B n T")


def cases(cus):
    """The named sample counts, each the smallest with its property on a device of `cus` compute units (the properties:
    tests/test_gen_walk_model.py).  A count is given in tiles, W = 4 cus walkers of the capped grid; "-tail" makes the
    last of those tiles ragged, and B = n x T by tile_walk_model.shape_for (a tail: T in 7, 5, 3, else T = 1)."""
    W = WALKERS * cus
    out = []

    def add(name, tiles, tail, shape=None):
        B, n, T = shape if shape is not None else shape_for(tiles - 1 if tail else tiles, tail)
        assert n_tiles(B) == tiles and (B % TILE != 0) == bool(tail) and n * T == B
        out.append(Case(name, B, n, T))

    add("B1", 1, True, shape=(1, 1, 1))
    add("B31", 1, True, shape=(31, 31, 1))
    add("B32", 1, False)
    add("B33", 2, True, shape=(33, 11, 3))
    add("wg-4", 4, False)        # one full workgroup
    add("wg-5-tail", 5, True)    # a second workgroup for the ragged tile: three of its walkers have no tile
    for d, tag in ((-1, "cap-1"), (0, "cap"), (1, "cap+1")):
        add(tag, W + d, False)
        add(tag + "-tail", W + d, True)
    add("rounds-2.5-tail", 2 * W + W // 2 + 1, True)
    add("flush-63-tail", GM_FLUSH * W - 1, True)
    add("flush-64", GM_FLUSH * W, False)
    add("flush-65", GM_FLUSH * W + 1, False)
    add("flush-65-tail", GM_FLUSH * W + 1, True)
    add("flush-all-65-tail", (GM_FLUSH + 1) * W + W // 2 + 3, True)
    assert len({c.name for c in out}) == len(out)
    return out


def case_names():
    """the names alone (they do not depend on the compute-unit count)"""
    return [c.name for c in cases(256)]


# the cases from 64 W tiles up: the only ones large enough to be worth a second and third pair-form module
FLUSH_CASES = ("flush-64", "flush-65", "flush-65-tail", "flush-all-65-tail")


def below_second_round(case, cus):
    """no walker has a second tile (and no pair a second iteration)"""
    return n_tiles(case.B) <= n_walkers(case.B, cus)


def probe_tiles(case, cus, form, limit=8):
    """The tiles to light up one at a time, in this order (duplicates dropped, at most `limit`): the ragged tile; of
    the busiest walker (the lowest-numbered of those with the most tiles) its first tile, the tile that completes its
    flush period, the one after it and its last; the 64th tile of the last walker where that is its last (a pair then
    runs a 65th iteration on zeros, and its second flush must add zero); tile n_full - 1; the first tile of the last
    workgroup."""
    lists = {w: [t for t in tiles if t is not None] for w, tiles in walk(case.B, cus, form).items()}
    n_full, tail = case.B // TILE, case.B % TILE
    picks = []

    def take(t):
        if t is not None and t not in picks:
            picks.append(t)

    if tail:
        take(n_full)
    busiest = max(lists, key=lambda w: (len(lists[w]), -w))
    mine = lists[busiest]
    take(mine[0])
    if len(mine) >= GM_FLUSH:
        take(mine[GM_FLUSH - 1])
    if len(mine) > GM_FLUSH:
        take(mine[GM_FLUSH])
    take(mine[-1])
    last = lists[max(lists)]
    if len(last) == GM_FLUSH:
        take(last[-1])
    if n_full > 0:
        take(n_full - 1)
    W = n_walkers(case.B, cus)
    take(next((lists[w][0] for w in range(W - WALKERS, W) if lists[w]), None))
    return picks[:limit]
