"""The tile walk of the fused 5-128 update kernels, restated in plain Python from the text of `fused_grid`
(relearn_amd/csrc/kernels.hpp), `bt::deal_tiles` and `bt::walk_tiles` (relearn_amd/csrc/bf16_tile.hpp): which real wave
of which workgroup walks which 32-sample tiles in which order, for a sample count B and a compute-unit count — and, from
that, the sample counts at which the walk changes behaviour (`cases`).  tests/test_tile_walk_model.py checks the model
against itself and against what tests/test_gpu_fused_bits.py states; tests/test_gpu_tile_walk.py runs the kernels at
the counts of `cases` and probes the tiles `probe_tiles` names.

Two forms share the code:
  EIGHT  eight waves per workgroup, every wave walks (8 walkers); the older wave of each SIMD (waves 0-3) plays
         SHARE_OLD = 5 virtual waves, the younger (4-7) SHARE_YOUNG = 3: 32 virtual waves per workgroup.  k_policy_bf16 in
         gradient, PPO and Fisher-vector mode (f32 -> f64 flush every PB_FLUSH = 16 tiles of a real wave) and
         k_critic_step_mfma<1> (C_FLUSH = 64).
  EVAL   sixteen waves, dealt 1 : 1: 16 virtual waves per workgroup, on the SAME grid (the launcher sizes it by 8
         walkers).  k_policy_bf16 in evaluation mode.
"""
from collections import namedtuple

TILE = 32
SHARE_OLD, SHARE_YOUNG = 5, 3
PB_FLUSH, C_FLUSH = 16, 64
GRID_WALKERS = 8  # fused_grid(traj, V2_WAVES) / fused_grid(traj, CRITIC_WAVES): both 8, the evaluation pass included

Form = namedtuple("Form", "name waves share_old share_young")
EIGHT = Form("eight", 8, SHARE_OLD, SHARE_YOUNG)
EVAL = Form("eval", 16, 1, 1)


def n_tiles(B):
    return (B + TILE - 1) // TILE


def fused_grid(B, cus, walkers=GRID_WALKERS):
    """kernels.hpp fused_grid: one workgroup per `walkers` tiles, at most one per compute unit"""
    nb = (n_tiles(B) + walkers - 1) // walkers
    return min(nb, cus)


def per_workgroup(form):
    return (form.waves // 2) * (form.share_old + form.share_young)


def virtual_waves(B, cus, form=EIGHT):
    """n_waves of deal_tiles for the launch over B samples"""
    return fused_grid(B, cus) * per_workgroup(form)


def deal_tiles(form, workgroup, wave, grid):
    """bf16_tile.hpp deal_tiles (CHANNELS = 1) -> (share, first, n_waves)"""
    half = form.waves // 2
    per_wg = half * (form.share_old + form.share_young)
    share = form.share_old if wave < half else form.share_young
    first = workgroup * per_wg + (wave * form.share_old if wave < half
                                  else half * form.share_old + (wave - half) * form.share_young)
    return share, first, grid * per_wg


def walk_tiles(dealing, n_full, tail, two_buffers):
    """bf16_tile.hpp walk_tiles -> (tiles in the order tile() is called on them, tile indices load_tile() was asked for).
    The ragged tile is index n_full."""
    share, first, n_waves = dealing
    walked, loaded = [], []
    for vw in range(share):
        wave_id = first + vw
        if wave_id < n_full:
            loaded.append(wave_id)
            if not two_buffers:
                g = wave_id
                while g < n_full:
                    g1 = g + n_waves
                    loaded.append(g1 if g1 < n_full else g)
                    walked.append(g)
                    g += n_waves
            else:
                g = wave_id
                while g < n_full:
                    g1, g2 = g + n_waves, g + 2 * n_waves
                    loaded.append(g1 if g1 < n_full else g)
                    walked.append(g)
                    if g1 >= n_full:
                        break
                    loaded.append(g2 if g2 < n_full else g1)
                    walked.append(g1)
                    g += 2 * n_waves
        if tail != 0 and n_full % n_waves == wave_id:
            loaded.append(n_full)
            walked.append(n_full)
    return walked, loaded


def walk(B, cus, form=EIGHT, two_buffers=True, with_loads=False):
    """{(workgroup, wave): [tile, ...]} of the launch over B samples, every wave of the grid present"""
    grid, n_full, tail = fused_grid(B, cus), B // TILE, B % TILE
    out = {}
    for wg in range(grid):
        for wave in range(form.waves):
            walked, loaded = walk_tiles(deal_tiles(form, wg, wave, grid), n_full, tail, two_buffers)
            out[(wg, wave)] = (walked, loaded) if with_loads else walked
    return out


def owner(lists, tile):
    """the (workgroup, wave) whose list holds `tile`"""
    found = [k for k, tiles in lists.items() if tile in tiles]
    assert len(found) == 1, (tile, found)
    return found[0]


def flush_pattern(count, period):
    """(in-loop flushes, tiles left for the flush after the walk) of a real wave that walks `count` tiles.  The first
    flush of a wave stores, every later one adds; the flush after the walk runs when tiles are left or none ran."""
    return count // period, count % period


# ------------------------------------------------------------------------------------------------ the case table
Case = namedtuple("Case", "name B n T passes")
ALL_PASSES = ("policy", "fvp", "eval", "critic")


def shape_for(n_full, want_tail, hint=1):
    """B = 32 n_full (+ a tail) as lanes x steps: with a tail, the first tail from `hint` upwards (wrapping inside
    1..31) that makes B divisible by 7, 5 or 3, and that divisor as T — the observation plane's stride (T + 1) n is then
    not simply 2 B; without one T = 1."""
    if not want_tail:
        return n_full * TILE, n_full * TILE, 1
    for k in range(31):
        tail = (hint - 1 + k) % 31 + 1
        B = n_full * TILE + tail
        for T in (7, 5, 3):
            if B % T == 0:
                return B, B // T, T
    raise AssertionError("seven consecutive tails hold a multiple of 7")


def cases(cus):
    """The named sample counts, each the smallest with its property on a device of `cus` compute units (the properties:
    tests/test_tile_walk_model.py).  NV / NVE: virtual waves of the capped grid, eight-wave form / evaluation pass."""
    NV, NVE, cap = per_workgroup(EIGHT) * cus, per_workgroup(EVAL) * cus, GRID_WALKERS * cus
    out = []

    def add(name, n_full, tail, hint=1, passes=ALL_PASSES, shape=None):
        B, n, T = shape if shape is not None else shape_for(n_full, tail, hint)
        assert B // TILE == n_full and (B % TILE != 0) == bool(tail) and n * T == B
        out.append(Case(name, B, n, T, passes))

    # below one workgroup's worth of virtual waves
    add("B1", 0, True, shape=(1, 1, 1))
    add("B31", 0, True, shape=(31, 31, 1))
    add("B32", 1, False)
    add("B33", 1, True, shape=(33, 11, 3))
    add("tail-opens-wave-1", 5, True, hint=17)
    add("tail-opens-first-younger-wave", 20, True, hint=10)  # 650 = 20 x 32 + 10
    add("tail-opens-workgroup-1", 32, True, hint=29)
    # the grid's cap: 8 x cus tiles and one either side, with and without a tail
    for d, tag in ((-1, "cap-1"), (0, "cap"), (1, "cap+1")):
        add("grid-%s" % tag, cap + d, False)
        add("grid-%s-tail" % tag, cap + d, True, hint=3 + 9 * (d + 1))
    # second round of the eight-wave form
    add("second-round-NV-1-tail", NV - 1, True, hint=5)
    add("second-round-NV-tail", NV, True, hint=30)
    add("second-round-NV+1-tail", NV + 1, True, hint=13)
    add("second-round-2NV+1-tail", 2 * NV + 1, True, hint=22)
    # the policy kernels' flush period on real wave 0 (plays virtual waves 0-4) and on the first younger wave (20-22)
    add("policy-flush-wave0-16", 3 * NV + 1, False, passes=("policy", "fvp", "eval"))
    add("policy-flush-wave0-18-tail", 3 * NV + 2, True, hint=7, passes=("policy", "fvp", "eval"))
    add("policy-flush-younger-16", 5 * NV + 21, False, passes=("policy", "fvp", "eval"))
    add("policy-flush-younger-18-tail", 5 * NV + 22, True, hint=19, passes=("policy", "fvp", "eval"))
    # the critic step's
    add("critic-flush-wave0-64", 12 * NV + 4, False, passes=("critic",))
    add("critic-flush-wave0-65-tail", 12 * NV + 5, True, hint=11, passes=("critic",))
    # second round of the evaluation pass
    add("eval-NVE-1-tail", NVE - 1, True, hint=25)
    add("eval-NVE-tail", NVE, True, hint=2)
    add("eval-NVE+1-tail", NVE + 1, True, hint=16)
    add("eval-2NVE+1-tail", 2 * NVE + 1, True, hint=9)
    assert len({c.name for c in out}) == len(out)
    return out


def case_names():
    """the names alone (they do not depend on the compute-unit count)"""
    return [c.name for c in cases(256)]


def below_second_round(case, cus):
    """no virtual wave of the eight-wave form walks a second tile"""
    return n_tiles(case.B) <= virtual_waves(case.B, cus, EIGHT)


def probe_tiles(B, cus, form=EIGHT, period=PB_FLUSH, limit=8):
    """The tiles to light up one at a time: of the real wave with the most tiles and of the ragged tile's owner — the
    first tile, the tile that completes a flush period and the one after it (where the wave has them), the last tile;
    the ragged tile itself; tile n_full - 1; the first tile of the last workgroup.  In the order walked, at most
    `limit`, the ragged tile and the period's edge kept first when there are more."""
    lists = walk(B, cus, form)
    n_full, tail = B // TILE, B % TILE
    picks = []

    def take(t):
        if t is not None and t not in picks:
            picks.append(t)

    busiest = max(lists, key=lambda k: (len(lists[k]), -k[0], -k[1]))
    waves = [busiest] + ([owner(lists, n_full)] if tail else [])
    if tail:
        take(n_full)
    for k in waves:  # the period's edges first: they are what the cap must not drop
        tiles = lists[k]
        if len(tiles) > period:
            take(tiles[period - 1])
            take(tiles[period])
    if n_full > 0:
        take(n_full - 1)
    last_wg = max(wg for wg, _ in lists)
    take(next((lists[(last_wg, w)][0] for w in range(form.waves) if lists[(last_wg, w)]), None))
    for k in waves:
        take(lists[k][0])
        take(lists[k][-1])
    return picks[:limit]


def probes_for(case, cus, limit=8):
    """the probe tiles of a case: by the flush period of the kernels that run at it, and for the evaluation pass's cases
    half of them from its own form"""
    if case.passes == ("critic",):
        return probe_tiles(case.B, cus, EIGHT, C_FLUSH, limit)
    if not case.name.startswith("eval-"):
        return probe_tiles(case.B, cus, EIGHT, PB_FLUSH, limit)
    picks = probe_tiles(case.B, cus, EVAL, PB_FLUSH, limit // 2)
    return picks + [t for t in probe_tiles(case.B, cus, EIGHT, PB_FLUSH, limit) if t not in picks][:limit - len(picks)]
