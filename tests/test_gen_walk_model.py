"""tests/gen_walk_model.py checked against itself: the restated walk of k_gen_mfma and k_gen_pair reaches every tile of
every case exactly once, the launcher's row count is the number of walkers that write, each named case of `cases` has the
property it is named for and is the smallest count with it, the names do not depend on the compute-unit count, and every
shape stays inside the kernels' 32-bit element offsets for both input widths tests/test_gpu_gen_tile_walk.py uses."""
import pytest

import gen_walk_model as M

CUS = [8, 64, 256, 304]  # a small device, a mid one, the MI355X, a count that is no power of two
IN_DIMS = (5, 7)         # the input widths of tests/test_gpu_gen_tile_walk.py


def case(cus, name):
    return next(c for c in M.cases(cus) if c.name == name)


def tile_counts(B, cus, form):
    return {w: sum(t is not None for t in tiles) for w, tiles in M.walk(B, cus, form).items()}


@pytest.mark.parametrize("cus", CUS)
def test_every_tile_is_walked_exactly_once(cus):
    """... in both forms; a pair's idle iterations come after its live ones; the tile fetched ahead is a tile of the
    same walker or lies past the end"""
    for c in M.cases(cus):
        tiles, W = M.n_tiles(c.B), M.n_walkers(c.B, cus)
        assert W == M.WALKERS * M.grid(c.B, cus) and 1 <= M.grid(c.B, cus) <= cus
        for form in M.FORMS:
            lists, fetched_by = M.walk(c.B, cus, form), M.fetches(c.B, cus, form)
            assert sorted(lists) == list(range(W))
            walked = sorted(t for v in lists.values() for t in v if t is not None)
            assert walked == list(range(tiles)), (c.name, form)
            for w, v in lists.items():
                live = [t for t in v if t is not None]
                assert v[:len(live)] == live and live == list(range(w, tiles, W))
                if form == M.PAIR:
                    assert len(v) == M.iterations(c.B, cus) >= 1
                fetched = fetched_by[w]
                assert fetched[:len(live)] == live and len(fetched) == (len(v) + 1 if v else 0)
                assert all(t >= tiles for t in fetched[len(live):])


@pytest.mark.parametrize("cus", CUS)
def test_rows_are_the_walkers_that_write(cus):
    for c in M.cases(cus):
        for form in M.FORMS:
            wr = M.writers(c.B, cus, form)
            assert M.rows(c.B, cus, form) == len(wr), (c.name, form)
            assert wr == list(range(len(wr)))  # rows 0 .. last_rows - 1, none skipped: the reduction reads them all
        assert M.rows(c.B, cus, M.PAIR) == M.n_walkers(c.B, cus)
    for B in (1, 33, 129, 32 * 4 * cus - 1, 32 * 4 * cus + 1):
        assert M.rows(B, cus, M.WAVE) == min(M.n_tiles(B), M.n_walkers(B, cus))


@pytest.mark.parametrize("cus", CUS)
def test_shapes_of_the_cases(cus):
    table = M.cases(cus)
    assert [c.name for c in table] == M.case_names() and set(M.FLUSH_CASES) <= set(M.case_names())
    for c in table:
        assert c.n * c.T == c.B and c.B >= 1
        assert ("tail" in c.name or c.name in ("B1", "B31", "B33")) == (c.B % M.TILE != 0), c.name
        if c.B % M.TILE and c.B > 33:
            assert c.T in (3, 5, 7)  # the observation plane's stride (T + 1) n is not 2 B
            # the smallest sample count with this tile count that the factoring rule admits
            assert all(b % 3 and b % 5 and b % 7 for b in range(32 * (M.n_tiles(c.B) - 1) + 1, c.B))
        if c.B % M.TILE == 0:
            assert c.T == 1
        for in_dim in IN_DIMS:  # gen_mfma_fits: 32-bit element offsets
            assert (c.T + 1) * c.n * in_dim < 2 ** 30
    assert [case(cus, n).B for n in ("B1", "B31", "B32", "B33")] == [1, 31, 32, 33]
    assert [(case(cus, n).n, case(cus, n).T) for n in ("B1", "B31", "B32", "B33")] == [(1, 1), (31, 1), (32, 1), (11, 3)]


@pytest.mark.parametrize("cus", CUS)
def test_cases_below_the_cap(cus):
    for name in ("B1", "B31", "B32"):
        c = case(cus, name)
        assert M.grid(c.B, cus) == 1 and M.walk(c.B, cus, M.WAVE) == {0: [0], 1: [], 2: [], 3: []}
        assert M.walk(c.B, cus, M.PAIR) == {0: [0], 1: [None], 2: [None], 3: [None]}  # three pairs on zeros
        assert M.rows(c.B, cus, M.WAVE) == 1 and M.rows(c.B, cus, M.PAIR) == 4
    c = case(cus, "B33")
    assert M.walk(c.B, cus, M.PAIR) == {0: [0], 1: [1], 2: [None], 3: [None]} and M.rows(c.B, cus, M.WAVE) == 2
    c = case(cus, "wg-4")
    assert c.B == 128 and M.grid(c.B, cus) == 1 and set(tile_counts(c.B, cus, M.PAIR).values()) == {1}
    assert M.grid(c.B - 1, cus) == 1 and M.n_tiles(c.B - 32) == 3  # the smallest count that fills a workgroup
    c = case(cus, "wg-5-tail")
    assert M.n_tiles(c.B) == 5 and c.B // 32 == 4 and M.grid(c.B, cus) == 2 and M.grid(128, cus) == 1
    assert M.walk(c.B, cus, M.PAIR)[4] == [4] and [M.walk(c.B, cus, M.PAIR)[w] for w in (5, 6, 7)] == [[None]] * 3
    assert M.rows(c.B, cus, M.WAVE) == 5 == M.n_tiles(c.B) and M.rows(c.B, cus, M.PAIR) == 8


@pytest.mark.parametrize("cus", CUS)
def test_cases_at_the_grid_cap(cus):
    W = 4 * cus
    for tag, tiles in (("cap-1", W - 1), ("cap", W), ("cap+1", W + 1)):
        for tail in ("", "-tail"):
            c = case(cus, tag + tail)
            assert M.n_tiles(c.B) == tiles and M.grid(c.B, cus) == cus and M.n_walkers(c.B, cus) == W
            for form in M.FORMS:
                counts = tile_counts(c.B, cus, form)
                if tag == "cap-1":  # the last walker of the last workgroup has no tile; the wave form writes W - 1 rows
                    assert counts[W - 1] == 0 and set(list(counts.values())[:-1]) == {1}
                    assert M.rows(c.B, cus, M.WAVE) == W - 1 and M.walk(c.B, cus, M.PAIR)[W - 1] == [None]
                elif tag == "cap":
                    assert set(counts.values()) == {1} and M.iterations(c.B, cus) == 1 and M.below_second_round(c, cus)
                else:  # walker 0 alone has a second tile; in the pair form the other W - 1 run it on zeros
                    assert counts[0] == 2 and set(list(counts.values())[1:]) == {1} and not M.below_second_round(c, cus)
                    pairs = M.walk(c.B, cus, M.PAIR)
                    assert pairs[0] == [0, W] and all(pairs[w] == [w, None] for w in range(1, W))
                    assert M.walk(c.B, cus, M.WAVE)[1] == [1]  # a wave does not run the idle iteration
            if tail:
                assert c.B // 32 == tiles - 1  # the ragged tile is the last of the named count
    assert M.grid(32 * (W - 4), cus) == cus - 1 and M.grid(32 * (W - 4) + 1, cus) == cus  # where the cap is first met


@pytest.mark.parametrize("cus", CUS)
def test_case_of_uneven_rounds(cus):
    W = 4 * cus
    c = case(cus, "rounds-2.5-tail")
    assert M.n_tiles(c.B) == 2 * W + W // 2 + 1 and M.iterations(c.B, cus) == 3
    for form in M.FORMS:
        counts = tile_counts(c.B, cus, form)
        assert [counts[w] for w in (0, W // 2, W // 2 + 1, W - 1)] == [3, 3, 2, 2]
        assert sum(1 for k in counts.values() if k == 3) == W // 2 + 1
    assert M.walk(c.B, cus, M.PAIR)[W // 2] == [W // 2, W // 2 + W, c.B // 32]  # the ragged tile: a third tile
    assert M.walk(c.B, cus, M.PAIR)[W - 1][-1] is None


@pytest.mark.parametrize("cus", CUS)
def test_cases_of_the_flush_period(cus):
    W = 4 * cus
    store, add = "store", "add"
    assert M.flush_pattern(1) == [(store, 1)] and M.flush_pattern(63) == [(store, 63)]
    assert M.flush_pattern(64) == [(store, 64)] and M.flush_pattern(65) == [(store, 64), (add, 1)]
    assert M.flush_pattern(130) == [(store, 64), (add, 64), (add, 2)] and M.flush_pattern(128) == [(store, 64), (add, 64)]

    def adders(B, form):
        """walkers with an adding flush: by iterations in the pair form (idle ones count), by tiles in the wave form"""
        return [w for w, v in M.walk(B, cus, form).items() if v and len(M.flush_pattern(len(v))) > 1]

    c = case(cus, "flush-63-tail")
    assert M.n_tiles(c.B) == 64 * W - 1 and M.iterations(c.B, cus) == 64
    for form in M.FORMS:
        counts = tile_counts(c.B, cus, form)
        assert counts[W - 1] == 63 and set(list(counts.values())[:-1]) == {64} and not adders(c.B, form)
    assert M.walk(c.B, cus, M.WAVE)[W - 2][-1] == c.B // 32  # the ragged tile is a walker's 64th: it completes a period
    assert M.walk(c.B, cus, M.PAIR)[W - 1][-1] is None        # the last pair's 64th iteration is idle, its one flush stores
    c = case(cus, "flush-64")
    assert c.B == 32 * 64 * W and all(set(tile_counts(c.B, cus, f).values()) == {64} for f in M.FORMS)
    assert not adders(c.B, M.WAVE) and not adders(c.B, M.PAIR)  # one flush each, the storing one
    if cus == 256:
        assert c.B == 16384 * 128  # the count tests/test_gpu_fullsize.py runs
    for name in ("flush-65", "flush-65-tail"):
        c = case(cus, name)
        assert M.n_tiles(c.B) == 64 * W + 1 and M.iterations(c.B, cus) == 65
        # the smallest count with an adding flush: one tile fewer has none in either form
        assert not adders(32 * 64 * W, M.WAVE) and not adders(32 * 64 * W, M.PAIR)
        assert adders(c.B, M.WAVE) == [0]                    # wave 0 alone adds: its 65th tile
        assert adders(c.B, M.PAIR) == list(range(W))         # every pair adds; all but pair 0 add an idle iteration's zeros
        pairs = M.walk(c.B, cus, M.PAIR)
        assert pairs[0][64] == 64 * W and all(pairs[w][64] is None and None not in pairs[w][:64] for w in range(1, W))
        if "tail" in name:
            assert c.B // 32 == 64 * W  # the ragged tile is the only tile of walker 0's second period
    c = case(cus, "flush-all-65-tail")
    assert M.n_tiles(c.B) == 65 * W + W // 2 + 3 and M.iterations(c.B, cus) == 66
    for form in M.FORMS:
        counts = tile_counts(c.B, cus, form)
        assert set(counts.values()) == {65, 66} and counts[W // 2 + 2] == 66 and counts[W // 2 + 3] == 65
        assert adders(c.B, form) == list(range(W))
    assert adders(32 * (65 * W - 1), M.WAVE) == list(range(W - 1))  # below 65 W tiles the last wave has no adding flush
    assert M.owner_of(c.B, cus, c.B // 32) == W // 2 + 2 and M.walk(c.B, cus, M.WAVE)[W // 2 + 2][-1] == c.B // 32
    assert [M.flush_pattern(k) for k in (65, 66)] == [[(store, 64), (add, 1)], [(store, 64), (add, 2)]]


@pytest.mark.parametrize("cus", CUS)
def test_probe_tiles(cus):
    W = 4 * cus
    for c in M.cases(cus):
        tiles, n_full = M.n_tiles(c.B), c.B // 32
        for form in M.FORMS:
            picks = M.probe_tiles(c, cus, form)
            assert 1 <= len(picks) <= 8 and len(set(picks)) == len(picks) and all(0 <= t < tiles for t in picks)
            if c.B % 32:
                assert picks[0] == n_full  # the ragged tile itself
            if n_full > 0:
                assert n_full - 1 in picks
            assert 0 in picks  # walker 0 is the busiest: its first tile
            assert M.probe_tiles(c, cus, form, limit=3) == picks[:3]
            assert picks == M.probe_tiles(c, cus, M.WAVE)  # the live tiles of a pair are the tiles of the wave
    for name in ("flush-65", "flush-65-tail"):
        c = case(cus, name)
        # walker 0: first, 64th, 65th (= last); the last walker's 64th, after which a pair runs on zeros and flushes again
        assert {0, 63 * W, 64 * W, 64 * W - 1} <= set(M.probe_tiles(c, cus, M.PAIR))
        assert M.owner_of(c.B, cus, 64 * W - 1) == W - 1
    c = case(cus, "flush-all-65-tail")
    assert {0, 63 * W, 64 * W, 65 * W, c.B // 32, c.B // 32 - 1, W - 4} <= set(M.probe_tiles(c, cus, M.PAIR))
    c = case(cus, "wg-5-tail")
    assert M.probe_tiles(c, cus, M.PAIR) == [4, 0, 3]  # tile 4 is also the first of the last workgroup
    c = case(cus, "cap+1")
    assert M.probe_tiles(c, cus, M.PAIR) == [0, W, W - 4]  # tile W: walker 0's second and last, and tile n_full - 1
