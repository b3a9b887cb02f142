"""tests/tile_walk_model.py checked against itself: the restated walk reaches every tile exactly once and never asks for
a tile past the last, each named case of `cases` has the property it is named for — in terms of the per-wave tile lists —
and the dealing that the docstring of tests/test_gpu_fused_bits.py states for its three shapes is what the model gives."""
import pytest

import tile_walk_model as M

CUS = [256, 8, 304]  # the MI355X, a small device (the cap at 64 tiles), a count that is no power of two


def case(cus, name):
    return next(c for c in M.cases(cus) if c.name == name)


def counts(lists):
    return {k: len(v) for k, v in lists.items()}


@pytest.mark.parametrize("cus", CUS)
def test_every_tile_is_walked_exactly_once(cus):
    """... in both forms and through both loops of walk_tiles, which agree on the order; load_tile is only ever asked for
    a tile that exists, and for the ragged tile only by its owner"""
    for c in M.cases(cus):
        tiles = M.n_tiles(c.B)
        for form in (M.EIGHT, M.EVAL):
            two = M.walk(c.B, cus, form, two_buffers=True, with_loads=True)
            one = M.walk(c.B, cus, form, two_buffers=False, with_loads=True)
            assert len(two) == M.fused_grid(c.B, cus) * form.waves
            walked = sorted(t for w, _ in two.values() for t in w)
            assert walked == list(range(tiles)), (c.name, form.name)
            for k in two:
                assert two[k][0] == one[k][0], (c.name, form.name, k)
                for w, loaded in (two[k], one[k]):
                    assert all(0 <= t < tiles for t in loaded) and set(w) <= set(loaded)
                    assert (c.B // M.TILE in loaded) == (c.B % M.TILE != 0 and c.B // M.TILE in w)


@pytest.mark.parametrize("cus", CUS)
def test_shapes_of_the_cases(cus):
    table = M.cases(cus)
    assert [c.name for c in table] == M.case_names()
    for c in table:
        assert c.n * c.T == c.B and c.B >= 1
        if c.B % M.TILE and c.B > 33:
            assert c.T in (3, 5, 7)  # the observation plane's stride (T + 1) n is not 2 B
        if c.B % M.TILE == 0:
            assert c.T == 1
        assert ("tail" in c.name or c.name in ("B1", "B31", "B33")) == (c.B % M.TILE != 0), c.name
    assert [case(cus, n).B for n in ("B1", "B31", "B32", "B33")] == [1, 31, 32, 33]
    assert case(cus, "tail-opens-first-younger-wave").B == 650
    # only the critic step runs at the two largest counts, and it runs at every other but the policy kernels' flush cases
    assert [c.name for c in table if c.passes == ("critic",)] == ["critic-flush-wave0-64", "critic-flush-wave0-65-tail"]
    assert max(table, key=lambda c: c.B).name == "critic-flush-wave0-65-tail"


@pytest.mark.parametrize("cus", CUS)
def test_cases_below_one_workgroup(cus):
    for name in ("B1", "B31"):
        lists = M.walk(case(cus, name).B, cus)
        assert counts(lists) == {(0, w): int(w == 0) for w in range(8)} and lists[(0, 0)] == [0]  # the ragged tile alone
    assert M.walk(32, cus)[(0, 0)] == [0] and M.walk(33, cus)[(0, 0)] == [0, 1]
    c = case(cus, "tail-opens-wave-1")
    lists = M.walk(c.B, cus)
    assert c.B // 32 == 5 and M.fused_grid(c.B, cus) == 1
    assert lists[(0, 0)] == [0, 1, 2, 3, 4] and lists[(0, 1)] == [5] and not any(lists[(0, w)] for w in range(2, 8))
    c = case(cus, "tail-opens-first-younger-wave")
    lists = M.walk(c.B, cus)
    assert c.B // 32 == 20 and all(len(lists[(0, w)]) == 5 for w in range(4)) and lists[(0, 4)] == [20]
    c = case(cus, "tail-opens-workgroup-1")
    lists = M.walk(c.B, cus)
    assert c.B // 32 == 32 and M.fused_grid(32 * 32, cus) == 4 and M.fused_grid(c.B, cus) == 5
    assert [len(lists[(0, w)]) for w in range(8)] == [5, 5, 5, 5, 3, 3, 3, 3]
    assert lists[(1, 0)] == [32] and sum(len(v) for k, v in lists.items() if k[0] >= 1) == 1
    # ... and in the evaluation pass, 16 virtual waves per workgroup on the same grid, the ragged tile's owner differs
    assert M.owner(M.walk(c.B, cus, M.EVAL), 32) == (2, 0)


@pytest.mark.parametrize("cus", CUS)
def test_cases_at_the_grid_cap(cus):
    uncapped = {}
    for tag in ("cap-1", "cap", "cap+1"):
        for tail in ("", "-tail"):
            c = case(cus, "grid-" + tag + tail)
            assert M.fused_grid(c.B, cus) == cus
            uncapped[tag + tail] = (M.n_tiles(c.B) + 7) // 8
            lists = M.walk(c.B, cus)
            # no virtual wave loops: a quarter of the workgroups (and one more past 8 x cus tiles) hold all the tiles
            assert all(len(v) <= (5 if w < 4 else 3) for (_, w), v in lists.items()) and M.below_second_round(c, cus)
            busy = {g for (g, _), v in lists.items() if v}
            assert busy == set(range((M.n_tiles(c.B) + 31) // 32)) and len(busy) in (cus // 4, cus // 4 + 1)
    assert M.n_tiles(case(cus, "grid-cap").B) == 8 * cus
    assert [uncapped[k] - cus for k in ("cap-1", "cap-1-tail", "cap", "cap-tail", "cap+1", "cap+1-tail")] == [0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("cus", CUS)
def test_cases_of_the_second_round(cus):
    NV = 32 * cus
    last = (cus - 1, 7)
    c = case(cus, "second-round-NV-1-tail")
    lists = M.walk(c.B, cus)
    assert M.virtual_waves(c.B, cus) == NV and c.B // 32 == NV - 1
    # one tile on every virtual wave; the ragged tile is the only one of the last virtual wave, on the last younger wave
    assert all(len(lists[(g, w)]) == (5 if w < 4 else 3) for g, w in lists) and lists[last] == [NV - 3, NV - 2, NV - 1]
    assert M.below_second_round(c, cus)
    c = case(cus, "second-round-NV-tail")
    assert c.B // 32 == NV and M.walk(c.B, cus)[(0, 0)] == [0, NV, 1, 2, 3, 4] and not M.below_second_round(c, cus)
    c = case(cus, "second-round-NV+1-tail")
    assert M.walk(c.B, cus)[(0, 0)] == [0, NV, 1, NV + 1, 2, 3, 4]  # virtual wave 0 loops twice, the tail is wave 1's
    c = case(cus, "second-round-2NV+1-tail")
    lists = M.walk(c.B, cus)
    assert lists[(0, 0)] == [0, NV, 2 * NV, 1, NV + 1, 2 * NV + 1, 2, NV + 2, 3, NV + 3, 4, NV + 4]
    assert lists == M.walk(c.B, cus, two_buffers=False)  # third iteration of one loop, second of the other


@pytest.mark.parametrize("cus", CUS)
def test_cases_of_the_flush_periods(cus):
    NV = 32 * cus

    def longest(B):
        return max(counts(M.walk(B, cus)).values())

    c = case(cus, "policy-flush-wave0-16")
    lists = M.walk(c.B, cus)
    assert len(lists[(0, 0)]) == 16 == longest(c.B) and longest(c.B - 32) == 15
    assert M.flush_pattern(16, M.PB_FLUSH) == (1, 0)  # one flush in the loop, none after it
    c = case(cus, "policy-flush-wave0-18-tail")
    lists = M.walk(c.B, cus)
    assert len(lists[(0, 0)]) == 18 and M.flush_pattern(18, M.PB_FLUSH) == (1, 2)  # the flush after the walk must ADD
    assert M.owner(lists, c.B // 32) == (0, 0) and lists[(0, 0)].index(c.B // 32) == 11  # the tail: vw 2's, before the flush
    assert len(lists[(0, 4)]) < 16
    c = case(cus, "policy-flush-younger-16")
    lists = M.walk(c.B, cus)
    assert len(lists[(0, 4)]) == 16 and len(M.walk(c.B - 32, cus)[(0, 4)]) == 15 and len(lists[(0, 0)]) == 30
    c = case(cus, "policy-flush-younger-18-tail")
    lists = M.walk(c.B, cus)
    assert len(lists[(0, 4)]) == 18 and lists[(0, 4)][-1] == c.B // 32  # the ragged tile is the remainder's last
    for name in ("policy-flush-wave0-16", "policy-flush-younger-18-tail"):
        assert "critic" not in case(cus, name).passes
    c = case(cus, "critic-flush-wave0-64")
    lists = M.walk(c.B, cus)
    assert len(lists[(0, 0)]) == 64 == longest(c.B) and longest(c.B - 32) == 63
    assert M.flush_pattern(64, M.C_FLUSH) == (1, 0)
    c = case(cus, "critic-flush-wave0-65-tail")
    lists = M.walk(c.B, cus)
    assert len(lists[(0, 0)]) == 65 and len(lists[(0, 1)]) == 61 and M.owner(lists, c.B // 32) == (0, 1)
    assert c.B // 32 == 12 * NV + 5


@pytest.mark.parametrize("cus", CUS)
def test_cases_of_the_evaluation_pass(cus):
    NVE = 16 * cus
    c = case(cus, "eval-NVE-1-tail")
    lists = M.walk(c.B, cus, M.EVAL)
    assert M.virtual_waves(c.B, cus, M.EVAL) == NVE and set(counts(lists).values()) == {1} and lists[(cus - 1, 15)] == [NVE - 1]
    c = case(cus, "eval-NVE-tail")
    assert M.walk(c.B, cus, M.EVAL)[(0, 0)] == [0, NVE]
    c = case(cus, "eval-NVE+1-tail")
    lists = M.walk(c.B, cus, M.EVAL)
    assert lists[(0, 0)] == [0, NVE] and lists[(0, 1)] == [1, NVE + 1]
    c = case(cus, "eval-2NVE+1-tail")
    lists = M.walk(c.B, cus, M.EVAL)
    assert lists[(0, 0)] == [0, NVE, 2 * NVE] and lists[(0, 1)] == [1, NVE + 1, 2 * NVE + 1]
    # the evaluation pass has its second round where the eight-wave form still has none
    assert M.below_second_round(case(cus, "eval-NVE+1-tail"), cus) and not M.below_second_round(c, cus)


def test_the_dealing_test_gpu_fused_bits_states():
    """its docstring, at 256 compute units: 64 x 16 — 32 full tiles, fewer than one workgroup's virtual waves, most waves
    walk nothing; 50 x 13 — 20 full tiles and a ragged tile of 10 samples on the wave whose turn it is;
    32768 x 128 — 131,072 tiles, an older wave walks 80 (and a younger one 48), past both flush periods"""
    lists = M.walk(64 * 16, 256)
    assert M.n_tiles(64 * 16) == 32 and M.fused_grid(64 * 16, 256) == 4
    assert sum(1 for v in lists.values() if v) == 8 and sum(1 for v in lists.values() if not v) == 24
    B = 50 * 13
    lists = M.walk(B, 256)
    assert (B // 32, B % 32) == (20, 10) and M.owner(lists, 20) == (0, 4) and (20 % M.virtual_waves(B, 256)) == 20
    B = 32768 * 128
    lists = M.walk(B, 256)
    assert M.n_tiles(B) == 131072 and B % 32 == 0
    assert {len(lists[(g, w)]) for g in range(256) for w in range(4)} == {80}
    assert {len(lists[(g, w)]) for g in range(256) for w in range(4, 8)} == {48}
    assert M.flush_pattern(80, M.PB_FLUSH) == (5, 0) and M.flush_pattern(80, M.C_FLUSH) == (1, 16)


@pytest.mark.parametrize("cus", CUS)
def test_probe_tiles(cus):
    for c in M.cases(cus):
        for form, period in ((M.EIGHT, M.PB_FLUSH), (M.EIGHT, M.C_FLUSH), (M.EVAL, M.PB_FLUSH)):
            picks = M.probe_tiles(c.B, cus, form, period)
            tiles, n_full = M.n_tiles(c.B), c.B // 32
            assert 1 <= len(picks) <= 8 and len(set(picks)) == len(picks) and all(0 <= t < tiles for t in picks)
            if c.B % 32:
                assert picks[0] == n_full  # the ragged tile itself
            if n_full > 0 and tiles > 8:
                assert n_full - 1 in picks
    c = case(cus, "policy-flush-wave0-18-tail")
    wave0 = M.walk(c.B, cus)[(0, 0)]
    picks = M.probe_tiles(c.B, cus)
    assert {wave0[0], wave0[15], wave0[16], wave0[-1], c.B // 32} <= set(picks)
    c = case(cus, "critic-flush-wave0-65-tail")
    wave0 = M.walk(c.B, cus)[(0, 0)]
    assert {wave0[0], wave0[63], wave0[64]} <= set(M.probe_tiles(c.B, cus, M.EIGHT, M.C_FLUSH))
