"""The case table and the f64 reference of tests/test_gpu_ppo_clip.py, checked without a device: the hand-written
d loss / d logits against torch autograd, the conditions every row's inputs must meet for the device test to mean anything
(conditions on the inputs, not measurements of the kernels), and that each row tells a wrong clipping rule from the right
one."""
import numpy as np
import pytest
import torch

import ppo_clip_cases as pc

ROW_IDS = [r.name for r in pc.ROWS]


def test_the_table_covers_every_statement_within_the_size_limits():
    assert len(set(ROW_IDS)) == len(ROW_IDS)
    assert {s for r in pc.ROWS for s in r.statement.values()} == {"fused", "gen", "terms", "seq"}
    for r in pc.ROWS:
        assert 256 <= r.n * r.T <= 1024, r.name
        if r.kind == "rnn" and r.spec[1:5] == (5, 128, 1, 128):  # the default GruMlp / LstmMlp kernels
            assert r.n % 32 == 0, r.name
        assert pc.initial_params(r.name).shape == (pc.blocks(r)[-1][1].stop,)
    assert {pc.actions_of(r) for r in pc.ROWS} >= {2, 3, 5, 8}
    assert {r.kind for r in pc.ROWS} == {"mlp", "rnn", "lin"} and any(r.spec[3] == "Tanh" for r in pc.ROWS if r.kind == "mlp")


@pytest.mark.parametrize("clip", pc.CLIPS)
def test_the_rule_at_ties_and_in_every_region_is_autograds(clip):
    """d min(r A, clamp(r, lo, hi) A) / d r with r given exactly — on either bound, at exactly 1, and in every region for
    both signs of A and A = 0: minimum() splits a tie, clamp() passes the gradient at its bounds"""
    lo, hi = pc.clip_bounds(clip)
    r = np.array([lo, hi, 1.0, np.nextafter(lo, -9.0), np.nextafter(lo, 9.0), np.nextafter(hi, -9.0), np.nextafter(hi, 9.0),
                  lo - 0.3, hi + 0.3, 0.5 * (lo + hi), 0.0, 7.0])
    ratio = np.repeat(r, 3)
    adv = np.tile(np.array([1.7, -0.6, 0.0]), len(r))
    rt = torch.tensor(ratio, requires_grad=True)
    at = torch.tensor(adv)
    torch.minimum(rt * at, torch.clamp(rt, lo, hi) * at).sum().backward()
    assert np.array_equal(pc.pass_weight(ratio, adv, lo, hi), rt.grad.numpy())
    assert min(pc.census(ratio, adv, lo, hi)) > 0 or clip == 4.0  # (nothing lies below a negative bound)


@pytest.mark.parametrize("A", [2, 3, 5, 8])
@pytest.mark.parametrize("clip", pc.CLIPS)
def test_handwritten_dlogits_against_autograd(A, clip):
    """the NumPy d loss / d logits equals torch autograd of the clipped surrogate with respect to the logits within 1e-12,
    with samples in every region and (clip 0.2) samples whose ratio is 1: log pi_0 = log pi"""
    lo, hi = pc.clip_bounds(clip)
    rng = np.random.default_rng(A)
    B = 400
    logits = rng.normal(size=(A, B)) * 2.0
    a = rng.integers(0, A, size=B)
    adv = rng.normal(size=B)
    lpa = np.take_along_axis(pc.log_softmax(logits), a[None], axis=0)[0]
    lp0a = lpa - rng.normal(size=B) * 0.4
    if clip == 0.2:
        lp0a[:40] = lpa[:40]
    dz, loss, ratio = pc.dloss_dlogits(logits, lp0a, a, adv, lo, hi)
    counts = pc.census(ratio, adv, lo, hi)
    assert pc.margin(ratio, lo, hi) > 1e-9  # ties are the test above's
    assert min(counts[1:]) >= 10 or clip == 4.0
    assert (counts[0] >= 40 and (ratio[:40] == 1.0).all()) if clip == 0.2 else True
    zt = torch.tensor(logits, requires_grad=True)
    lp = torch.log_softmax(zt, dim=0)
    rt = torch.exp(lp.gather(0, torch.tensor(a)[None])[0] - torch.tensor(lp0a))
    at = torch.tensor(adv)
    lt = -torch.minimum(rt * at, torch.clamp(rt, lo, hi) * at).mean()
    lt.backward()
    assert np.abs(dz - zt.grad.numpy()).max() <= 1e-12 and abs(loss - lt.item()) <= 1e-12
    assert np.abs(dz).max() > 1e-4


@pytest.mark.parametrize("name", ROW_IDS)
def test_conditions_on_the_inputs(name):
    """At the reference's own p1 — one SGD step at the row's rate from p0: with clip 0.2 each of the four outside regions
    holds at least 5 % of the samples and the inside at least 15 %; with clip 0.0 each outside region holds 5 %; no ratio
    lies within 1e-4 of a bound of any clip; the wide clip clips nothing, so its reference is the unclipped surrogate's
    gradient; every parameter block has a gradient; and a feed-forward row's two routes to the reference — torch autograd
    of the loss, and the hand-written d loss / d logits through the transposed Jacobian — agree."""
    row = pc.BY_NAME[name]
    B = row.n * row.T
    ref = {clip: pc.reference_at_own_step(name, clip) for clip in pc.CLIPS}
    print(name, {clip: (r["census"], "%.3g" % r["margin"]) for clip, r in ref.items()})
    c = ref[0.2]["census"]
    assert sum(c) == B and min(c[1:]) >= 0.05 * B and c[0] >= 0.15 * B, c
    c = ref[0.0]["census"]
    assert c[0] == 0 and min(c[1:]) >= 0.05 * B, c
    for clip in pc.CLIPS:
        assert ref[clip]["margin"] > pc.MARGIN, (clip, ref[clip]["margin"])
        for blk, s in pc.blocks(row):
            assert np.abs(ref[clip]["grad"][s]).max() > 0, (clip, blk)
    assert ref[4.0]["census"] == (B, 0, 0, 0, 0)
    p0, p1 = pc.initial_params(name), pc.reference_first_step(name)
    assert not np.array_equal(p0, p1)
    lp0a = pc.logp0_of(row, p0)
    h = pc.history(name)
    a = (h["action"].reshape(-1) if row.kind == "mlp" else h["action"]).astype(np.int64)
    dz, loss, _ = pc.dloss_dlogits(pc.logits64(row, p1), lp0a, a, ref[4.0]["adv"], -1e300, 1e300)
    assert pc.rel_err(ref[4.0]["grad"], pc.vjp(row, p1, dz)) <= 1e-12 and abs(loss - ref[4.0]["loss"]) <= 1e-12
    if row.kind == "mlp":
        lo, hi = pc.clip_bounds(0.2)
        dz, loss, _ = pc.dloss_dlogits(pc.logits64(row, p1), lp0a, a, ref[0.2]["adv"], lo, hi)
        assert pc.rel_err(pc.vjp(row, p1, dz), ref[0.2]["grad"]) <= 1e-12 and abs(loss - ref[0.2]["loss"]) <= 1e-12


@pytest.mark.parametrize("name", ROW_IDS)
def test_the_cases_discriminate(name):
    """each deliberately wrong rule — no mask, max for min, the clipped side following the bound alone whatever the
    advantage's sign — gives a gradient at least 0.1 of max |g| from the right one, with clip 0.2 and with clip 0.0.
    With clip 4.0 every sample is inside (the test above), u1 = u2 on every sample and all three wrong rules, max for min
    included, coincide with the right one: that case holds the bounds' arithmetic (a negative lower bound), not the mask."""
    for clip in (0.2, 0.0):
        g = pc.reference_at_own_step(name, clip)["grad"]
        for mutant in pc.MUTANTS:
            d = pc.rel_err(pc.reference_at_own_step(name, clip, mutant)["grad"], g)
            print("%s clip %.1f %s: %.2f of max|g|" % (name, clip, mutant, d))
            assert d >= 0.1, (clip, mutant, d)
    g = pc.reference_at_own_step(name, 4.0)["grad"]
    for mutant in pc.MUTANTS:
        assert pc.rel_err(pc.reference_at_own_step(name, 4.0, mutant)["grad"], g) <= 1e-12
