"""The gradients that rl_dqn_update computes step by step, against a float64 chain that shares no code with the kernels.

k_dqn_step_bf16 (one-step TD targets formed inside the gradient launch) is reached only from rl_dqn_update, and the
reward-to-go update takes k_critic_step_mfma<2> through the same all-at-once path; tests/test_gpu_dqn.py sees both only
through six Adam steps at one shape.  Here the device agent runs plain SGD (no momentum, no weight decay, a power of two
as learning rate), so (p0 - pK) / lr IS the sum of the K gradients the update computed, up to the f32 rounding of each
parameter write, and the loss of step k depends on the targets at the parameters of step k.

The reference: the oracle's store and sampler (bit-identical to the device's, tests/test_gpu_dqn.py) give the episodes of
the K minibatches; everything after that is float64 NumPy — targets (one-step TD: r + gamma max_a Q_p(s') with the
chain's current parameters, 0 beyond a Terminate, successor = the stored Interrupt successor or else the next stored
step; reward-to-go: the discounted sum to the episode's end), gradient and loss of mean((Q_p(s)[a] - target)^2), and
p <- p - lr g.  Beside it the same chain in f32 (the oracle's f32 targets and gradient, tests/optim_ref.py's SGD): its
distance e32 from the f64 chain is the measured size of f32 rounding on this problem.

Bars, with rel(a, b) = max|a - b| / max|b|:
  1. summed gradient: rel((p0 - pK_device) / lr, (p0 - pK_f64) / lr) <= GRAD_RTOL + 2 e32 (GRAD_RTOL: the bar of one
     device gradient against f64; no farther from f64 than twice the f32 restatement, the TRPO tests' rule);
  2. every step's loss: |loss_device[k] - loss_f64[k]| <= 2e-5 loss_f64[k] (test_update_against_oracle's bar);
  3. each of W1, b1, W2, b2 on its own, relative to the block's maximum (> 0): 50 (GRAD_RTOL + 2 e32) (the factor of
     test_policy_gradient_through_time) — db2 has the largest entries and would hide an error in dW1;
  4. the data (asserted, not tolerances): every minibatch holds both actions and a Terminate, an Interrupt and a Continue
     successor, its step count is no multiple of 32, and its tile count is the one the case is named for.

Cases (C compute units; both kernels' grids are min(ceil(tiles / 4), C) workgroups of four tile walkers, tile g goes to
walker g mod 4 x grid):
  20 steps, K = 3            one ragged tile: three of four waves walk nothing and still define their image; K = 3 spans
                             two draw chunks (2 + 1)
  150 steps, K = 3           5 tiles on 2 workgroups, the second holds one tile, ragged
  32 x 4C + 40, K = 2        4C + 2 tiles: two waves walk two tiles (the second walk of wave 1 is the ragged last tile),
                             every other wave prefetches past the end
  32 x 16 x 4C + 1, K = 2    16 x 4C + 1 tiles, TD only: wave 0 walks 17 (a flush mid-walk, then a final flush of one
                             tile), the others exactly 16 (the period ends on the last tile: no final flush).  (The pair
                             kernel's period is 64 tiles per wave — two million steps — and is left out.)

Observed on an MI355X (256 CUs), lr = 2^-4 (nothing on the device asked for another); bar 1 is 2.1e-6 to 2.2e-6, bar 3
fifty times that, and nothing comes close to either:
  case (steps per minibatch)           e32      device vs f64   worst block (W1)   worst loss difference
  one-step TD    20, 29, 22            7.4e-8   7.4e-8          2.8e-7             9.4e-8
  reward-to-go   20, 29, 22            7.7e-8   5.9e-8          1.8e-7 (b1)        1.1e-7
  one-step TD    151, 156, 150         9.6e-8   6.5e-8          2.9e-7             3.7e-8
  reward-to-go   151, 156, 150         6.4e-8   6.4e-8          1.5e-7             1.0e-7
  one-step TD    32810, 32810          7.6e-8   7.3e-8          3.2e-7             3.0e-8
  reward-to-go   32810, 32810          5.5e-8   5.5e-8          1.6e-7             1.2e-7
  one-step TD    524291, 524292        (7.6e-8) 6.9e-8          2.9e-7             5.9e-8
(Where the device's distance equals e32 to the digits shown, both are the f32 rounding of the same parameter write: half
an ulp of a parameter of 0.2, over lr and max|g|, is what the summed gradient resolves — a thirtieth of bar 1.)
On the CPU, with the f32 chain in the device's place, a f64 chain that ignores Terminate, takes gamma = 1, drops the
last B mod 32 samples or drops one tile misses bar 1 by a factor of 3 (the three last samples of 524,291) to 100,000.
"""
import numpy as np
import pytest

import oracle as O
from optim_ref import sgd_step

pytestmark = pytest.mark.gpu

ra = pytest.importorskip("relearn_amd")

from test_gpu_dqn import GRAD_RTOL, KEY, make  # noqa: E402

LR = 2.0 ** -4  # max|g| is about 1.5: moderate steps, and the factor is exact
GAMMA = float(np.float32(0.99))  # the discount factor the agent is configured with (a float in the C ABI)
H = 128
BLOCKS = {"W1": slice(0, 5 * H), "b1": slice(5 * H, 6 * H), "W2": slice(6 * H, 8 * H), "b2": slice(8 * H, 8 * H + 2)}
SMALL = dict(n=64, capacity=64, horizon=40)    # collections: lanes, ring capacity, steps per lane (nothing is evicted)
LARGE = dict(n=256, capacity=96, horizon=70)
# The 20-step case draws two or three episodes, off lanes 0, 1 (and 2).  The only Interrupt successor of such a lane is,
# but for the rare episode that reaches the step limit, its last stored step (the horizon rule), and KEY's first draws
# land on the first and second episode of lanes 0 and 1: the first minibatch has no Interrupt, whatever the env and actor
# seeds (none in 64,000 pairs).  So this case has an agent key of its own, found on the CPU with the oracle alone: KEY with
# another third word, the first from 0 up for which each of the three minibatches has a Terminate and an Interrupt and
# fits one tile, and the first has the 20 steps asked for (20, 29 and 22 steps; 5, 14 and 48 give 29 or 22 first).
KEY_20 = KEY[:2] + [49] + KEY[3:]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / np.abs(b).max()


# ---------------------------------------------------------------- the reference (CPU only)
def oracle_agent(coll, minibatch, td, key):
    """the oracle half of test_gpu_dqn.make, after its collection"""
    sim = O.LaneSim(coll["n"], max_steps=23, limit=ra.LIMIT_VISIBLE, seed_env=21, seed_actor=34)
    qs = O.MlpShape(5, H, 2)
    osim = O.DqnSim(sim, qs, O.mlp_init(qs, 77), coll["capacity"], key, minibatch, gamma=np.float32(0.99),
                    one_step_td=td)
    _, full = osim.collect(coll["horizon"], 0.3)
    assert not full
    return osim


def store_arrays(osim, coll):
    """every stored step of the oracle's lanes as [lane][step] arrays (the store is append-only and nothing was evicted)"""
    n, T = coll["n"], coll["horizon"]
    obs, nobs = np.zeros((n, T, 5)), np.zeros((n, T, 5))
    act, code, rew = np.zeros((n, T), dtype=np.int64), np.zeros((n, T), dtype=np.int64), np.zeros((n, T))
    for i in range(n):
        assert osim.lane_info(i)[0] == osim.lane_info(i)[2] == T
        for t in range(T):
            obs[i, t], act[i, t], rew[i, t], code[i, t], nobs[i, t] = osim.step_data(i, t)
    return dict(obs=obs, nobs=nobs, act=act, code=code, rew=rew)


def gather(store, lanes, starts, lens):
    """the minibatch of the drawn episodes, episode after episode, in float64: observations, actions, rewards, successor
    codes, successor observations (the stored Interrupt successor, or else the next stored step) and each sample's
    distance from its episode's end"""
    lens = lens.astype(np.int64)
    ep = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    lane, t = lanes.astype(np.int64)[ep], starts.astype(np.int64)[ep] + pos
    code = store["code"][lane, t]
    nxt = np.minimum(t + 1, store["obs"].shape[1] - 1)  # (the last stored step of a lane is never a Continue)
    succ = np.where((code == O.INTERRUPT)[:, None], store["nobs"][lane, t], store["obs"][lane, nxt])
    return dict(obs=store["obs"][lane, t], act=store["act"][lane, t], rew=store["rew"][lane, t], code=code, succ=succ,
                to_end=lens[ep] - 1 - pos)


def unflatten(p):
    p = np.asarray(p, dtype=np.float64)
    return (p[BLOCKS["W1"]].reshape(H, 5), p[BLOCKS["b1"]], p[BLOCKS["W2"]].reshape(2, H), p[BLOCKS["b2"]])


def q64(p, x):
    """Q_p(x) of the 5-128-2 relu network -> (values [rows][2], hidden outputs, relu')"""
    W1, b1, W2, b2 = unflatten(p)
    pre = x @ W1.T + b1
    h = np.maximum(pre, 0.0)
    return h @ W2.T + b2, h, pre > 0


def td_targets64(p, mb, gamma):
    """r + gamma max_a Q_p(s'), 0 beyond a Terminate"""
    v = np.concatenate([q64(p, mb["succ"][i:i + 65536])[0].max(axis=1) for i in range(0, len(mb["rew"]), 65536)])
    return mb["rew"] + gamma * np.where(mb["code"] == O.TERMINATE, 0.0, v)


def rtg_targets64(mb, gamma):
    """the discounted sum of rewards to the episode's end"""
    g = np.zeros(len(mb["rew"]))
    for d in range(int(mb["to_end"].max()) + 1):  # samples d steps before their episode's last: built from the end
        i = np.nonzero(mb["to_end"] == d)[0]
        g[i] = mb["rew"][i] + (gamma * g[i + 1] if d else 0.0)
    return g


def loss_grad64(p, mb, tgt):
    """loss and flat gradient of mean((Q_p(s)[a] - target)^2)"""
    B = len(tgt)
    W2 = unflatten(p)[2]
    g, loss = np.zeros(len(p)), 0.0
    for i in range(0, B, 65536):
        x, a, t = mb["obs"][i:i + 65536], mb["act"][i:i + 65536], tgt[i:i + 65536]
        z, h, mask = q64(p, x)
        rows = np.arange(len(a))
        d = z[rows, a] - t
        loss += (d * d).sum()
        dz = np.zeros_like(z)
        dz[rows, a] = 2.0 * d / B
        dh = (dz @ W2) * mask
        g += np.concatenate([(dh.T @ x).ravel(), dh.sum(axis=0), (h.T @ dz).T.ravel(), dz.sum(axis=0)])
    return loss / B, g


def chain64(p0, batches, td, gamma=GAMMA):
    p, losses = np.asarray(p0, dtype=np.float64).copy(), []
    for mb in batches:
        tgt = td_targets64(p, mb, gamma) if td else rtg_targets64(mb, gamma)
        loss, g = loss_grad64(p, mb, tgt)
        losses.append(loss)
        p = p - LR * g
    return p, np.array(losses)


def chain32(osim, draws):
    """the same chain in f32: the oracle's targets (at the chain's current parameters) and gradient, optim_ref's SGD"""
    state, losses = {}, []
    for lanes, starts, lens in draws:
        obs, act, tgt = osim.minibatch(lanes, starts, lens)
        g, loss = osim.grad(obs, act, tgt)
        losses.append(loss)
        osim.qparams[:] = sgd_step(osim.qparams, g, state, lr=LR)
    return osim.qparams.copy(), np.array(losses)


_references = {}


def reference(coll, minibatch, td, K, key=KEY, f32=True):
    """the K minibatches' conditions and the two chains, computed once per case on the CPU"""
    case = (coll["n"], minibatch, td, K, tuple(key))
    if case in _references:
        return _references[case]
    osim = oracle_agent(coll, minibatch, td, key)
    store = store_arrays(osim, coll)
    draws = [osim.sample()[:3] for _ in range(K)]
    batches = [gather(store, *d) for d in draws]
    obs_o, act_o, _ = osim.minibatch(*draws[0])  # the gather above against the oracle's
    assert np.array_equal(batches[0]["obs"], obs_o) and np.array_equal(batches[0]["act"], act_o)
    p0 = osim.qparams.copy()
    p64, losses64 = chain64(p0, batches, td)
    ref = dict(p0=p0, p64=p64, losses64=losses64, agent_pos=osim.agent_pos(), steps=[len(mb["rew"]) for mb in batches],
               batches=batches, e32=None)
    if f32:
        p32, ref["losses32"] = chain32(osim, draws)
        ref["e32"] = rel((p0 - p32.astype(np.float64)) / LR, (p0 - p64) / LR)
    _references[case] = ref
    return ref


def check_data(ref, tiles):
    for mb in ref["batches"]:
        B = len(mb["rew"])
        assert set(mb["act"]) == {0, 1}
        assert {O.TERMINATE, O.INTERRUPT, O.CONTINUE} <= set(mb["code"])
        assert B % 32 != 0 and (B + 31) // 32 == tiles, (B, tiles)


# ---------------------------------------------------------------- the device against it
def sgd(q):
    cfg = ra.optimizer_config_default(ra.OPTIMIZER_SGD)
    cfg.learning_rate, cfg.momentum, cfg.dampening, cfg.weight_decay, cfg.nesterov = LR, 0.0, 0.0, 0.0, 0
    return ra.Optimizer(q, cfg)


def run_case(engine, coll, minibatch, td, K, tiles, key=KEY, e32=None):
    ref = reference(coll, minibatch, td, K, key, f32=e32 is None)
    e32 = ref["e32"] if e32 is None else e32
    check_data(ref, tiles)
    dqn, _ = make(engine, n=coll["n"], capacity=coll["capacity"], minibatch=minibatch, td=td, opt_steps=K, opt=sgd,
                  key=key)
    dqn.collect(coll["horizon"])
    p0 = dqn.qnet.get_params()
    assert np.array_equal(p0, ref["p0"])
    st, losses_d = dqn.update(want_losses=True)
    assert st.opt_steps == K and st.last_minibatch_steps == ref["steps"][-1]
    assert dqn.agent_rng_pos() == ref["agent_pos"]  # the same episodes were drawn in every step
    lr, p0 = np.float64(LR), p0.astype(np.float64)
    g_d, g64 = (p0 - dqn.qnet.get_params().astype(np.float64)) / lr, (p0 - ref["p64"]) / lr
    bar = GRAD_RTOL + 2.0 * e32
    loss_err = np.abs(losses_d - ref["losses64"]) / ref["losses64"]
    per_block = {k: rel(g_d[s], g64[s]) for k, s in BLOCKS.items()}
    print("\nsteps %s: e32 %.3g, device vs f64 %.3g (bar %.3g); per block %s (bar %.3g)" % (
        ref["steps"], e32, rel(g_d, g64), bar, {k: "%.3g" % v for k, v in per_block.items()}, 50.0 * bar))
    print("losses device %s f64 %s rel. difference %s (bar 2e-5)" % (losses_d, ref["losses64"], loss_err))
    assert rel(g_d, g64) <= bar
    assert np.all(loss_err <= 2e-5)
    for k, s in BLOCKS.items():
        assert np.abs(g64[s]).max() > 0 and per_block[k] <= 50.0 * bar, k
    dqn.close()


TARGETS = pytest.mark.parametrize("td", [True, False], ids=["one-step-td", "reward-to-go"])


@TARGETS
def test_one_ragged_tile(engine, td):
    run_case(engine, SMALL, 20, td, 3, tiles=1, key=KEY_20)


@TARGETS
def test_five_tiles_on_two_workgroups(engine, td):
    run_case(engine, SMALL, 150, td, 3, tiles=5)


@TARGETS
def test_two_waves_walk_a_second_tile(engine, td):
    cus = engine.info()[2]
    run_case(engine, LARGE, 32 * 4 * cus + 40, td, 2, tiles=4 * cus + 2)


def test_td_flush_periods(engine):
    cus = engine.info()[2]
    # (the f64 chain of 524k steps takes seconds on the host and the f32 chain as long again: e32 is the third case's,
    # the same store and target at a sixteenth of the steps — 7.6e-8; computed once for this size on the CPU: 6.9e-8)
    e32 = reference(LARGE, 32 * 4 * cus + 40, True, 2)["e32"]
    run_case(engine, LARGE, 32 * 16 * 4 * cus + 1, True, 2, tiles=16 * 4 * cus + 1, e32=e32)
