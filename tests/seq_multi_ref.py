"""Reference for the recurrent chains of MORE THAN TWO outputs (rl_rnn_chain_create, ra.RnnChain; test infrastructure,
not a test): ChainConfig<GruConfig | LstmConfig, MlpConfig | LinearConfig> over IndexSpace::new(3..8).

The oracle is already general in the action count — oracle/stacked.py (f64 forward, backward, jvp, policy_fvp) and the C
forward (oracle.stack_seq_forward, oracle/stack_impl.inc) — and tests/test_seq_multi_ref.py pins it at A = 3 and 8 against
torch.  What this file adds:
  layouts    a module's flat vector <-> the oracle's (recurrent bias vectors always present there: zeros where the module
             has none; a Linear tail by tests/chain_linear_ref.py's embedding, W1 = I, b1 = 0)
  policy     d loss / d logits of the surrogate at ratio 1 and of the clipped PPO surrogate, loss and KL, in f64
  rollouts   the closed loop on meta-bandit lanes of k = 2..4 arms (D = k + 4), built as tests/meta_rollout_ref.py is for
             two arms: logits from the teacher-forced C forward over the prefix, the action from oracle_log_softmax_f32 /
             oracle_categorical_sample_u at word period * T + t of the lane's actor stream, the env from
             tests/meta_lanes_ref.py; `margin` is the smallest distance of a uniform from ANY cumulative boundary
and the cases the CPU test (margins) and the GPU test (the device against this) share."""
import collections
import ctypes as C
import functools

import numpy as np

import chain_linear_ref as CL
import meta_lanes_ref as M
import oracle as O
from oracle import stacked as S

L = O.lib()
Net = collections.namedtuple("Net", "cell D H L H2 bias A")  # H2 = 0: a Linear tail
PLANES = ("obs", "action", "reward", "flag", "term_obs")
BIAS_INIT = ("Uniform", "FanAvg", 0.0)  # recurrent bias vectors that are not the default's zeros


def net_id(c):
    return "%s-D%d-H%d-L%d-%s-%s-A%d" % (c.cell, c.D, c.H, c.L, "linear" if c.H2 == 0 else "mlp%d" % c.H2,
                                          "bias" if c.bias else "nobias", c.A)


def spec_of(c):
    """the f64 spec of the chain the oracle runs (a Linear tail embedded at mlp_hidden = H)"""
    return S.Spec(S.GRU if c.cell == "gru" else S.LSTM, c.D, c.H, c.L, c.H2 if c.H2 else c.H, c.A)


def shape_of(c, H2=None):
    return O.GruShape(c.D, c.H, (c.H2 if c.H2 else c.H) if H2 is None else H2, c.A,
                      O.CELL_GRU if c.cell == "gru" else O.CELL_LSTM)


def blocks(c):
    """[(name, layer, shape, offset in the module's flat vector, offset in the oracle's)] in the module's flat order"""
    if c.H2 == 0:
        return CL.blocks(c.cell, c.D, c.H, c.L, c.A, c.bias)
    out, o = [], 0
    for name, l, shp, eo in spec_of(c).slices()[0]:
        if not c.bias and name in ("bih", "bhh"):
            continue
        out.append((name, l, shp, o, eo))
        o += int(np.prod(shp))
    return out


def index(c):
    return np.concatenate([np.arange(eo, eo + int(np.prod(shp))) for _, _, shp, _, eo in blocks(c)])


def num_params(c):
    return len(index(c))


def to_oracle(c, params, tangent=False):
    """the module's flat vector -> the oracle's layout (same dtype); `tangent`: a direction (zero on an embedded W1)"""
    params = np.asarray(params)
    idx = index(c)
    assert params.shape == (len(idx),)
    spec = spec_of(c)
    full = np.zeros(spec.num_params(), dtype=params.dtype)
    full[idx] = params
    if c.H2 == 0 and not tangent:
        (o,) = [eo for name, _, _, eo in spec.slices()[0] if name == "W1"]
        full[o:o + c.H * c.H] = np.eye(c.H, dtype=params.dtype).reshape(-1)
    return full


def restrict(c, full):
    full = np.asarray(full)
    assert full.shape == (spec_of(c).num_params(),)
    return full[index(c)]


def init(c, seed, inits=O.RNN_DEFAULT_INITS):
    """the module's initial parameters from the oracle's init stream, the head drawn at its real A (a Linear tail: the
    MLP-tail chain with mlp_hidden = A draws Linear::new(H, A)'s kernel and bias after its layers)"""
    if c.H2 == 0:
        return CL.init(c.cell, c.D, c.H, c.L, c.A, c.bias, seed, inits)
    assert c.bias or inits[2][0] in ("Zeros", "Constant")
    with_bias = c._replace(bias=True)
    p = O.stack_init_with(shape_of(c), c.L, seed, tuple(inits))
    assert p.shape == (num_params(with_bias),)
    if c.bias:
        return p
    keep = np.concatenate([np.arange(o, o + int(np.prod(shp))) for name, _, shp, o, _ in blocks(with_bias)
                           if name not in ("bih", "bhh")])
    return p[keep]


# ---------------------------------------------------------------- the per-sample policy terms in f64
def log_softmax(z):
    z = z - z.max(axis=0)
    return z - np.log(np.exp(z).sum(axis=0))


def one_hot(action, A):
    a = np.asarray(action).astype(np.int64)
    return (np.arange(A).reshape((-1,) + (1,) * a.ndim) == a[None]).astype(np.float64)


def surrogate_dlogits(logits, action, adv):
    """loss = -mean(ratio adv) at ratio 1: d loss / d logits [A][T][n], loss, mean entropy"""
    lp = log_softmax(np.asarray(logits, dtype=np.float64))
    adv = np.asarray(adv, dtype=np.float64)
    pr = np.exp(lp)
    dz = -(adv / adv.size)[None] * (one_hot(action, lp.shape[0]) - pr)
    return dz, -adv.mean(), -(pr * lp).sum(0).mean()


def loss_and_kl(logits, logits0, action, adv):
    """(-mean(ratio adv), mean KL(pi_0 || pi)) of `logits` against the policy of `logits0`"""
    lp, lp0 = log_softmax(np.asarray(logits, dtype=np.float64)), log_softmax(np.asarray(logits0, dtype=np.float64))
    a = np.asarray(action).astype(np.int64)[None]
    ratio = np.exp(np.take_along_axis(lp, a, 0)[0] - np.take_along_axis(lp0, a, 0)[0])
    return -(ratio * np.asarray(adv, dtype=np.float64)).mean(), (np.exp(lp0) * (lp0 - lp)).sum(0).mean()


def ppo_dlogits(logits, logits0, action, adv, clip):
    """Ppo::update's loss -mean(min(r A, clamp(r, 1 - clip, 1 + clip) A)) (policies/ppo.rs:124-137) and its gradient as
    torch autograd gives it — minimum() splits a tie between its arguments, clamp() passes the gradient inside
    [lo, hi], bounds included: d loss / d logits, loss, the ratios"""
    lo, hi = 1.0 - clip, 1.0 + clip
    lp, lp0 = log_softmax(np.asarray(logits, dtype=np.float64)), log_softmax(np.asarray(logits0, dtype=np.float64))
    adv = np.asarray(adv, dtype=np.float64)
    a = np.asarray(action).astype(np.int64)[None]
    ratio = np.exp(np.take_along_axis(lp, a, 0)[0] - np.take_along_axis(lp0, a, 0)[0])
    u1, u2 = ratio * adv, np.clip(ratio, lo, hi) * adv
    through_clamp = np.where((ratio >= lo) & (ratio <= hi), adv, 0.0)
    w = np.where(u1 < u2, adv, np.where(u1 == u2, 0.5 * adv + 0.5 * through_clamp, through_clamp))
    c = -(w * ratio) / adv.size
    return c[None] * (one_hot(action, lp.shape[0]) - np.exp(lp)), -np.minimum(u1, u2).mean(), ratio


# ---------------------------------------------------------------- histories written by the host
def history(c, n, T, seed):
    """planes of a host-written trajectory: Terminate and Interrupt inside and at the horizon, every action index"""
    rng = np.random.default_rng(seed)
    h = {"obs": rng.normal(size=(c.D, T + 1, n)).astype(np.float32),
         "flag": rng.choice(np.array([0, 0, 0, 0, 1, 2], dtype=np.uint8), size=(T, n)),
         "term_obs": rng.normal(size=(c.D, T, n)).astype(np.float32),
         "action": rng.integers(0, c.A, size=(T, n)).astype(np.uint8),
         "reward": rng.normal(size=(T, n)).astype(np.float32),
         "adv": rng.normal(size=(T, n)).astype(np.float32),
         "rtg": rng.normal(size=(T, n)).astype(np.float32)}
    lane = np.arange(n)
    h["action"][lane % T, lane] = (lane % c.A).astype(np.uint8)  # (n >= A, or T >= A at n = 1: below)
    if n == 1:
        h["action"][:, 0] = (np.arange(T) % c.A).astype(np.uint8)
    h["flag"][T - 1, 0] = 2          # an Interrupt at the horizon
    h["flag"][T - 1, n - 1] = 1 if n > 1 else 2
    h["flag"][T // 2, 0] = 2         # and inside
    h["flag"][1, n // 2] = 1
    h["flag"][0, 0] = 0              # lane 0's step 1 continues step 0: the hidden-side weights see a non-zero state at n = 1
    return h


# ---------------------------------------------------------------- closed-loop rollouts on the meta-bandit lanes
MetaCase = collections.namedtuple("MetaCase", "net n T E arms offset seed")
# (D = k + 4, A = k); seed: the module's init seed, seed_env = seed + 1, seed_actor = seed + 2.  The seeds are chosen on
# the CPU (tests/test_seq_multi_ref.py) so that every sampled action is decided by more than MIN_MARGIN.
META_CASES = [
    MetaCase(Net("gru", 7, 12, 1, 0, True, 3), 70, 9, 3, M.UNIFORM_BERNOULLI, 0, 401),
    MetaCase(Net("lstm", 7, 9, 2, 6, True, 3), 70, 9, 3, M.ONE_HOT, 25, 411),   # lanes 25..94: the offset in a 2nd workgroup
    MetaCase(Net("gru", 8, 10, 1, 7, False, 4), 70, 9, 3, M.ONE_HOT, 0, 421),
    MetaCase(Net("lstm", 8, 8, 1, 0, True, 4), 70, 9, 2, M.UNIFORM_BERNOULLI, 0, 431),
]
PERIODS = 2
MIN_MARGIN = 1e-5
Reference = collections.namedtuple("Reference", "periods margin observe")


def meta_case_id(m):
    return "%s-n%d-T%d-E%d-%s-off%d" % (net_id(m.net), m.n, m.T, m.E, m.arms, m.offset)


def meta_case_params(m):
    inits = list(O.RNN_DEFAULT_INITS)
    if m.net.bias:
        inits[2] = BIAS_INIT
    return init(m.net, m.seed, tuple(inits))


def meta_rollout(net, n, T, E, distribution, seed_env, seed_actor, params, lane_offset=0, periods=PERIODS):
    k = net.A
    assert net.D == k + 4
    shape, full = shape_of(net), to_oracle(net, np.ascontiguousarray(params, dtype=np.float32))
    lanes = M.MetaLanes(n, k, E, distribution, lane_offset=lane_offset, seed_env=seed_env)
    rngs = []
    for i in range(n):
        r = O.Prng()
        L.oracle_prng_seed_from_u64(C.byref(r), seed_actor)
        L.oracle_prng_set_stream(C.byref(r), lane_offset + i)
        rngs.append(r)
    lp = np.zeros(k, np.float32)
    margin = np.inf
    out = []
    for period in range(periods):
        obs = np.zeros((net.D, T + 1, n), np.float32)
        term = np.zeros((net.D, T, n), np.float32)
        action = np.zeros((T, n), np.uint8)
        reward = np.zeros((T, n), np.float32)
        flag = np.zeros((T, n), np.uint8)
        obs[:, 0] = lanes.observe()
        for t in range(T):
            prefix = {"obs": np.ascontiguousarray(obs[:, :t + 2]), "flag": np.ascontiguousarray(flag[:t + 1]),
                      "term_obs": np.ascontiguousarray(term[:, :t + 1])}
            z = O.stack_seq_forward(shape, net.L, full, prefix, want_succ=False)[0][:, t]  # [k][n]
            for i in range(n):
                L.oracle_prng_set_word_pos(C.byref(rngs[i]), period * T + t)
                w = L.oracle_prng_next_u32(C.byref(rngs[i]))
                u = np.float32(w >> 8) * np.float32(1.0 / (1 << 24))
                zi = np.ascontiguousarray(z[:, i])
                L.oracle_log_softmax_f32(O.f32p(zi), k, O.f32p(lp), 0)
                action[t, i] = L.oracle_categorical_sample_u(O.f32p(lp), k, C.c_float(u), 0)
                cum = np.cumsum(np.exp(log_softmax(zi.astype(np.float64))))[:-1]
                margin = min(margin, np.abs(np.float64(u) - cum).min())
            reward[t], flag[t], obs[:, t + 1], term[:, t] = lanes.step(action[t])
        out.append({"obs": obs, "action": action, "reward": reward, "flag": flag, "term_obs": term})
    return Reference(out, float(margin), lanes.observe())


@functools.lru_cache(maxsize=None)
def meta_reference(m):
    """the case's closed-loop reference (computed once per process; callers leave it unchanged)"""
    return meta_rollout(m.net, m.n, m.T, m.E, m.arms, m.seed + 1, m.seed + 2, meta_case_params(m), lane_offset=m.offset)
