"""Reference for the recurrent chains with a Linear tail, ChainConfig<GruConfig | LstmConfig, LinearConfig>
(modules/chain.rs:12-54): layers -> ReLU -> Linear(H, A), by EMBEDDING into the oracle's MLP-tail chain (test
infrastructure, not a test).

A linear-tail chain with parameters [rnn .., kernel, bias] and width H equals the MLP-tail chain with mlp_hidden = H and
parameters [rnn .., W1 = I_H, b1 = 0, W2 = kernel, b2 = bias] — under the kernels' arithmetic contract (acc = bias;
acc = fma(x_k, w_k, acc), k ascending) bit for bit: relu(top) is >= +0 and finite, fma(x, 0, acc) = acc and
fma(x, 1, +0) = x exactly, so the hidden layer reproduces relu(top) and its ReLU is the identity on it; the output layer
is then the same k-ascending chain.  Gradient and Fisher-vector product are the embedded chain's restricted to the blocks
rnn .., W2, b2, with the tangent zero on W1, b1 (both masks are [top > 0]).  tests/test_chain_linear_ref.py pins the
embedding against torch.nn.GRU / LSTM -> relu -> torch.nn.Linear.

The embedded vector always has recurrent bias vectors (the oracle's layout): zeros where the module has none."""
import collections
import functools

import numpy as np

import meta_lanes_ref as M
import meta_rollout_ref as R
import oracle as O
from oracle import stacked as S


def spec_of(cell, D, H, L, A):
    """the embedded chain's f64 spec (oracle/stacked.py)"""
    return S.Spec(S.GRU if cell == "gru" else S.LSTM, D, H, L, H, A)


def shape_of(cell, D, H, A, H2=None):
    """the embedded chain's shape for the C restatement (H2: another head width, for the init stream)"""
    return O.GruShape(D, H, H if H2 is None else H2, A, O.CELL_GRU if cell == "gru" else O.CELL_LSTM)


def blocks(cell, D, H, L, A, rnn_bias=True):
    """[(name, layer, shape, offset in the module's own flat vector, offset in the embedded vector)] in the module's flat
    order: per layer Wih, Whh (, bih, bhh), then kernel (the embedded W2), bias (b2)"""
    out, o = [], 0
    for name, l, shp, eo in spec_of(cell, D, H, L, A).slices()[0]:
        if name in ("W1", "b1") or (not rnn_bias and name in ("bih", "bhh")):
            continue
        out.append(({"W2": "kernel", "b2": "bias"}.get(name, name), l, shp, o, eo))
        o += int(np.prod(shp))
    return out


def num_params(cell, D, H, L, A, rnn_bias=True):
    G = 4 if cell == "lstm" else 3
    P = 0
    for l in range(L):
        K = D if l == 0 else H
        P += G * H * K + G * H * H + (2 * G * H if rnn_bias else 0)
    return P + A * H + A


def index(cell, D, H, L, A, rnn_bias=True):
    """where the module's entries sit in the embedded vector, in the module's flat order"""
    return np.concatenate([np.arange(eo, eo + int(np.prod(shp))) for _, _, shp, _, eo in blocks(cell, D, H, L, A, rnn_bias)])


def embed(cell, D, H, L, A, rnn_bias, params, tangent=False):
    """the module's flat vector -> the embedded chain's (same dtype); `tangent`: a direction — zero on W1, b1"""
    params = np.asarray(params)
    idx = index(cell, D, H, L, A, rnn_bias)
    assert params.shape == (len(idx),) == (num_params(cell, D, H, L, A, rnn_bias),)
    spec = spec_of(cell, D, H, L, A)
    full = np.zeros(spec.num_params(), dtype=params.dtype)
    full[idx] = params
    if not tangent:
        (o,) = [eo for name, _, _, eo in spec.slices()[0] if name == "W1"]
        full[o:o + H * H] = np.eye(H, dtype=params.dtype).reshape(-1)
    return full


def restrict(cell, D, H, L, A, rnn_bias, full):
    """a vector in the embedded layout (parameters, a gradient, a Fisher-vector product) -> the module's entries"""
    full = np.asarray(full)
    assert full.shape == (spec_of(cell, D, H, L, A).num_params(),)
    return full[index(cell, D, H, L, A, rnn_bias)]


def init(cell, D, H, L, A, rnn_bias, seed, inits=O.RNN_DEFAULT_INITS):
    """the module's initial parameters from the oracle's init stream: the MLP-tail chain with mlp_hidden = A draws, after
    its layers, W1 [A, H] and b1 [A] with fan_in = H + 1 — exactly Linear::new(H, A)'s kernel and bias, in stream order.
    `inits`: (input, hidden, bias, kernel, linear bias); without recurrent bias vectors the bias initializer must draw
    nothing (no tensors, no draws: seq/rnn/mod.rs:246-251)."""
    assert rnn_bias or inits[2][0] in ("Zeros", "Constant")
    p = O.stack_init_with(shape_of(cell, D, H, A, H2=A), L, seed, tuple(inits))[:num_params(cell, D, H, L, A, True)]
    if rnn_bias:
        return p
    drop = np.concatenate([np.arange(o, o + int(np.prod(shp))) for name, _, shp, o, _ in blocks(cell, D, H, L, A, True)
                           if name in ("bih", "bhh")])
    return p[np.setdiff1d(np.arange(len(p)), drop)]


# ---- rollouts on the meta-bandit lanes (D = 6, two arms): the cases tests/test_chain_linear_ref.py (margins, no device)
# and tests/test_gpu_chain_linear.py (the device against the reference) share
MetaCase = collections.namedtuple("MetaCase", "cell H L bias n T E arms offset seed")
META_CASES = [
    MetaCase("gru", 7, 1, True, 70, 10, 3, M.UNIFORM_BERNOULLI, 0, 301),
    MetaCase("lstm", 32, 2, True, 70, 10, 3, M.UNIFORM_BERNOULLI, 25, 311),  # lanes 25..94: the offset in a 2nd workgroup
    MetaCase("gru", 12, 1, False, 70, 10, 3, M.UNIFORM_BERNOULLI, 0, 321),
]


def meta_case_id(c):
    return "%s-%d-%d-%s-n%d-off%d" % (c.cell, c.H, c.L, "bias" if c.bias else "nobias", c.n, c.offset)


def meta_case_inits(c):
    """as tests/meta_rollout_ref.py: bias vectors that are not the default's zeros where the module has them"""
    inits = list(O.RNN_DEFAULT_INITS)
    if c.bias:
        inits[2] = R.BIAS_INIT
    return tuple(inits)


def meta_case_params(c):
    return init(c.cell, R.D, c.H, c.L, R.ARMS, c.bias, c.seed, meta_case_inits(c))


@functools.lru_cache(maxsize=None)
def meta_reference(c):
    """the closed-loop reference of the case (computed once per process; callers leave it unchanged)"""
    full = embed(c.cell, R.D, c.H, c.L, R.ARMS, c.bias, meta_case_params(c))
    return R.rollout(c.cell, c.H, c.L, c.H, True, c.n, c.T, c.E, c.arms, c.seed + 1, c.seed + 2, full,
                     lane_offset=c.offset)
