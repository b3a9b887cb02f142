"""numpy restatement of the first-order rules beside Adam, for the optimiser tests: SGD, RMSProp and AdamW in the
operation order of libtorch 1.12's C++ optimisers, which tch 0.8 binds and the reference's COptimizer configurations pass
their fields straight to (src/torch/optimizers/coptimizer.rs:76-86, 120-131, 195-204).  float32 arrays, one numpy
operation (one rounding) per written operation; scalars are formed in float64 and rounded to float32 once, as the library's
host side does.  State lives in a dict that starts empty.  Shared by tests/test_optimizers_cpu.py (which checks this file
against torch.optim on the CPU) and tests/test_gpu_optimizers.py (which checks the kernels against this file)."""
import math

import numpy as np

f32 = np.float32


def sgd_step(p, g, state, lr=1e-2, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """torch::optim::SGD::step; state: 'step', 'buf' (with momentum).  On the first step the buffer is a copy of the
    (decayed) gradient, without dampening."""
    p, g = np.asarray(p, dtype=f32), np.asarray(g, dtype=f32)
    k = state["step"] = state.get("step", 0) + 1
    if weight_decay != 0:
        g = g + f32(weight_decay) * p
    if momentum != 0:
        if k == 1:
            buf = g.copy()
        else:
            buf = state["buf"] * f32(momentum) + f32(1.0 - dampening) * g
        state["buf"] = buf
        g = g + f32(momentum) * buf if nesterov else buf
    return p + f32(-lr) * g


def rmsprop_step(p, g, state, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False):
    """torch::optim::RMSprop::step; state: 'step', 'sq', 'buf' (with momentum), 'ga' (centered)"""
    p, g = np.asarray(p, dtype=f32), np.asarray(g, dtype=f32)
    state["step"] = state.get("step", 0) + 1
    zeros = np.zeros_like(p)
    if weight_decay != 0:
        g = g + f32(weight_decay) * p
    sq = state.get("sq", zeros) * f32(alpha) + f32(1.0 - alpha) * g * g
    state["sq"] = sq
    if centered:
        ga = state.get("ga", zeros) * f32(alpha) + f32(1.0 - alpha) * g
        state["ga"] = ga
        avg = np.sqrt(sq + f32(-1.0) * ga * ga) + f32(eps)
    else:
        avg = np.sqrt(sq) + f32(eps)
    if momentum > 0:
        buf = state.get("buf", zeros) * f32(momentum) + g / avg
        state["buf"] = buf
        return p + f32(-lr) * buf
    return p + f32(-lr) * (g / avg)


def adamw_step(p, g, state, lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=0.0, eps=1e-8):
    """torch::optim::AdamW::step (amsgrad off); state: 'step', 'm', 'v'.  The decay multiplies the parameter first and
    never reaches the gradient."""
    p, g = np.asarray(p, dtype=f32), np.asarray(g, dtype=f32)
    k = state["step"] = state.get("step", 0) + 1
    zeros = np.zeros_like(p)
    p = p * f32(1.0 - lr * weight_decay)
    m = state.get("m", zeros) * f32(beta1) + f32(1.0 - beta1) * g
    v = state.get("v", zeros) * f32(beta2) + f32(1.0 - beta2) * g * g
    state["m"], state["v"] = m, v
    neg_step_size = -f32(lr / (1.0 - math.pow(beta1, k)))
    sqrt_bc2 = f32(math.sqrt(1.0 - math.pow(beta2, k)))
    denom = np.sqrt(v) / sqrt_bc2 + f32(eps)
    return p + (neg_step_size * m) / denom


RULES = {"sgd": sgd_step, "rmsprop": rmsprop_step, "adamw": adamw_step}
# the name of each state slot of the C ABI (rl_optimizer_state_read) in the dicts above
SLOTS = {"sgd": ("buf",), "rmsprop": ("sq", "buf", "ga"), "adamw": ("m", "v")}

# the configurations the tests share: (name, rule, keyword arguments of the rule)
CASES = [
    ("sgd_plain", "sgd", {}),
    ("sgd_momentum", "sgd", dict(momentum=0.9, dampening=0.1, weight_decay=1e-3)),
    ("sgd_nesterov", "sgd", dict(momentum=0.9, nesterov=True)),
    ("rmsprop_default", "rmsprop", {}),
    ("rmsprop_full", "rmsprop", dict(lr=1e-3, alpha=0.95, momentum=0.9, centered=True, weight_decay=1e-3)),
    ("adamw_decay", "adamw", dict(weight_decay=1e-2)),
]


def quadratic_gradient(x):
    """gradient of the reference's test problem 0.5 x'Mx + b'x (optimizers/mod.rs:140-169), minimum at [-1, 1]"""
    M = np.array([[1.0, -1.0], [-1.0, 2.0]], dtype=f32)
    b = np.array([2.0, -3.0], dtype=f32)
    return M @ np.asarray(x, dtype=f32) + b
