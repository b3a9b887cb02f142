"""The first-order rules beside Adam, without a device: the numpy restatement the GPU tests compare the kernels with
(tests/optim_ref.py) against torch.optim on the CPU and on the reference's own quadratic, and what the C ABI does before it
touches a device — the rules' default configurations and the configurations it rejects.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import optim_ref as R
import relearn_amd as ra


def _torch_optimizer(torch, rule, params, kw):
    if rule == "sgd":
        return torch.optim.SGD(params, lr=kw.get("lr", 1e-2), momentum=kw.get("momentum", 0.0),
                               dampening=kw.get("dampening", 0.0), weight_decay=kw.get("weight_decay", 0.0),
                               nesterov=kw.get("nesterov", False))
    if rule == "rmsprop":
        return torch.optim.RMSprop(params, lr=kw.get("lr", 1e-2), alpha=kw.get("alpha", 0.99), eps=kw.get("eps", 1e-8),
                                   weight_decay=kw.get("weight_decay", 0.0), momentum=kw.get("momentum", 0.0),
                                   centered=kw.get("centered", False))
    return torch.optim.AdamW(params, lr=kw.get("lr", 1e-3), betas=(kw.get("beta1", 0.9), kw.get("beta2", 0.999)),
                             eps=kw.get("eps", 1e-8), weight_decay=kw.get("weight_decay", 0.0))


@pytest.mark.parametrize("name,rule,kw", R.CASES, ids=[c[0] for c in R.CASES])
def test_restatement_matches_torch_optim(name, rule, kw):
    """897 parameters N(0, 0.2^2), 80 steps, gradients N(0, 1) x 10^randint(-6, 1).  Bound 1e-6 absolute on every step:
    four times the worst difference measured when the restatement was written (6.0e-8 ... 2.4e-7 over the six cases, with
    parameters moving by 0.03 - 1.4).  torch 2.x updates the first moment with lerp_ where libtorch 1.12 multiplies and
    adds, so the last place can differ; a wrong dampening, a dampened first step, coupled instead of decoupled decay or a
    misplaced eps are orders of magnitude above the bound."""
    import torch
    rng = np.random.default_rng(11)
    p0 = (rng.standard_normal(897) * 0.2).astype(np.float32)
    tp = torch.nn.Parameter(torch.tensor(p0.copy()))
    topt = _torch_optimizer(torch, rule, [tp], kw)
    p, state, worst = p0.copy(), {}, 0.0
    for _ in range(80):
        g = (rng.standard_normal(897) * 10.0 ** rng.integers(-6, 1)).astype(np.float32)
        p = R.RULES[rule](p, g, state, **kw)
        tp.grad = torch.tensor(g.copy())
        topt.step()
        worst = max(worst, float(np.abs(p - tp.detach().numpy()).max()))
    moved = float(np.abs(p - p0).max())
    print("%s: worst |restatement - torch| %.3g, parameters moved by %.3g" % (name, worst, moved))
    assert p.dtype == np.float32 and moved > 0.01
    assert worst <= 1e-6


@pytest.mark.parametrize("rule", ["sgd", "rmsprop"])
def test_restatement_minimises_the_reference_quadratic(rule):
    """the reference's own check of its optimisers (optimizers/mod.rs:140-169, coptimizer.rs:214-246): default
    configuration at learning rate 0.1, 500 steps from 0, within 1e-3 of [-1, 1]"""
    x, state = np.zeros(2, dtype=np.float32), {}
    for _ in range(500):
        x = R.RULES[rule](x, R.quadratic_gradient(x), state, lr=0.1)
    err = float(np.linalg.norm(x.astype(np.float64) - np.array([-1.0, 1.0])))
    print("%s: |x - [-1, 1]| = %.3g" % (rule, err))
    assert err < 1e-3


def _fields(c):
    return {k: getattr(c, k) for k, _ in c._fields_}


def test_default_configurations_are_the_reference_defaults():
    """SgdConfig / RmsPropConfig / AdamConfig / AdamWConfig::default (coptimizer.rs:64-74, 107-118, 147-156, 184-193);
    eps is libtorch's 1e-8 where the reference has no such field"""
    zero = dict(nesterov=0, centered=0, reserved=0, weight_decay=0.0, beta1=0.0, beta2=0.0, momentum=0.0, dampening=0.0,
                alpha=0.0, eps=1e-8)
    assert _fields(ra.optimizer_config_default(ra.OPTIMIZER_SGD)) == dict(zero, kind=ra.OPTIMIZER_SGD, learning_rate=1e-2)
    assert _fields(ra.optimizer_config_default(ra.OPTIMIZER_RMSPROP)) == dict(
        zero, kind=ra.OPTIMIZER_RMSPROP, learning_rate=1e-2, alpha=0.99)
    for kind in (ra.OPTIMIZER_ADAM, ra.OPTIMIZER_ADAMW):
        assert _fields(ra.optimizer_config_default(kind)) == dict(zero, kind=kind, learning_rate=1e-3, beta1=0.9,
                                                                   beta2=0.999)
    a, o = ra.adam_config_default(), ra.optimizer_config_default(ra.OPTIMIZER_ADAM)
    assert all(getattr(a, k) == getattr(o, k) for k, _ in a._fields_)
    assert (ra.OPTIMIZER_ADAM, ra.OPTIMIZER_ADAMW, ra.OPTIMIZER_SGD, ra.OPTIMIZER_RMSPROP) == (0, 1, 2, 3)
    with pytest.raises(ra.RelearnError) as e:
        ra.optimizer_config_default(4)
    assert e.value.code == ra.ERR_INVALID_ARGUMENT and "kind" in str(e.value)


REJECTED = [
    (ra.OPTIMIZER_SGD, dict(learning_rate=-1e-2), "learning_rate"),
    (ra.OPTIMIZER_SGD, dict(momentum=-0.5), "momentum"),
    (ra.OPTIMIZER_SGD, dict(weight_decay=-1e-3), "weight_decay"),
    (ra.OPTIMIZER_SGD, dict(nesterov=1), "nesterov"),                               # momentum 0
    (ra.OPTIMIZER_SGD, dict(nesterov=1, momentum=0.9, dampening=0.1), "nesterov"),  # dampening != 0
    (ra.OPTIMIZER_RMSPROP, dict(learning_rate=-1.0), "learning_rate"),
    (ra.OPTIMIZER_RMSPROP, dict(momentum=-0.1), "momentum"),
    (ra.OPTIMIZER_RMSPROP, dict(weight_decay=-1.0), "weight_decay"),
    (ra.OPTIMIZER_RMSPROP, dict(eps=-1e-8), "eps"),
    (ra.OPTIMIZER_RMSPROP, dict(alpha=-0.5), "alpha"),
    (ra.OPTIMIZER_ADAM, dict(learning_rate=-1e-3), "learning_rate"),
    (ra.OPTIMIZER_ADAM, dict(eps=-1.0), "eps"),
    (ra.OPTIMIZER_ADAM, dict(beta1=1.0), "beta1"),
    (ra.OPTIMIZER_ADAM, dict(beta2=-0.1), "beta2"),
    (ra.OPTIMIZER_ADAMW, dict(weight_decay=-1e-2), "weight_decay"),
    (ra.OPTIMIZER_ADAMW, dict(beta1=-0.1), "beta1"),
    (ra.OPTIMIZER_ADAMW, dict(beta2=1.0), "beta2"),
    (ra.OPTIMIZER_ADAMW, dict(kind=7), "kind"),
]


@pytest.mark.parametrize("kind,change,field", REJECTED, ids=["%d-%s" % (k, "-".join(sorted(c))) for k, c, _ in REJECTED])
def test_rejected_configurations(kind, change, field):
    """what libtorch's option checks reject is RL_ERR_INVALID_ARGUMENT with a message that names the field — decided before
    the module is looked at, so no device is needed: the module handle here is NULL, and only a configuration that passes
    the checks gets as far as the NULL-argument message"""
    cfg = ra.optimizer_config_default(kind)
    for k, v in change.items():
        setattr(cfg, k, v)
    out = C.c_void_p()
    assert ra.lib().rl_optimizer_create(None, C.byref(cfg), C.byref(out)) == ra.ERR_INVALID_ARGUMENT
    assert field in ra.lib().rl_last_error(None).decode()
    assert not out.value


@pytest.mark.parametrize("kind", [ra.OPTIMIZER_ADAM, ra.OPTIMIZER_ADAMW, ra.OPTIMIZER_SGD, ra.OPTIMIZER_RMSPROP])
def test_accepted_configurations_reach_the_module_check(kind):
    cfg = ra.optimizer_config_default(kind)
    if kind == ra.OPTIMIZER_SGD:
        cfg.momentum, cfg.nesterov = 0.9, 1
    out = C.c_void_p()
    assert ra.lib().rl_optimizer_create(None, C.byref(cfg), C.byref(out)) == ra.ERR_INVALID_ARGUMENT
    assert ra.lib().rl_last_error(None).decode() == "NULL argument"
