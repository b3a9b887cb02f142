"""Recurrent chains with a Linear tail — ChainConfig<GruConfig | LstmConfig, LinearConfig> (modules/chain.rs:12-54), the
model of the reference's rl2-bandits experiment (rl2-bandits.rs:349,379-394) — on the lane-per-thread kernels'
linear-tail instantiations (relearn_amd/csrc/kernels_seq_stack.hip), against the oracle by embedding
(tests/chain_linear_ref.py: the MLP-tail chain with mlp_hidden = H, W1 = I, b1 = 0; pinned on the CPU by
tests/test_chain_linear_ref.py): initialisation and forward bit for bit, gradients and Fisher-vector products against the
restricted f64 results, rollouts on both lane families, every update entry point, actor documents, refusals, and the
experiment's agent learning to use its memory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cbor_ref
import chain_linear_ref as CL
import meta_lanes_ref as M
import meta_rollout_ref as R
import oracle as O
import relearn_amd as ra
from oracle import stacked as S
from test_gpu_stacked import GRAD_RTOL, rel_err, synthetic_history

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (cell, in_dim, H, L, A, rnn_bias): the smallest widths at which each loop of the head can go wrong — dot_rows takes 4 k
# per trip, the forward deals 4 units x 8 waves, the backward's tdot 8 k x 8 waves = 64 per pass
SHAPES = [
    ("gru", 3, 1, 1, 1, True),     # H below every block size
    ("gru", 6, 7, 1, 2, True),     # the meta lanes' input width; H off the 4- and 8-blocks
    ("lstm", 8, 33, 2, 1, True),   # one past the 32-unit pass, stacked, widest input
    ("lstm", 5, 70, 1, 2, True),   # second pass of the backward's 64-wide k loop, with a tail
    ("gru", 7, 12, 3, 2, True),    # three layers
    ("gru", 5, 128, 1, 2, True),   # the experiment's width: with an MLP tail the tile kernels' shape, here the lane kernels'
    ("gru", 6, 7, 1, 2, False),    # layers without bias vectors
    ("lstm", 5, 36, 2, 1, False),
]
EXPERIMENT_INITS = (("Uniform", "FanAvg", 0.0), ("Orthogonal", "FanAvg", 0.0), ("Zeros", "FanAvg", 0.0),
                    ("Uniform", "FanAvg", 0.0), ("Uniform", "FanAvg", 0.0))  # rl2-bandits.rs:379-394, LinearConfig::default


def shape_id(s):
    return "%s-%d-%d-%d-%d-%s" % (s[0], s[1], s[2], s[3], s[4], "bias" if s[5] else "nobias")


def module(engine, cell, D, H, NL, A, bias, seed=None):
    m = (ra.GruLinear if cell == "gru" else ra.LstmLinear)(engine, D, A, H, num_layers=NL, rnn_bias=bias)
    if seed is not None:
        m.init(seed)
    return m


def code_of(fn):
    with pytest.raises(ra.RelearnError) as e:
        fn()
    return e.value.code


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_parameters_and_initialisation(engine, shape):
    """P; rl_mlp_init: the layers' draws are the embedded shape's chain's, the Linear's continue the stream as
    Linear::new(H, A) (fan_in = H + 1); rl_rnn_mlp_init_with with the experiment's initializers and with others"""
    cell, D, H, NL, A, bias = shape
    m = module(engine, *shape)
    G = 4 if cell == "lstm" else 3
    P = sum(G * H * (D if l == 0 else H) + G * H * H + (2 * G * H if bias else 0) for l in range(NL)) + A * H + A
    assert m.P == P == CL.num_params(cell, D, H, NL, A, bias)
    m.init(31)
    p = m.get_params()
    emb = O.stack_init(CL.shape_of(cell, D, H, A), NL, 31)
    bl = CL.blocks(cell, D, H, NL, A, bias)
    for name, l, shp, o, eo in bl[:-2]:  # restrict(stack_init(embedded shape)) on the recurrent blocks
        assert np.array_equal(p[o:o + int(np.prod(shp))], emb[eo:eo + int(np.prod(shp))]), (name, l)
    assert np.array_equal(p, CL.init(cell, D, H, NL, A, bias, 31))
    assert np.abs(p[bl[-2][3]:]).min() > 0  # kernel and bias are drawn
    none_if = lambda x: x if bias else None
    m.init_with(33, EXPERIMENT_INITS[0], EXPERIMENT_INITS[1], none_if(EXPERIMENT_INITS[2]), *EXPERIMENT_INITS[3:])
    assert np.array_equal(m.get_params(), CL.init(cell, D, H, NL, A, bias, 33, EXPERIMENT_INITS))
    other = (("Normal", "FanIn", 0.0), ("Uniform", "Constant", 0.25), ("Constant", "FanAvg", 0.5),
             ("Orthogonal", "FanAvg", 0.0), ("Normal", "FanOut", 0.0))
    if bias:
        other = other[:2] + (("Normal", "FanOut", 0.0),) + other[3:]
    m.init_with(7, other[0], other[1], none_if(other[2]), other[3], other[4])
    assert np.array_equal(m.get_params(), CL.init(cell, D, H, NL, A, bias, 7, other))
    assert code_of(lambda: m.init_with(7, bias=None if bias else ("Zeros", "FanAvg", 0.0))) == ra.ERR_INVALID_ARGUMENT
    assert code_of(lambda: m.init_with(7, bias=none_if(("Zeros", "FanAvg", 0.0)), linear_bias=None)) == ra.ERR_UNSUPPORTED
    q = np.random.default_rng(2).normal(size=m.P).astype(np.float32)
    m.set_params(q)
    assert np.array_equal(m.get_params(), q)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("n", [33, 70, 128])
def test_forward_is_bit_exact(engine, shape, n):
    """module outputs and successor outputs (Interrupt and horizon cuts) against the C restatement of the embedded
    module: identical bits; values, advantages and returns through the recurrent critic path"""
    cell, D, H, NL, A, bias = shape
    m = module(engine, *shape, seed=31)
    traj, want = synthetic_history(engine, n, 11, D, 5)
    out_d, succ_d = m.seq_forward(traj)
    full = CL.embed(cell, D, H, NL, A, bias, m.get_params())
    out_o, succ_o = O.stack_seq_forward(CL.shape_of(cell, D, H, A), NL, full, want)
    assert np.array_equal(out_d, out_o) and np.array_equal(succ_d, succ_o)
    assert np.abs(out_o).max() > 0 and np.count_nonzero(succ_o) > 0 and np.count_nonzero(succ_d) > 0
    if A == 1:
        ra.gae(traj, m, 0.95, 0.9)
        adv_o, rtg_o = O.seq_gae(out_o[0], succ_o[0], want, np.float32(0.95), np.float32(0.9))
        assert np.array_equal(traj.read(ra.TRAJ_ADVANTAGES), adv_o) and np.array_equal(traj.read(ra.TRAJ_RETURNS), rtg_o)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_gradients_against_f64(engine, shape):
    """surrogate / critic gradient through time and (policies) a Fisher-vector product against the embedded chain's f64
    results restricted to the module's blocks (tangent zero on W1, b1); every block, kernel and bias included, receives
    gradient"""
    cell, D, H, NL, A, bias = shape
    m = module(engine, *shape, seed=41)
    spec = CL.spec_of(cell, D, H, NL, A)
    traj, want = synthetic_history(engine, 96, 9, D, 6)
    p = m.get_params()
    full = CL.embed(cell, D, H, NL, A, bias, p)
    rs = lambda v: CL.restrict(cell, D, H, NL, A, bias, v)
    B = want["action"].size
    if A == 2:
        g_d, loss_d, ent_d = ra.policy_gradient(m, traj)
        logits, _, _ = S.forward(spec, full, want, want_succ=False)
        z = logits - logits.max(0)
        pr = np.exp(z - np.log(np.exp(z).sum(0)))
        a = want["action"].astype(np.int64)
        ind = np.stack([a == 0, a == 1]).astype(np.float64)
        g64 = rs(S.backward(spec, full, want, -(want["adv"].astype(np.float64) / B) * (ind - pr)))
        print("gradient rel err %.3g" % rel_err(g_d, g64))
        assert g_d.shape == g64.shape and rel_err(g_d, g64) < GRAD_RTOL, rel_err(g_d, g64)
        assert abs(loss_d + want["adv"].astype(np.float64).mean()) < 1e-6  # -mean(ratio * A) at ratio 1
        v = np.random.default_rng(3).normal(size=m.P).astype(np.float32)
        h_d = ra.policy_fvp(m, traj, v, 1e-5)
        h64 = rs(S.policy_fvp(spec, full, CL.embed(cell, D, H, NL, A, bias, v, tangent=True), want, 1e-5))
        print("fvp rel err %.3g" % rel_err(h_d, h64))
        assert rel_err(h_d, h64) < 2e-5, rel_err(h_d, h64)
    else:
        g_d, loss_d = ra.critic_gradient(m, traj)
        vv, _, _ = S.forward(spec, full, want, want_succ=False)
        d = vv - want["rtg"].astype(np.float64)[None]
        g64 = rs(S.backward(spec, full, want, 2.0 * d / B))
        print("gradient rel err %.3g" % rel_err(g_d, g64))
        assert rel_err(g_d, g64) < GRAD_RTOL, rel_err(g_d, g64)
        assert abs(loss_d - (d * d).mean()) <= 1e-5 * (d * d).mean()
        st, losses = ra.critic_update(m, ra.Adam(m), traj, 3, want_losses=True)
        assert losses[-1] < losses[0] and not np.array_equal(m.get_params(), p)
    for name, l, shp, o, _ in CL.blocks(cell, D, H, NL, A, bias):
        blk = slice(o, o + int(np.prod(shp)))
        assert np.abs(g_d[blk]).max() > 0, (name, l)
        assert rel_err(g_d[blk], g64[blk]) < 100 * GRAD_RTOL, (name, l, rel_err(g_d[blk], g64[blk]))


def meta_run(engine, case, variants):
    """one env, one policy, one trajectory, one collection per entry of `variants`"""
    try:
        env = ra.MetaBanditEnv(engine, case.n, R.ARMS, case.E, case.arms, lane_offset=case.offset,
                               seed_env=case.seed + 1, seed_actor=case.seed + 2)
        assert (env.D, env.A) == (R.D, R.ARMS)
        pol = module(engine, case.cell, R.D, case.H, case.L, R.ARMS, case.bias)
        if case.bias:
            pol.init_with(case.seed, bias=R.BIAS_INIT)
        else:
            pol.init(case.seed)
        assert np.array_equal(pol.get_params(), CL.meta_case_params(case))
        traj = ra.Trajectory(engine, case.n, case.T, R.D)
        planes = []
        for variant in variants:
            engine.set_kernel_variant(variant)
            ra.rollout(env, pol, traj)
            planes.append(traj.read_all())
        engine.set_kernel_variant(0)
        logits = pol.seq_forward(traj, want_succ=False)[0]
        observe = env.observe()
        driven = env.step(R.driven_actions(case.n))
    finally:
        engine.set_kernel_variant(0)
    return planes, logits, observe, driven


@pytest.mark.parametrize("case", CL.META_CASES, ids=CL.meta_case_id)
def test_rollout_on_meta_bandit_lanes(engine, case):
    """all steps in one launch (kernel variant 0), the launch sequence per step (variant 1), and one then the other,
    against the closed-loop reference of the embedded module: whole planes, two collections in a row, no sample excused
    (tests/test_chain_linear_ref.py holds every sampled action's margin above 1e-5)"""
    ref = CL.meta_reference(case)
    full = CL.embed(case.cell, R.D, case.H, case.L, R.ARMS, case.bias, CL.meta_case_params(case))
    z = O.stack_seq_forward(CL.shape_of(case.cell, R.D, case.H, R.ARMS), case.L, full, ref.periods[-1], want_succ=False)[0]
    runs = {}
    for what, variants in (("one launch", (0, 0)), ("per step", (1, 1)), ("one launch, then per step", (0, 1))):
        planes, logits, observe, driven = runs[what] = meta_run(engine, case, variants)
        for p in range(R.PERIODS):
            for key in ("action", "reward", "flag", "obs"):
                assert np.array_equal(planes[p][key], ref.periods[p][key]), (what, p, key)
            cut = ref.periods[p]["flag"] == M.INTERRUPT
            assert cut.any() and np.array_equal(planes[p]["term_obs"][:, cut], ref.periods[p]["term_obs"][:, cut]), (what, p)
        assert np.array_equal(logits, z), what
        assert np.array_equal(observe, ref.observe), what
        for got, want in zip(driven[:3], ref.driven[:3]):
            assert np.array_equal(got, want), what
    for p in range(R.PERIODS):  # the two against each other: every term_obs entry included
        for key in R.PLANES:
            assert np.array_equal(runs["one launch"][0][p][key], runs["per step"][0][p][key]), (p, key)


def test_rollout_and_updates_on_chain_lanes(engine):
    """the index-env lanes (Chain) at the experiment's width, 5 -> GRU(128) -> Linear: env side against the oracle's lanes,
    logits against the embedded forward, then one update of each kind — TRPO, PPO, REINFORCE, critic fitting"""
    n, T, H = 64, 12, 128
    env = ra.ChainEnv(engine, n, max_steps=9, seed_env=3, seed_actor=4)
    sim = O.ChainLaneSim(n, max_steps=9, seed_env=3, seed_actor=4)
    pol, cri = module(engine, "gru", 5, H, 1, 2, True, 13), module(engine, "gru", 5, H, 1, 1, True, 14)
    traj = ra.Trajectory(engine, n, T, 5)
    ra.rollout(env, pol, traj)
    got = traj.read_all()
    assert np.array_equal(got["obs"][:, 0, :], sim.observe())
    for t in range(T):
        reward, flag, obs, term = sim.step(got["action"][t])
        assert np.array_equal(got["reward"][t], reward) and np.array_equal(got["flag"][t], flag), t
        assert np.array_equal(got["obs"][:, t + 1, :], obs), t
    assert (got["flag"] != O.CONTINUE).any() and set(np.unique(got["action"])) == {0, 1}
    z, _ = O.stack_seq_forward(CL.shape_of("gru", 5, H, 2), 1, CL.embed("gru", 5, H, 1, 2, True, pol.get_params()), got,
                               want_succ=False)
    zd, _ = pol.seq_forward(traj, want_succ=False)
    assert np.array_equal(z, zd)
    # the recorded actions are the inverse-CDF draws at those logits (samples within 1e-6 of the boundary set aside)
    r = O.Prng()
    checked = 0
    for t in range(T):
        p0 = 1.0 / (1.0 + np.exp(z[1, t].astype(np.float64) - z[0, t]))
        for i in range(n):
            O.lib().oracle_prng_seed_from_u64(C.byref(r), 4)
            O.lib().oracle_prng_set_stream(C.byref(r), i)
            O.lib().oracle_prng_set_word_pos(C.byref(r), t)
            u = O.lib().oracle_prng_gen_f32(C.byref(r))
            if abs(u - p0[i]) > 1e-6:
                assert got["action"][t, i] == (0 if u < p0[i] else 1), (t, i)
                checked += 1
    assert checked > 0.99 * n * T
    ra.gae(traj, cri, 0.95, 0.9)
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = 4
    cst, losses = ra.values_opt_update(cri, ra.Adam(cri), traj, ccfg, want_losses=True)
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    p0 = pol.get_params()
    st = ra.trpo_update(pol, traj)
    assert st.status == ra.OPT_OK and st.constraint_val_final <= 0.01 and st.loss_final < st.loss_initial
    assert np.isfinite(st.loss_final) and not np.array_equal(pol.get_params(), p0)
    cfg = ra.ppo_config_default()
    cfg.opt_steps_per_update = 4
    st, losses = ra.ppo_update(pol, ra.Adam(pol), traj, cfg, want_losses=True)
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    p1 = pol.get_params()
    st = ra.reinforce_update(pol, ra.Adam(pol), traj)
    assert np.isfinite(st.loss_first) and np.isfinite(st.entropy) and not np.array_equal(pol.get_params(), p1)
    assert np.all(np.isfinite(pol.get_params())) and np.all(np.isfinite(cri.get_params()))


@pytest.mark.parametrize("tails", ["linear-linear", "linear-mlp", "mlp-linear"])
def test_actor_critic_update_with_either_tail(engine, tails):
    """rl_actor_critic_update with both modules linear-tail, and with one of each on ONE trajectory (the workspace serves
    the tail of the module at hand): bit-identical to rl_trpo_update followed by rl_values_opt_update; the begin / finish
    pair gives the same"""
    n, T = 64, 12
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = 4
    ptail, ctail = tails.split("-")

    def build(tail, A, seed):
        m = ra.GruLinear(engine, 5, A, 20, num_layers=2) if tail == "linear" else ra.GruMlp(engine, 5, A, 20, 12, num_layers=2)
        m.init(seed)
        return m

    def run(how):
        env = ra.ChainEnv(engine, n, max_steps=9, seed_env=5, seed_actor=6)
        pol, cri = build(ptail, 2, 2), build(ctail, 1, 3)
        opt = ra.Adam(cri)
        traj = ra.Trajectory(engine, n, T, 5)
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.95)
        if how == "joint":
            pst, cst, losses = ra.actor_critic_update(pol, cri, opt, traj, None, ccfg, want_losses=True)
        elif how == "begin-finish":
            pst = ra.actor_critic_update_begin(pol, cri, opt, traj, None, ccfg)
            cst, losses = ra.actor_critic_update_finish(traj, want_losses=True)
        else:
            pst = ra.trpo_update(pol, traj)
            cst, losses = ra.values_opt_update(cri, opt, traj, ccfg, want_losses=True)
        return pol.get_params(), cri.get_params(), pst.as_dict(), losses.copy()

    a = run("in turn")
    for how in ("joint", "begin-finish"):
        b = run(how)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]), how
    assert a[2]["status"] == ra.OPT_OK and np.all(np.isfinite(a[3])) and a[3][-1] < a[3][0]


@pytest.mark.parametrize("cell,NL,bias", [("gru", 2, True), ("lstm", 1, False)])
def test_actor_documents(engine, cell, NL, bias):
    """Chain { first: RnnBase, second: Linear { kernel, bias }, activation: "Relu" } (ff/linear.rs:45-50): written, decoded,
    read back bit for bit; a document of the other tail than the module's is refused, either way"""
    D, H, A = 5, 12, 2
    env = ra.ChainEnv(engine, 64, max_steps=9, seed_env=3, seed_actor=4)
    m = module(engine, cell, D, H, NL, A, bias, seed=19)
    doc = ra.actor_to_cbor(env, m)
    chain = cbor_ref.decode(doc)["policy_module"]
    assert sorted(chain) == ["activation", "first", "second"] and chain["activation"] == "Relu"
    assert sorted(chain["second"]) == ["bias", "kernel"]
    assert chain["second"]["kernel"]["shape"] == [A, H] and chain["second"]["bias"]["shape"] == [A]
    p = m.get_params()
    assert bytes(chain["second"]["kernel"]["data"]) == p[-A * H - A:-A].tobytes()
    assert bytes(chain["second"]["bias"]["data"]) == p[-A:].tobytes()
    assert chain["first"]["weights"]["has_biases"] is bias and len(chain["first"]["weights"]["flat_weights"]) == (4 if bias else 2) * NL
    other = module(engine, cell, D, H, NL, A, bias)
    ra.module_from_cbor(other, doc)
    assert np.array_equal(other.get_params(), p)
    mlp_tail = (ra.GruMlp if cell == "gru" else ra.LstmMlp)(engine, D, A, H, H, num_layers=NL, rnn_bias=bias)
    mlp_tail.init(5)
    before = mlp_tail.get_params()
    assert code_of(lambda: ra.module_from_cbor(mlp_tail, doc)) == ra.ERR_INVALID_ARGUMENT
    assert np.array_equal(mlp_tail.get_params(), before)
    assert code_of(lambda: ra.module_from_cbor(other, ra.actor_to_cbor(env, mlp_tail))) == ra.ERR_INVALID_ARGUMENT
    assert np.array_equal(other.get_params(), p)


def test_refusals(engine):
    h = C.c_void_p()

    def create(cell=0, D=5, H=32, NL=1, bias=1, A=2):
        return ra.lib().rl_rnn_linear_create(engine.h, C.c_int32(cell), C.c_uint32(D), C.c_uint32(H), C.c_uint32(NL),
                                             C.c_int32(bias), C.c_uint32(A), C.byref(h))

    assert create(NL=0) == ra.ERR_BUILD_AGENT
    assert create(NL=5) == ra.ERR_UNSUPPORTED
    for kw in (dict(D=0), dict(D=9), dict(H=0), dict(H=257), dict(A=0), dict(A=3), dict(bias=2), dict(cell=2)):
        assert create(**kw) == ra.ERR_BUILD_AGENT, kw
        assert not h.value
    assert ra.lib().rl_rnn_linear_create(engine.h, C.c_int32(0), C.c_uint32(5), C.c_uint32(32), C.c_uint32(1), C.c_int32(1),
                                         C.c_uint32(2), None) == ra.ERR_INVALID_ARGUMENT
    for kw in (dict(D=1, H=1, NL=1, A=1), dict(D=8, H=256, NL=4, A=2, cell=1)):  # the corners of the range build
        assert create(**kw) == ra.OK
        assert ra.lib().rl_mlp_destroy(h) == ra.OK
    m = module(engine, "gru", 5, 16, 1, 2, True, seed=1)
    assert code_of(lambda: ra.Mlp.forward(m, np.zeros((3, 5), np.float32))) == ra.ERR_UNSUPPORTED  # rl_mlp_forward
    # rl_mlp_init_with
    assert code_of(lambda: ra.Mlp.init(m, 1, ("Uniform", "FanAvg", 0.0), ("Zeros", "FanAvg", 0.0))) == ra.ERR_UNSUPPORTED
    env3 = ra.MemoryEnv(engine, 64, 3, 2)  # five features, three actions
    assert code_of(lambda: ra.rollout(env3, m, ra.Trajectory(engine, 64, 4, 5))) == ra.ERR_UNSUPPORTED
    env = ra.ChainEnv(engine, 64, max_steps=9)
    assert code_of(lambda: ra.Dqn(env, m, ra.Adam(m), ra.dqn_config_default())) == ra.ERR_BUILD_AGENT


PERIODS = 10  # twice the smallest count at which two seeds both pass (below)


def test_the_experiments_agent_learns_to_use_its_memory(engine):
    """The configuration of tests/test_gpu_meta_bandit.py::test_a_recurrent_policy_learns_to_use_its_memory — OneHotBandits(2),
    five episodes per trial, 1,024 lanes, H = 32, rl_actor_critic_update with GAE lambda 0.3 and 10 critic steps — with the
    experiment's model, GRU -> ReLU -> Linear, as policy and critic.  The bar is the same: a policy without memory across
    inner episodes earns exactly E / 2 = 2.5 per trial (standard error over 4,096 evaluation trials at most 0.04); the mean
    trial reward must exceed 3.0.
    Measured on an MI355X with this configuration, evaluated after every period (profiles/chain_linear_learning_periods.txt):
    seed 40 gives 2.851 after 4 periods, 3.037 after 5, 3.795 after 10, 4.492 after 20; a second seed (50) 2.971 after 4,
    3.275 after 5, 4.112 after 10, 4.442 after 20; both stay above the bar from period 5 on and level off at 4.50 (the
    policy that remembers earns 4.5).  The test runs 10 = twice the smallest sufficient count."""
    n, E, trials, H, seed = 1024, 5, 2, 32, 40
    mean, se = learn(engine, n, E, trials, H, PERIODS, seed)
    print("mean trial reward after %d periods: %.3f (se %.3f)" % (PERIODS, mean, se))
    assert mean > 3.0


def learn(engine, n, E, trials, H, periods, seed):
    T = trials * (2 * E - 1)
    env = ra.MetaBanditEnv(engine, n, 2, E, "one_hot", seed_env=seed, seed_actor=seed + 1)
    pol, cri = ra.GruLinear(engine, env.D, 2, H), ra.GruLinear(engine, env.D, 1, H)
    pol.init(seed + 2)
    cri.init(seed + 3)
    opt = ra.Adam(cri)
    ccfg = ra.values_opt_config_default()
    ccfg.opt_steps_per_update = 10
    traj = ra.Trajectory(engine, n, T, env.D)
    for _ in range(periods):
        ra.rollout(env, pol, traj)
        ra.gae(traj, cri, 0.99, 0.3)
        ra.actor_critic_update(pol, cri, opt, traj, None, ccfg)
    ev_env = ra.MetaBanditEnv(engine, 4096, 2, E, "one_hot", seed_env=seed + 10, seed_actor=seed + 11)
    ev_traj = ra.Trajectory(engine, 4096, 2 * E - 1, env.D)  # one whole trial per lane
    ra.rollout(ev_env, pol, ev_traj)
    assert np.all(ev_traj.read(ra.TRAJ_FLAG)[-1] == M.INTERRUPT)
    trial_reward = ev_traj.read(ra.TRAJ_REWARD).astype(np.float64).sum(axis=0)
    return trial_reward.mean(), trial_reward.std() / 64.0


def test_cpp_host_mirror_builds_the_experiments_agent():
    """tests/cpp/rl2_chain_linear_demo.cpp: ActorCriticConfig<TrpoConfig<GruLinearConfig>, ValuesOptConfig<GruLinearConfig>>
    on two-arm meta lanes, two periods; prints P and the two critic losses"""
    ra.build()
    exe = os.path.join(tempfile.mkdtemp(), "rl2_chain_linear_demo")
    libdir = os.path.join(ROOT, "relearn_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", ROOT,
                           os.path.join(ROOT, "tests", "cpp", "rl2_chain_linear_demo.cpp"), "-o", exe, "-L", libdir,
                           "-lrelearn_hip", "-Wl,-rpath," + libdir])
    words = subprocess.check_output([exe], timeout=120).decode().split()
    H, D = 32, 6
    rnn = 3 * H * D + 3 * H * H + 6 * H
    assert (int(words[0]), int(words[1])) == (rnn + 2 * H + 2, rnn + H + 1)
    losses = [float(w) for w in words[2:]]
    assert len(losses) == 2 and np.all(np.isfinite(losses)) and min(losses) > 0
