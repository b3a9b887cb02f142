"""The case table of the two-rank tests of recurrent and general modules (tests/test_gpu_sharded_modules.py on the
device, tests/test_sharded_cases_cpu.py for the table itself).  A plain table: nothing here imports the device library
or the oracle.

Every row takes its module shapes and its env from a case a one-rank test already runs (`taken_from` says which), so a
failure points at the sharding and not at the shape.  World size 2, equal shards: `lanes` is the lane count of EACH
rank, the whole batch is 2 * lanes lanes of T steps.  Lanes are independent columns in every kernel, so the one-rank f64
reference over all lanes is the reference of the sharded run as well.

Per-rank lane counts are the smallest that still reach the family's edges: 32 and 96 are one and three tiles of the tile
kernels (an odd tile count), 35 and 33 are off the wave size of the lane kernels on each rank and in the sum (70, 66), 64
is one wave per rank of the feed-forward kernels."""
import collections

WORLD = 2
LOOPBACK_SKEW_MIN = 64  # RELEARN_LOOPBACK_TEST_WEIGHT leaves vectors of <= 64 floats alone (abi.hip, loopback_allreduce)

# a recurrent chain in the fields of tests/seq_multi_ref.py's Net (H2 = 0: a Linear tail); out_dim A
Net = collections.namedtuple("Net", "cell D H L H2 bias A")
# a feed-forward module: MlpConfig's hidden_sizes, the activation's variant name
Mlp = collections.namedtuple("Mlp", "D hidden act A")
# env: (kind, keyword arguments of the constructor) or ("history", seed): the host-written planes of
# tests/seq_multi_ref.py's history(), what the row's one-rank test runs
# seeds: (policy init, critic init); checks: which of the longer checks run on the row beside the probe vectors, the
# exchange counts and the first-order updates every row gets
Row = collections.namedtuple("Row", "id family ctor policy critic env lanes T seeds gae taken_from checks")

CHAIN = ("chain", dict(max_steps=3, seed_env=3, seed_actor=4))          # tests/test_gpu_gru.py chain_pair, edge shapes
CHAIN9 = ("chain", dict(max_steps=9, seed_env=3, seed_actor=4))         # tests/test_gpu_stacked.py, chain lanes
CARTPOLE = ("cartpole", dict(max_steps=9, seed_env=5, seed_actor=6))    # tests/narrow_cases.py ROLLOUT_SEEDS, max_steps

ROWS = [
    # ---- tile kernels (kernels_seq_train.hip, kernels_seq_fvp.hip): 5 -> 128 -> 128 -> A, one layer, an MLP tail
    Row("tile-gru-32", "tile", "GruMlp", Net("gru", 5, 128, 1, 128, True, 2), Net("gru", 5, 128, 1, 128, True, 1), CHAIN,
        32, 7, (21, 22), (0.95, 0.9), "tests/test_gpu_gru.py edge shapes (one tile, max_steps=3)",
        ("trpo", "actor_critic", "both_targets", "negative")),
    Row("tile-gru-96", "tile", "GruMlp", Net("gru", 5, 128, 1, 128, True, 2), Net("gru", 5, 128, 1, 128, True, 1), CHAIN,
        96, 7, (21, 22), (0.95, 0.9), "tests/test_gpu_gru.py edge shapes (96, 7, 3): three tiles", ()),
    Row("tile-lstm-32", "tile", "LstmMlp", Net("lstm", 5, 128, 1, 128, True, 2), Net("lstm", 5, 128, 1, 128, True, 1), CHAIN,
        32, 7, (21, 22), (0.95, 0.9), "tests/test_gpu_lstm.py setup_update, edge shapes", ()),
    # a narrow chain on the tile kernels: it runs on a zero-padded 5-128-128 twin (rl_mlp::exec), and its gradient comes
    # back in the twin's layout — the one row whose passes gather into flat order (seq_gradient_to_flat_order) and pad
    # the tangent before the exchange
    Row("tile-gru-narrow-32", "tile", "GruMlp", Net("gru", 5, 128, 1, 40, True, 2), Net("gru", 5, 32, 1, 64, True, 1), CHAIN,
        32, 7, (41, 41), (0.95, 0.9), "tests/test_gpu_gru.py NARROW (gru, 5, 128, 40, 2) and (gru, 5, 32, 64, 1)", ()),
    # ---- lane kernels (kernels_seq_stack.hip), stacked layers
    Row("stacked-gru-2", "lane", "GruMlp", Net("gru", 5, 32, 2, 16, True, 2), Net("lstm", 5, 16, 2, 8, True, 1), CHAIN9,
        35, 6, (41, 14), (0.95, 0.9), "tests/test_gpu_stacked.py SHAPES[0]; critic: test_rollout_and_updates_on_chain_lanes",
        ("trpo", "negative")),
    Row("stacked-lstm-2-nobias", "lane", "LstmMlp", Net("lstm", 5, 24, 2, 12, False, 2), Net("gru", 5, 32, 2, 16, True, 1),
        CHAIN9, 35, 6, (51, 41), (0.95, 0.9),
        "tests/test_gpu_stacked.py test_recurrent_layers_without_bias_vectors; critic: SHAPES[0] at one output", ()),
    # ---- lane kernels, linear head (the RL2 experiment's model on two arms)
    Row("linear-gru-meta2", "lane", "GruLinear", Net("gru", 6, 7, 1, 0, True, 2), Net("gru", 6, 7, 1, 0, True, 1),
        ("meta", dict(n_arms=2, episodes_per_trial=3, distribution="uniform_bernoulli", seed_env=302, seed_actor=303)),
        33, 5, (301, 302), (0.99, 0.3), "tests/chain_linear_ref.py META_CASES[0], tests/test_gpu_chain_linear.py SHAPES", ()),
    # ---- lane kernels, 3..8 actions
    Row("multi-gru-A3", "lane", "RnnChain", Net("gru", 7, 7, 1, 6, True, 3), Net("lstm", 7, 8, 1, 6, True, 1),
        ("meta", dict(n_arms=3, episodes_per_trial=3, distribution="one_hot", seed_env=3, seed_actor=4)),
        35, 6, (31, 32), (0.99, 0.3), "tests/test_gpu_seq_multi_action.py NETS[0]; env and critic: its update test", ()),
    Row("multi-lstm-A3", "lane", "RnnChain", Net("lstm", 7, 9, 2, 6, True, 3), Net("lstm", 7, 8, 1, 6, True, 1),
        ("meta", dict(n_arms=3, episodes_per_trial=3, distribution="one_hot", seed_env=412, seed_actor=413)),
        35, 6, (411, 32), (0.99, 0.3), "tests/seq_multi_ref.py META_CASES[1]", ()),
    Row("multi-gru-A8", "lane", "RnnChain", Net("gru", 5, 33, 1, 0, True, 8), Net("gru", 5, 12, 1, 0, True, 1),
        ("history", 6), 35, 6, (41, 3), None, "tests/test_gpu_seq_multi_action.py NETS[2] on its written history",
        ("trpo",)),
    Row("multi-lstm-A8", "lane", "RnnChain", Net("lstm", 5, 7, 1, 6, True, 8), Net("gru", 5, 12, 1, 0, True, 1),
        ("history", 6), 35, 6, (41, 3), None, "tests/test_gpu_seq_multi_action.py NETS[4] on its written history", ()),
    # ---- lane kernels, wide (9 and 12 arms: 13 and 16 features); one trial of 3 episodes is 5 steps
    Row("wide-gru-13-9", "lane", "RnnChainWide", Net("gru", 13, 7, 1, 0, True, 9), Net("gru", 13, 7, 1, 0, True, 1),
        ("meta_wide", dict(n_arms=9, episodes_per_trial=3, distribution="one_hot", seed_env=3, seed_actor=4)),
        35, 5, (31, 32), (0.99, 0.3), "tests/wide_meta_cases.py NETS[2]", ()),
    Row("wide-lstm-16-12", "lane", "RnnChainWide", Net("lstm", 16, 33, 2, 6, True, 12), Net("lstm", 16, 33, 1, 6, True, 1),
        ("meta_wide", dict(n_arms=12, episodes_per_trial=3, distribution="uniform_bernoulli", seed_env=3, seed_actor=4)),
        35, 5, (31, 32), (0.99, 0.3), "tests/wide_meta_cases.py NETS[4]; critic: CRITICS[1] at one output", ("trpo",)),
    # ---- feed-forward modules
    Row("general-16-16-tanh-A4", "general", "Mlp", Mlp(7, (16, 16), "Tanh", 4), Mlp(7, (16, 16), "Tanh", 1),
        ("memory", dict(num_actions=4, history_len=3, seed_env=32, seed_actor=33)), 64, 9, (31, 62), (0.99, 0.95),
        "tests/test_gpu_multi_action.py (4, 3, [16, 16], Tanh)", ("actor_critic", "negative")),
    Row("narrow-5-17", "narrow", "Mlp", Mlp(5, (17,), "Relu", 2), Mlp(5, (17,), "Relu", 1), CARTPOLE, 64, 9, (2, 3),
        (0.99, 0.95), "tests/narrow_cases.py SHAPES (5, 17), MODULE_SEEDS", ()),
    Row("fused-5-128", "fused", "Mlp", Mlp(5, (128,), "Relu", 2), Mlp(5, (128,), "Relu", 1),
        ("cartpole", dict(max_steps=40, seed_env=5, seed_actor=6)), 64, 9, (2, 3), (0.99, 0.95),
        "tests/test_gpu_multirank.py run_rank", ("both_targets",)),
]
ROW_IDS = [r.id for r in ROWS]
TRPO_ROWS = [r.id for r in ROWS if "trpo" in r.checks]
ACTOR_CRITIC_ROWS = [r.id for r in ROWS if "actor_critic" in r.checks]
NEGATIVE_ROWS = [r.id for r in ROWS if "negative" in r.checks]


def row(row_id):
    return ROWS[ROW_IDS.index(row_id)]


def num_params(m):
    """P of a module of the table, in closed form (the device's count is compared with it on the GPU)"""
    if isinstance(m, Mlp):
        w = [m.D] + list(m.hidden) + [m.A]
        return sum(fi * fo + fo for fi, fo in zip(w[:-1], w[1:]))
    G = 4 if m.cell == "lstm" else 3
    P = sum(G * m.H * (m.D if l == 0 else m.H) + G * m.H * m.H + (2 * G * m.H if m.bias else 0) for l in range(m.L))
    if m.H2 == 0:
        return P + m.A * m.H + m.A
    return P + m.H2 * m.H + m.H2 + m.A * m.H2 + m.A


# the exchanges rl_allreduce_sum_f32 makes per call with a collective installed (run_pass, abi_update.hip): one per pass
PPO_STEPS, CRITIC_STEPS = 3, 3


def prescribed_exchanges(call, steps=0):
    return {"policy_gradient": 1, "policy_fvp": 2, "critic_gradient": 1, "ppo_update": 1 + steps, "reinforce_update": 1,
            "critic_update": steps, "values_opt_update": steps}[call]
