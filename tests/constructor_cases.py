"""The case list of the constructor table: what every env and module constructor of the C ABI refuses, in which order,
and what it decides for the shapes it accepts.  Two tests read it:

  tests/test_gpu_constructor_table.py  makes every call on the device and compares with tests/golden/constructor_table.json
  tests/test_handle_spec_cpp.py        feeds the same list to tests/cpp/handle_spec_demo.cpp (the HIP-free half of the
                                       constructors, csrc/handle_spec.hpp) and compares with the same file

A case is (name, constructor, numbers).  The numbers of each constructor, in order:

  env              kind limit_kind max_steps n_lanes chain_size memory_num_actions memory_history_len      rl_env_create
  bandit           kind limit_kind max_steps n_lanes n_arms          rl_env_create_bandit, arm a's value = 0.5 a - 1
  meta, meta_wide  limit_kind max_steps n_lanes n_arms distribution episodes_per_trial   rl_env_create_meta_bandit[_wide]
  mdp              limit_kind max_steps n_lanes n_states n_actions discount_factor table     rl_env_create_tabular_mdp
  meta_as, meta_wide_as, mdp_as    kind memory_num_actions memory_history_len, then the numbers of meta / mdp: the same
                   constructors on a config that says another kind (they name the kind; cfg.kind is not read)
  mlp              in_dim hidden out_dim                                                     rl_mlp_create
  mlp_layers       in_dim out_dim activation output_activation n_hidden widths..            rl_mlp_create_layers
  mlp_config       in_dim out_dim activation output_activation bias n_hidden widths..       rl_mlp_create_config
  gru_mlp, lstm_mlp    in_dim hidden mlp_hidden out_dim                        rl_gru_mlp_create, rl_lstm_mlp_create
  rnn_mlp          cell in_dim hidden num_layers mlp_hidden out_dim                          rl_rnn_mlp_create
  rnn_mlp_config   cell in_dim hidden num_layers bias mlp_hidden out_dim                     rl_rnn_mlp_create_config
  rnn_linear       cell in_dim hidden num_layers rnn_bias out_dim                            rl_rnn_linear_create
  chain, chain_wide    cell in_dim hidden num_layers rnn_bias mlp_hidden out_dim       rl_rnn_chain_create[_wide]
  init_mlp         module, then kernel_init and bias_init as (given kind scale value)        rl_mlp_init_with
  init_rnn         module, then input, hidden, bias, mlp_kernel, mlp_bias as (given ...)     rl_rnn_mlp_init_with

`table` of an mdp case (S states, A actions; row = state * A + action): every transition row is uniform, (float)(1 / S)
each; reward_mean[row] = 0.25 row; reward_stddev NULL — then 1: transitions[row 3][0] = -0.5, 2: transitions[row 1][0] = 0,
3: reward_mean[2] = inf, 4: reward_stddev given, 0.5 everywhere but [1] = -1, 5: reward_stddev given, 0.5 everywhere,
6: both 2 and 3.
`module` of an init case: 0 Mlp(4, [3], 1), 1 the same without bias vectors, 2 a GRU chain 4-3-3-1, 3 the same without
recurrent bias vectors.

    python tests/constructor_cases.py        prints the list, one case per line: what the demo reads
"""
ENV_CARTPOLE, ENV_CHAIN, ENV_MEMORY, ENV_BANDIT, ENV_META, ENV_MDP = range(6)
NONE, LATENT, VISIBLE = 0, 1, 2
UNIFORM, ONE_HOT, ROUND_ROBIN = 0, 1, 2
IDENTITY, RELU, SIGMOID, TANH = range(4)
GRU, LSTM = 0, 1
ZEROS, CONSTANT, UNIFORM_INIT, NORMAL, ORTHOGONAL = range(5)
SC_CONSTANT, FAN_IN, FAN_OUT, FAN_AVG = range(4)


def init(kind=UNIFORM_INIT, scale=FAN_AVG, value=0.0):
    return [1, kind, scale, value]


ABSENT = [0, 0, 0, 0.0]
GLOROT, ORTHO, ZERO = init(), init(ORTHOGONAL), init(ZEROS)

CASES = [
    # ------------------------------------------------------------------ refusals: rl_env_create
    ("env-kind-meta", "env", [ENV_META, NONE, 0, 4, 0, 0, 0]),
    ("env-kind-mdp", "env", [ENV_MDP, NONE, 0, 4, 0, 0, 0]),
    ("env-kind-unknown", "env", [99, NONE, 0, 4, 0, 0, 0]),
    ("env-kind-negative", "env", [-1, NONE, 0, 4, 0, 0, 0]),
    ("memory-3-features", "env", [ENV_MEMORY, NONE, 0, 4, 0, 2, 1]),
    ("memory-1-action", "env", [ENV_MEMORY, NONE, 0, 4, 0, 1, 4]),
    ("memory-no-history", "env", [ENV_MEMORY, NONE, 0, 4, 0, 4, 0]),
    ("memory-9-actions", "env", [ENV_MEMORY, NONE, 0, 4, 0, 9, 1]),
    ("memory-9-features", "env", [ENV_MEMORY, NONE, 0, 4, 0, 4, 5]),
    ("memory-8-features-visible", "env", [ENV_MEMORY, VISIBLE, 5, 4, 0, 4, 4]),
    ("chain-3-states", "env", [ENV_CHAIN, LATENT, 10, 4, 3, 0, 0]),
    ("limit-of-0-steps", "env", [ENV_CARTPOLE, VISIBLE, 0, 4, 0, 0, 0]),
    ("limit-of-2^32-steps", "env", [ENV_CHAIN, LATENT, 1 << 32, 4, 5, 0, 0]),
    ("no-lanes", "env", [ENV_CARTPOLE, VISIBLE, 9, 0, 0, 0, 0]),
    ("2^31-lanes", "env", [ENV_CARTPOLE, VISIBLE, 9, 1 << 31, 0, 0, 0]),
    ("bandit-under-limit", "env", [ENV_BANDIT, LATENT, 3, 4, 0, 0, 0]),
    # ... in order: the first of two that apply
    ("order-memory-3-features-no-lanes", "env", [ENV_MEMORY, NONE, 0, 0, 0, 2, 1]),
    ("order-chain-3-states-limit-0", "env", [ENV_CHAIN, LATENT, 0, 4, 3, 0, 0]),
    ("order-limit-0-no-lanes", "env", [ENV_CARTPOLE, LATENT, 0, 0, 0, 0, 0]),
    ("order-bandit-limit-0", "env", [ENV_BANDIT, LATENT, 0, 4, 0, 0, 0]),
    ("order-bandit-limit-no-lanes", "env", [ENV_BANDIT, LATENT, 3, 0, 0, 0, 0]),
    # ------------------------------------------------------------------ rl_env_create_bandit
    ("bandit-values-on-chain", "bandit", [ENV_CHAIN, NONE, 0, 4, 3]),
    ("bandit-1-arm", "bandit", [ENV_BANDIT, NONE, 0, 4, 1]),
    ("bandit-9-arms", "bandit", [ENV_BANDIT, NONE, 0, 4, 9]),
    ("bandit-3-arms-under-limit", "bandit", [ENV_BANDIT, VISIBLE, 3, 4, 3]),
    ("order-bandit-limit-9-arms", "bandit", [ENV_BANDIT, LATENT, 3, 4, 9]),
    ("order-bandit-values-on-meta-kind", "bandit", [ENV_META, NONE, 0, 4, 3]),
    ("order-bandit-9-arms-no-lanes", "bandit", [ENV_BANDIT, NONE, 0, 0, 9]),
    # ------------------------------------------------------------------ rl_env_create_meta_bandit[_wide]
    ("meta-1-arm", "meta", [NONE, 0, 4, 1, UNIFORM, 3]),
    ("meta-5-arms", "meta", [NONE, 0, 4, 5, UNIFORM, 3]),
    ("meta-wide-1-arm", "meta_wide", [NONE, 0, 4, 1, UNIFORM, 3]),
    ("meta-wide-13-arms", "meta_wide", [NONE, 0, 4, 13, UNIFORM, 3]),
    ("meta-no-episodes", "meta", [NONE, 0, 4, 2, UNIFORM, 0]),
    ("meta-2^32-episodes", "meta", [NONE, 0, 4, 2, UNIFORM, 1 << 32]),
    ("meta-distribution-unknown", "meta", [NONE, 0, 4, 2, 3, 3]),
    ("meta-distribution-negative", "meta_wide", [NONE, 0, 4, 9, -1, 3]),
    ("meta-under-limit", "meta", [LATENT, 5, 4, 2, UNIFORM, 3]),
    ("meta-no-lanes", "meta_wide", [NONE, 0, 0, 12, ONE_HOT, 3]),
    ("order-meta-limit-no-episodes", "meta", [VISIBLE, 5, 4, 2, UNIFORM, 0]),
    ("order-meta-wide-13-arms-distribution", "meta_wide", [NONE, 0, 4, 13, 7, 3]),
    ("order-meta-5-arms-no-episodes", "meta", [NONE, 0, 4, 5, UNIFORM, 0]),
    ("order-meta-episodes-distribution", "meta", [NONE, 0, 4, 3, 7, 1 << 32]),
    ("order-meta-limit-0-steps", "meta", [LATENT, 0, 4, 2, UNIFORM, 3]),
    # ------------------------------------------------------------------ rl_env_create_tabular_mdp
    ("mdp-1-state", "mdp", [NONE, 0, 4, 1, 2, 1.0, 0]),
    ("mdp-9-states", "mdp", [NONE, 0, 4, 9, 2, 1.0, 0]),
    ("mdp-1-action", "mdp", [NONE, 0, 4, 2, 1, 1.0, 0]),
    ("mdp-9-actions", "mdp", [NONE, 0, 4, 2, 9, 1.0, 0]),
    ("mdp-8-states-visible", "mdp", [VISIBLE, 5, 4, 8, 2, 1.0, 0]),
    ("mdp-discount-inf", "mdp", [NONE, 0, 4, 2, 2, "inf", 0]),
    ("mdp-negative-probability", "mdp", [NONE, 0, 4, 2, 2, 1.0, 1]),
    ("mdp-row-sum", "mdp", [NONE, 0, 4, 3, 2, 1.0, 2]),
    ("mdp-mean-inf", "mdp", [NONE, 0, 4, 2, 3, 1.0, 3]),
    ("mdp-negative-stddev", "mdp", [NONE, 0, 4, 2, 2, 1.0, 4]),
    ("mdp-limit-of-0-steps", "mdp", [LATENT, 0, 4, 2, 2, 1.0, 0]),
    ("mdp-no-lanes", "mdp", [NONE, 0, 0, 2, 2, 1.0, 0]),
    ("order-mdp-9-states-discount", "mdp", [NONE, 0, 4, 9, 2, "inf", 0]),
    ("order-mdp-table-no-lanes", "mdp", [NONE, 0, 0, 2, 2, 1.0, 1]),
    ("order-mdp-row-sum-before-mean-of-later-row", "mdp", [NONE, 0, 4, 2, 2, 1.0, 6]),
    # ... whatever cfg.kind says: nothing of another kind's rules applies (all accepted)
    ("mdp-on-bandit-config-under-limit", "mdp_as", [ENV_BANDIT, 0, 0, LATENT, 4, 4, 2, 2, 1.0, 0]),
    ("mdp-on-memory-config-of-3-features", "mdp_as", [ENV_MEMORY, 2, 1, VISIBLE, 4, 4, 3, 2, 1.0, 5]),
    ("mdp-on-chain-config", "mdp_as", [ENV_CHAIN, 0, 0, NONE, 0, 4, 2, 2, 1.0, 0]),
    ("mdp-on-unknown-kind", "mdp_as", [99, 0, 0, NONE, 0, 4, 2, 2, 1.0, 0]),
    ("meta-on-bandit-config", "meta_as", [ENV_BANDIT, 0, 0, NONE, 0, 4, 2, UNIFORM, 3]),
    ("meta-on-memory-config-of-3-features", "meta_as", [ENV_MEMORY, 2, 1, NONE, 0, 4, 3, ONE_HOT, 3]),
    ("meta-wide-on-mdp-config", "meta_wide_as", [ENV_MDP, 9, 9, NONE, 0, 4, 6, ROUND_ROBIN, 3]),
    ("meta-on-negative-kind", "meta_as", [-1, 0, 0, NONE, 0, 4, 2, UNIFORM, 3]),
    ("order-meta-on-bandit-config-under-limit", "meta_as", [ENV_BANDIT, 0, 0, LATENT, 3, 4, 2, UNIFORM, 3]),  # meta's words
    # ------------------------------------------------------------------ rl_mlp_create
    ("mlp-in-3", "mlp", [3, 8, 2]),
    ("mlp-in-6", "mlp", [6, 8, 2]),
    ("mlp-out-0", "mlp", [5, 8, 0]),
    ("mlp-out-3", "mlp", [5, 8, 3]),
    ("mlp-hidden-0", "mlp", [5, 0, 2]),
    ("mlp-hidden-129", "mlp", [5, 129, 2]),
    # ------------------------------------------------------------------ rl_mlp_create_layers / rl_mlp_create_config
    ("layers-in-0", "mlp_layers", [0, 2, RELU, IDENTITY, 1, 8]),
    ("layers-in-9", "mlp_layers", [9, 2, RELU, IDENTITY, 1, 8]),
    ("layers-out-0", "mlp_layers", [6, 0, RELU, IDENTITY, 1, 8]),
    ("layers-out-9", "mlp_layers", [5, 9, RELU, IDENTITY, 1, 8]),
    ("layers-5-hidden", "mlp_layers", [5, 2, RELU, IDENTITY, 5, 8, 8, 8, 8, 8]),
    ("layers-width-0", "mlp_layers", [5, 2, RELU, IDENTITY, 2, 8, 0]),
    ("layers-width-257", "mlp_layers", [5, 2, RELU, IDENTITY, 2, 257, 8]),
    ("layers-activation-4", "mlp_layers", [5, 2, 4, IDENTITY, 1, 8]),
    ("layers-activation-negative", "mlp_config", [5, 2, -1, IDENTITY, 1, 1, 8]),
    ("layers-output-activation-4", "mlp_config", [5, 2, RELU, 4, 0, 1, 8]),
    ("layers-output-activation-negative", "mlp_layers", [5, 2, TANH, -1, 1, 8]),
    ("order-layers-fused-shape-width-0", "mlp_layers", [5, 2, RELU, IDENTITY, 1, 0]),  # handed to rl_mlp_create: its words
    ("order-layers-width-0-no-bias", "mlp_config", [5, 2, RELU, IDENTITY, 0, 1, 0]),
    ("order-layers-shape-activation", "mlp_layers", [9, 2, 7, IDENTITY, 1, 8]),
    # ------------------------------------------------------------------ the recurrent constructors
    ("gru-mlp-in-0", "gru_mlp", [0, 8, 8, 2]),
    ("gru-mlp-in-9", "gru_mlp", [9, 8, 8, 2]),
    ("lstm-mlp-hidden-0", "lstm_mlp", [5, 0, 8, 2]),
    ("lstm-mlp-hidden-257", "lstm_mlp", [5, 257, 8, 2]),
    ("gru-mlp-mlp-hidden-0", "gru_mlp", [5, 8, 0, 2]),
    ("gru-mlp-mlp-hidden-257", "gru_mlp", [5, 8, 257, 2]),
    ("lstm-mlp-out-0", "lstm_mlp", [5, 8, 8, 0]),
    ("gru-mlp-out-3", "gru_mlp", [5, 8, 8, 3]),
    ("rnn-mlp-cell", "rnn_mlp", [2, 5, 8, 1, 8, 2]),
    ("rnn-mlp-no-layers", "rnn_mlp", [GRU, 5, 8, 0, 8, 2]),
    ("rnn-mlp-5-layers", "rnn_mlp", [LSTM, 5, 8, 5, 8, 2]),
    ("rnn-mlp-out-3", "rnn_mlp", [LSTM, 5, 8, 2, 8, 3]),
    ("rnn-mlp-config-cell", "rnn_mlp_config", [-1, 5, 8, 1, 1, 8, 2]),
    ("rnn-mlp-config-mlp-hidden-0", "rnn_mlp_config", [GRU, 5, 8, 1, 0, 0, 2]),
    ("rnn-linear-cell", "rnn_linear", [2, 5, 8, 1, 1, 2]),
    ("rnn-linear-bias-2", "rnn_linear", [GRU, 5, 8, 1, 2, 2]),
    ("rnn-linear-out-3", "rnn_linear", [GRU, 5, 8, 1, 1, 3]),
    ("rnn-linear-in-9", "rnn_linear", [LSTM, 9, 8, 1, 0, 2]),
    ("chain-cell", "chain", [2, 5, 8, 1, 1, 8, 2]),
    ("chain-bias-2", "chain", [GRU, 5, 8, 1, 2, 8, 2]),
    ("chain-bias-negative", "chain", [GRU, 5, 8, 1, -1, 8, 2]),
    ("chain-mlp-hidden-257", "chain", [GRU, 8, 8, 1, 1, 257, 8]),
    ("chain-out-9", "chain", [GRU, 5, 8, 1, 1, 8, 9]),
    ("chain-out-0", "chain", [LSTM, 5, 8, 1, 1, 0, 0]),
    ("chain-hidden-257", "chain", [LSTM, 5, 257, 1, 1, 0, 3]),
    ("chain-no-layers", "chain", [GRU, 5, 8, 0, 1, 8, 3]),
    ("chain-wide-cell", "chain_wide", [2, 16, 8, 1, 1, 8, 12]),
    ("chain-wide-bias-2", "chain_wide", [GRU, 16, 8, 1, 2, 8, 12]),
    ("chain-wide-in-17", "chain_wide", [GRU, 17, 8, 1, 1, 8, 2]),
    ("chain-wide-out-13", "chain_wide", [LSTM, 5, 8, 1, 1, 0, 13]),
    ("chain-wide-in-0-out-12", "chain_wide", [LSTM, 0, 8, 1, 1, 0, 12]),
    ("chain-wide-5-layers", "chain_wide", [GRU, 16, 8, 5, 1, 8, 12]),
    ("chain-wide-narrow-out-0", "chain_wide", [GRU, 5, 8, 1, 1, 8, 0]),  # within the narrow bounds: rl_rnn_chain_create's words
    ("order-chain-5-layers-in-0", "chain", [GRU, 0, 8, 5, 1, 8, 2]),
    ("order-rnn-mlp-no-layers-in-0", "rnn_mlp", [GRU, 0, 8, 0, 8, 2]),
    ("order-rnn-linear-cell-bias", "rnn_linear", [2, 5, 8, 1, 2, 2]),
    ("order-chain-cell-bias", "chain", [2, 5, 8, 1, 2, 8, 2]),
    ("order-chain-wide-cell-bias", "chain_wide", [2, 16, 8, 1, 2, 8, 12]),
    ("order-chain-wide-narrow-cell-bias", "chain_wide", [2, 5, 8, 1, 2, 8, 2]),
    ("order-chain-bias-layers", "chain", [GRU, 5, 8, 0, 2, 8, 2]),
    ("order-rnn-mlp-config-cell-layers", "rnn_mlp_config", [2, 5, 8, 0, 2, 8, 2]),
    # ------------------------------------------------------------------ rl_mlp_init_with / rl_rnn_mlp_init_with
    ("init-mlp-on-chain", "init_mlp", [2] + GLOROT + GLOROT),
    ("init-mlp-bias-init-missing", "init_mlp", [0] + GLOROT + ABSENT),
    ("init-mlp-bias-init-given", "init_mlp", [1] + GLOROT + GLOROT),
    ("init-mlp-kind", "init_mlp", [0] + init(5) + GLOROT),
    ("init-mlp-kind-negative", "init_mlp", [0] + GLOROT + init(-1)),
    ("init-mlp-scale", "init_mlp", [0] + init(NORMAL, 4) + GLOROT),
    ("init-mlp-ok-scale-unread", "init_mlp", [0] + init(CONSTANT, 9, 0.5) + init(ZEROS, -3)),
    ("init-mlp-negative-variance", "init_mlp", [0] + GLOROT + init(UNIFORM_INIT, SC_CONSTANT, -0.5)),
    ("init-mlp-orthogonal-bias", "init_mlp", [0] + ORTHO + ORTHO),
    ("init-mlp-ok", "init_mlp", [0] + init(NORMAL, FAN_IN) + init(CONSTANT, SC_CONSTANT, 0.1)),
    ("init-mlp-ok-no-bias", "init_mlp", [1] + ORTHO + ABSENT),
    ("order-init-mlp-chain-kind", "init_mlp", [2] + init(5) + ABSENT),
    ("order-init-mlp-bias-missing-kind", "init_mlp", [0] + init(5) + ABSENT),
    ("order-init-mlp-kind-orthogonal-bias", "init_mlp", [0] + init(NORMAL, 7) + ORTHO),
    ("init-rnn-on-mlp", "init_rnn", [0] + GLOROT + ORTHO + ZERO + GLOROT + GLOROT),
    ("init-rnn-bias-init-missing", "init_rnn", [2] + GLOROT + ORTHO + ABSENT + GLOROT + GLOROT),
    ("init-rnn-bias-init-given", "init_rnn", [3] + GLOROT + ORTHO + ZERO + GLOROT + GLOROT),
    ("init-rnn-mlp-bias-missing", "init_rnn", [2] + GLOROT + ORTHO + ZERO + GLOROT + ABSENT),
    ("init-rnn-input-missing", "init_rnn", [2] + ABSENT + ORTHO + ZERO + GLOROT + GLOROT),
    ("init-rnn-hidden-missing", "init_rnn", [2] + GLOROT + ABSENT + ZERO + GLOROT + GLOROT),
    ("init-rnn-mlp-kernel-missing", "init_rnn", [3] + GLOROT + ORTHO + ABSENT + ABSENT + GLOROT),
    ("init-rnn-kind", "init_rnn", [2] + GLOROT + init(5) + ZERO + GLOROT + GLOROT),
    ("init-rnn-scale", "init_rnn", [2] + GLOROT + ORTHO + ZERO + init(UNIFORM_INIT, -1) + GLOROT),
    ("init-rnn-negative-variance", "init_rnn", [2] + init(NORMAL, SC_CONSTANT, -1.0) + ORTHO + ZERO + GLOROT + GLOROT),
    ("init-rnn-orthogonal-bias", "init_rnn", [2] + GLOROT + ORTHO + ORTHO + GLOROT + GLOROT),
    ("init-rnn-orthogonal-mlp-bias", "init_rnn", [3] + GLOROT + ORTHO + ABSENT + GLOROT + ORTHO),
    ("init-rnn-ok", "init_rnn", [2] + ORTHO + GLOROT + init(CONSTANT, SC_CONSTANT, 0.25) + init(NORMAL, FAN_OUT) + ZERO),
    ("init-rnn-ok-no-bias", "init_rnn", [3] + GLOROT + ORTHO + ABSENT + GLOROT + GLOROT),
    ("order-init-rnn-bias-missing-mlp-bias-missing", "init_rnn", [2] + GLOROT + ORTHO + ABSENT + GLOROT + ABSENT),
    ("order-init-rnn-mlp-bias-missing-input-missing", "init_rnn", [2] + ABSENT + ORTHO + ZERO + GLOROT + ABSENT),
    ("order-init-rnn-input-missing-kind", "init_rnn", [2] + ABSENT + init(9) + ZERO + GLOROT + GLOROT),
    ("order-init-rnn-kind-orthogonal-bias", "init_rnn", [2] + GLOROT + ORTHO + ORTHO + init(7) + GLOROT),
    # ------------------------------------------------------------------ accepted: envs at the edges of every bound
    ("cartpole-visible", "env", [ENV_CARTPOLE, VISIBLE, 9, 64, 0, 0, 0]),
    ("cartpole-latent", "env", [ENV_CARTPOLE, LATENT, (1 << 32) - 1, 33, 0, 0, 0]),
    ("cartpole-no-limit", "env", [ENV_CARTPOLE, NONE, 0, 1, 0, 0, 0]),
    ("cartpole-no-limit-steps-ignored", "env", [ENV_CARTPOLE, NONE, 1 << 32, 2, 7, 9, 9]),
    ("chain-default-size", "env", [ENV_CHAIN, LATENT, 100, 7, 0, 0, 0]),
    ("chain-5-visible", "env", [ENV_CHAIN, VISIBLE, 1, 64, 5, 0, 0]),
    ("memory-default", "env", [ENV_MEMORY, NONE, 0, 5, 0, 0, 0]),
    ("memory-history-alone", "env", [ENV_MEMORY, NONE, 0, 5, 0, 0, 2]),
    ("memory-2-2", "env", [ENV_MEMORY, NONE, 0, 3, 0, 2, 2]),
    ("memory-4-4", "env", [ENV_MEMORY, LATENT, 6, 64, 0, 4, 4]),
    ("memory-4-3-visible", "env", [ENV_MEMORY, VISIBLE, 6, 9, 0, 4, 3]),
    ("memory-7-1", "env", [ENV_MEMORY, NONE, 0, 2, 0, 7, 1]),
    ("bandit-of-the-config", "env", [ENV_BANDIT, NONE, 0, 6, 0, 0, 0]),
    ("bandit-2-arms", "bandit", [ENV_BANDIT, NONE, 0, 6, 2]),
    ("bandit-8-arms", "bandit", [ENV_BANDIT, NONE, 5, 64, 8]),
    ("meta-2-arms", "meta", [NONE, 0, 8, 2, UNIFORM, 1]),
    ("meta-4-arms", "meta", [NONE, 7, 64, 4, ROUND_ROBIN, (1 << 32) - 1]),
    ("meta-wide-2-arms", "meta_wide", [NONE, 0, 8, 2, UNIFORM, 1]),
    ("meta-wide-4-arms", "meta_wide", [NONE, 7, 64, 4, ROUND_ROBIN, (1 << 32) - 1]),
    ("meta-wide-5-arms", "meta_wide", [NONE, 0, 3, 5, ONE_HOT, 10]),
    ("meta-wide-12-arms", "meta_wide", [NONE, 0, 64, 12, UNIFORM, 10]),
    ("mdp-2x2", "mdp", [NONE, 0, 1, 2, 2, 1.0, 0]),
    ("mdp-8x8", "mdp", [LATENT, 4, 64, 8, 8, 0.9, 5]),
    ("mdp-7-states-visible", "mdp", [VISIBLE, 4, 5, 7, 3, 1.0, 0]),
    # ------------------------------------------------------------------ accepted: feed-forward modules
    ("mlp-4-1-1", "mlp", [4, 1, 1]),
    ("mlp-5-128-2", "mlp", [5, 128, 2]),
    ("layers-5-128-2-is-fused", "mlp_layers", [5, 2, RELU, IDENTITY, 1, 128]),
    ("layers-4-1-1-is-fused", "mlp_config", [4, 1, RELU, IDENTITY, 1, 1, 1]),
    ("layers-5-129-2", "mlp_layers", [5, 2, RELU, IDENTITY, 1, 129]),
    ("layers-5-128-2-tanh", "mlp_layers", [5, 2, TANH, IDENTITY, 1, 128]),
    ("layers-5-128-3", "mlp_layers", [5, 3, RELU, IDENTITY, 1, 128]),
    ("layers-6-128-2", "mlp_layers", [6, 2, RELU, IDENTITY, 1, 128]),
    ("layers-no-hidden", "mlp_layers", [5, 2, RELU, IDENTITY, 0]),
    ("layers-1-to-1", "mlp_layers", [1, 1, IDENTITY, SIGMOID, 0]),
    ("layers-4-of-256", "mlp_layers", [8, 8, SIGMOID, TANH, 4, 256, 256, 256, 256]),
    ("layers-no-bias", "mlp_config", [5, 2, RELU, IDENTITY, 0, 1, 128]),
    ("layers-no-bias-3-layers", "mlp_config", [7, 1, TANH, IDENTITY, 0, 3, 9, 1, 31]),
    ("layers-bias-flag-7", "mlp_config", [5, 2, RELU, IDENTITY, 7, 2, 16, 16]),
    ("layers-8-outputs", "mlp_layers", [5, 8, RELU, IDENTITY, 1, 32]),
    # ------------------------------------------------------------------ accepted: recurrent chains
    ("gru-5-128-128-2", "gru_mlp", [5, 128, 128, 2]),
    ("lstm-5-128-128-1", "lstm_mlp", [5, 128, 128, 1]),
    ("lstm-5-32-32-2-twin", "lstm_mlp", [5, 32, 32, 2]),
    ("gru-4-128-128-2-twin", "gru_mlp", [4, 128, 128, 2]),
    ("gru-5-128-1-1-twin", "gru_mlp", [5, 128, 1, 1]),
    ("gru-6-128-128-2-lanes", "gru_mlp", [6, 128, 128, 2]),
    ("gru-8-256-256-2", "gru_mlp", [8, 256, 256, 2]),
    ("gru-5-129-128-2-lanes", "gru_mlp", [5, 129, 128, 2]),
    ("rnn-mlp-gru-5-128-128-2", "rnn_mlp", [GRU, 5, 128, 1, 128, 2]),
    ("rnn-mlp-2-layers", "rnn_mlp", [GRU, 5, 16, 2, 12, 2]),
    ("rnn-mlp-4-layers", "rnn_mlp", [LSTM, 5, 16, 4, 12, 1]),
    ("rnn-mlp-config-no-bias", "rnn_mlp_config", [GRU, 5, 128, 1, 0, 128, 2]),
    ("rnn-mlp-config-bias-flag-2", "rnn_mlp_config", [LSTM, 5, 32, 1, 2, 32, 2]),
    ("rnn-mlp-config-no-bias-3-layers", "rnn_mlp_config", [LSTM, 3, 7, 3, 0, 5, 2]),
    ("rnn-linear-5-128-2", "rnn_linear", [GRU, 5, 128, 1, 1, 2]),
    ("rnn-linear-no-bias-2-layers", "rnn_linear", [LSTM, 8, 256, 2, 0, 1]),
    ("chain-5-128-128-2", "chain", [GRU, 5, 128, 1, 1, 128, 2]),
    ("chain-5-32-32-2-twin", "chain", [LSTM, 5, 32, 1, 1, 32, 2]),
    ("chain-linear-tail", "chain", [GRU, 5, 128, 1, 1, 0, 2]),
    ("chain-8-outputs", "chain", [GRU, 5, 128, 1, 1, 128, 8]),
    ("chain-8-256-4-256-8", "chain", [LSTM, 8, 256, 4, 1, 256, 8]),
    ("chain-1-1-1-1-linear", "chain", [GRU, 1, 1, 1, 0, 0, 1]),
    ("chain-wide-5-128-128-2", "chain_wide", [GRU, 5, 128, 1, 1, 128, 2]),
    ("chain-wide-5-32-32-2-twin", "chain_wide", [LSTM, 5, 32, 1, 1, 32, 2]),
    ("chain-wide-8-outputs", "chain_wide", [GRU, 5, 128, 1, 1, 128, 8]),
    ("chain-wide-16-to-12", "chain_wide", [GRU, 16, 32, 1, 1, 0, 12]),
    ("chain-wide-9-to-1", "chain_wide", [LSTM, 9, 256, 4, 0, 256, 1]),
    ("chain-wide-1-to-9", "chain_wide", [GRU, 1, 8, 2, 1, 8, 9]),
]

# a wide constructor at a narrow shape builds what the narrow constructor builds: equal records
SAME_RECORD = [("meta-wide-2-arms", "meta-2-arms"), ("meta-wide-4-arms", "meta-4-arms"),
               ("chain-wide-5-128-128-2", "chain-5-128-128-2"), ("chain-wide-5-32-32-2-twin", "chain-5-32-32-2-twin"),
               ("chain-wide-8-outputs", "chain-8-outputs"), ("rnn-mlp-gru-5-128-128-2", "gru-5-128-128-2"),
               ("chain-5-128-128-2", "gru-5-128-128-2"), ("layers-5-128-2-is-fused", "mlp-5-128-2"),
               ("layers-4-1-1-is-fused", "mlp-4-1-1")]

# ---------------------------------------------------------------------- rl_rollout: one case per path and per refusal
# name -> (env case, module case, the path rollout_path names or None for a refusal).  Env and module are cases of the
# list above or of ROLLOUT_EXTRA; the GPU test rolls 64 lanes x 4 steps whatever n_lanes the case has.
ROLLOUT_EXTRA = [
    ("memory-3-3", "env", [ENV_MEMORY, NONE, 0, 64, 0, 3, 3]),
    ("bandit-3-arms", "bandit", [ENV_BANDIT, NONE, 0, 64, 3]),
    ("meta-3-arms", "meta", [NONE, 0, 64, 3, UNIFORM, 2]),
    ("mdp-5x3", "mdp", [NONE, 0, 64, 5, 3, 1.0, 0]),
    ("mdp-5x2", "mdp", [LATENT, 3, 64, 5, 2, 1.0, 0]),
    ("layers-32-32", "mlp_layers", [5, 2, RELU, IDENTITY, 2, 32, 32]),
    ("layers-6-32-3", "mlp_layers", [6, 3, RELU, IDENTITY, 1, 32]),
    ("layers-4-32-2", "mlp_layers", [4, 2, RELU, IDENTITY, 1, 32]),
    ("mlp-5-64-2", "mlp", [5, 64, 2]),
    ("gru-4-128-128-2", "gru_mlp", [4, 128, 128, 2]),
    ("gru-2-layers", "rnn_mlp", [GRU, 5, 16, 2, 12, 2]),
    ("chain-7-to-3", "chain", [GRU, 7, 16, 1, 1, 0, 3]),
    ("chain-5-to-3", "chain", [GRU, 5, 128, 1, 1, 128, 3]),
    ("gru-5-128-128-1", "gru_mlp", [5, 128, 128, 1]),
]
ROLLOUT_CASES = {
    "cartpole-mlp-5-128-2": ("cartpole-visible", "mlp-5-128-2", "ROLL_CARTPOLE"),
    "cartpole-4-mlp-4-32-2": ("cartpole-no-limit", "layers-4-32-2", "ROLL_CARTPOLE"),
    "chain-mlp-5-128-2": ("chain-default-size", "mlp-5-128-2", "ROLL_INDEX_MLP"),
    "memory-2-2-mlp-4-32-2": ("memory-2-2", "layers-4-32-2", "ROLL_GENERAL"),  # a fused shape off the five-state envs
    "cartpole-mlp-32-32": ("cartpole-visible", "layers-32-32", "ROLL_GENERAL"),
    "memory-3-3-mlp-6-32-3": ("memory-3-3", "layers-6-32-3", "ROLL_GENERAL"),
    "chain-gru-5-128-128-2": ("chain-default-size", "gru-5-128-128-2", "ROLL_TILE_RECURRENT"),
    "chain-lstm-5-32-32-2-twin": ("chain-default-size", "lstm-5-32-32-2-twin", "ROLL_TILE_RECURRENT"),
    "cartpole-gru-2-layers": ("cartpole-visible", "gru-2-layers", "ROLL_STACK"),
    "meta-chain-variant-0": ("meta-3-arms", "chain-7-to-3", "ROLL_STACK"),
    "meta-chain-variant-1": ("meta-3-arms", "chain-7-to-3", "ROLL_STACK"),
    "mdp-gru-5-128-128-2": ("mdp-5x2", "gru-5-128-128-2", "ROLL_STACK"),
    "mdp-mlp-5-64-2": ("mdp-5x2", "mlp-5-64-2", "ROLL_GENERAL"),
    "bandit-mlp-5-128-2": ("bandit-of-the-config", "mlp-5-128-2", "ROLL_INDEX_MLP"),
    # refusals
    "refused-memory-2-2-gru-4": ("memory-2-2", "gru-4-128-128-2", None),
    "refused-bandit-3-arms-two-output-chain": ("bandit-3-arms", "gru-5-128-128-2", None),
    "refused-cartpole-4-gru-4": ("cartpole-no-limit", "gru-4-128-128-2", None),
    "refused-out-dim": ("cartpole-visible", "gru-5-128-128-1", None),
    "refused-in-dim": ("cartpole-visible", "layers-4-32-2", None),
    "refused-mdp-3-actions-two-output-chain": ("mdp-5x3", "gru-5-128-128-2", None),
    "refused-order-two-output-chain-before-shape": ("bandit-3-arms", "gru-4-128-128-2", None),
}
ROLLOUT_VARIANT = {"meta-chain-variant-1": 1}


# ---------------------------------------------------------------------- initial parameter vectors, held to the oracle bit for bit
# name -> ("mlp", seed, in_dim, hidden_sizes, out_dim, bias, kernel_init, bias_init)
#       | ("chain", seed, cell, in_dim, hidden, num_layers, mlp_hidden (0: a Linear tail), out_dim, five initializers)
# Initializers as the oracle and the wrapper name them: (kind, scale, value).
INIT_DEFAULT = ("Uniform", "FanAvg", 0.0)
RNN_DEFAULT = (INIT_DEFAULT, ("Orthogonal", "FanAvg", 0.0), ("Zeros", "FanAvg", 0.0), INIT_DEFAULT, INIT_DEFAULT)
INIT_VECTORS = {
    "mlp-uniform": ("mlp", 3, 5, [7], 2, True, INIT_DEFAULT, INIT_DEFAULT),
    "mlp-uniform-fan-in-constant-variance": ("mlp", 4, 4, [3, 9], 1, True, ("Uniform", "FanIn", 0.0), ("Uniform", "Constant", 0.02)),
    "mlp-normal-odd-counts": ("mlp", 5, 5, [3], 1, True, ("Normal", "FanIn", 0.0), ("Normal", "FanOut", 0.0)),  # 15, 3, 3, 1
    "mlp-orthogonal-tall-and-wide": ("mlp", 6, 3, [8, 2], 4, True, ("Orthogonal", "FanAvg", 0.0), ("Constant", "Constant", 0.1)),
    "mlp-constant-and-zeros": ("mlp", 7, 5, [4], 2, True, ("Constant", "Constant", 0.25), ("Zeros", "FanAvg", 0.0)),
    "mlp-no-bias": ("mlp", 8, 5, [6, 4], 2, False, ("Normal", "FanAvg", 0.0), None),
    "mlp-no-hidden-layer": ("mlp", 9, 8, [], 8, True, ("Orthogonal", "FanIn", 0.0), ("Uniform", "FanOut", 0.0)),
    "chain-gru-default": ("chain", 10, GRU, 5, 8, 1, 6, 2, RNN_DEFAULT),
    "chain-lstm-2-layers": ("chain", 11, LSTM, 3, 4, 2, 5, 1, (("Normal", "FanIn", 0.0), ("Orthogonal", "FanAvg", 0.0),
                                                                 ("Constant", "Constant", 0.5), ("Uniform", "FanOut", 0.0),
                                                                 ("Zeros", "FanAvg", 0.0))),
    "chain-linear-tail": ("chain", 12, GRU, 6, 5, 1, 0, 3, RNN_DEFAULT),
    "chain-orthogonal-input-wide": ("chain", 13, GRU, 8, 2, 1, 3, 2, (("Orthogonal", "FanAvg", 0.0), ("Orthogonal", "FanAvg", 0.0),
                                                                       ("Normal", "Constant", 0.01), INIT_DEFAULT, INIT_DEFAULT)),
}
INIT_KINDS = ["Zeros", "Constant", "Uniform", "Normal", "Orthogonal"]
INIT_SCALES = ["Constant", "FanIn", "FanOut", "FanAvg"]


def _init_numbers(spec):
    kind, scale, value = spec if spec is not None else ("Zeros", "FanAvg", 0.0)  # (a module without bias vectors reads none)
    return [INIT_KINDS.index(kind), INIT_SCALES.index(scale), value]


def by_name():
    return {name: (ctor, nums) for name, ctor, nums in CASES + ROLLOUT_EXTRA}


def lines():
    """the list as the demo reads it: `case NAME CTOR NUMBERS..`, `rollout NAME ENV-CASE MODULE-CASE` and
    `initvec NAME mlp SEED in_dim out_dim bias n_hidden widths.. kernel_init bias_init` /
    `initvec NAME chain SEED cell in_dim hidden num_layers rnn_bias mlp_hidden out_dim` + five initializers, each as
    kind scale value"""
    out = ["case %s %s %s" % (name, ctor, " ".join(str(x) for x in nums)) for name, ctor, nums in CASES + ROLLOUT_EXTRA]
    out += ["rollout %s %s %s" % (name, env, mod) for name, (env, mod, _) in sorted(ROLLOUT_CASES.items())]
    for name, v in sorted(INIT_VECTORS.items()):
        if v[0] == "mlp":
            _, seed, in_dim, hidden, out_dim, bias, kinit, binit = v
            nums = [seed, in_dim, out_dim, int(bias), len(hidden)] + hidden + _init_numbers(kinit) + _init_numbers(binit)
        else:
            _, seed, cell, in_dim, H, layers, H2, out_dim, inits = v
            nums = [seed, cell, in_dim, H, layers, 1, H2, out_dim] + [x for i in inits for x in _init_numbers(i)]
        out.append("initvec %s %s %s" % (name, v[0], " ".join(str(x) for x in nums)))
    return out


if __name__ == "__main__":
    print("\n".join(lines()))
