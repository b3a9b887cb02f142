// abi_module.hip — extern "C" entry points of include/relearn_hip.h, part: modules (feed-forward and recurrent chains).
// What a constructor decides — shape, refusals, initial weights — is handle_spec.hpp; module_build here is what it allocates.
#include "abi_internal.hpp"

extern "C" {

// ---------------------------------------------------------------- constructors
// The allocating half of every module constructor (`shape` was decided and checked in handle_spec.hpp: nothing is refused
// from here on, only a HIP call can fail): the parameters, zeroed, in `owner`'s memory — the module's own, or that of the
// module a twin belongs to.
static std::unique_ptr<rl_mlp> module_alloc(rl_engine *e, const ModuleShape &shape, rl_mlp *owner) {
  std::unique_ptr<rl_mlp> m(new rl_mlp(e, shape));
  const size_t alloc = shape.alloc_floats();
  m->d_params = (owner ? owner : m.get())->mem.alloc<float>(alloc);
  RL_HIP_CHECK(hipMemsetAsync(m->d_params, 0, alloc * sizeof(float), e->stream));
  return m;
}

// `e` and `out` not NULL
static void module_build(rl_engine *e, const ModuleShape &shape, rl_mlp **out) {
  RL_HIP_CHECK(hipSetDevice(e->device));
  std::unique_ptr<rl_mlp> m = module_alloc(e, shape, nullptr);
  if (shape.needs_twin()) {
    m->exec = module_alloc(e, chain_twin_shape(shape), m.get()).release();  // every padding entry stays 0 for the life of the module
    m->x_tmp = m->mem.alloc<float>(m->exec->P);
    m->x_tan = m->mem.alloc<float>(m->exec->P);
    RL_HIP_CHECK(hipMemsetAsync(m->x_tan, 0, m->exec->P * sizeof(float), e->stream));
  }
  sync(e);
  e->live_handles += 1;
  *out = m.release();
}

int32_t rl_mlp_create(rl_engine *e, uint32_t in_dim, uint32_t hidden, uint32_t out_dim, rl_mlp **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && out, "NULL argument");
    *out = nullptr;
    module_build(e, fused_mlp_shape(in_dim, hidden, out_dim), out);
  });
}

int32_t rl_mlp_create_config(rl_engine *e, uint32_t in_dim, const uint32_t *hidden_sizes, uint32_t n_hidden,
                             uint32_t out_dim, int32_t activation, int32_t output_activation, int32_t bias, rl_mlp **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && out && (hidden_sizes || n_hidden == 0), "NULL argument");
    *out = nullptr;
    module_build(e, mlp_shape(in_dim, hidden_sizes, n_hidden, out_dim, activation, output_activation, bias != 0), out);
  });
}

int32_t rl_mlp_create_layers(rl_engine *e, uint32_t in_dim, const uint32_t *hidden_sizes, uint32_t n_hidden,
                             uint32_t out_dim, int32_t activation, int32_t output_activation, rl_mlp **out) {
  return rl_mlp_create_config(e, in_dim, hidden_sizes, n_hidden, out_dim, activation, output_activation, 1, out);
}

// Every recurrent constructor fills an rl_rnn_chain_config, names its limits (handle_spec.hpp, chain_shape) and ends here,
// inside its guarded call.  An unknown cell or flag is refused before a NULL handle is, then the shape.
static void chain_create(rl_engine *e, const rl_rnn_chain_config &cfg, const ChainLimits &lim, rl_mlp **out) {
  chain_kind(cfg);
  RL_REQUIRE(e && out, "NULL argument");
  *out = nullptr;
  module_build(e, chain_shape(cfg, lim), out);
}

// the module the recurrent kernels run (see rl_mlp::exec), its parameter image refreshed from the module's flat vector
rl_mlp *seq_exec(const rl_mlp *m) {
  if (m->exec == nullptr) return const_cast<rl_mlp *>(m);
  launch_seq_pad(m, m->exec->d_params, m->d_params);
  return m->exec;
}

int32_t rl_gru_mlp_create(rl_engine *e, uint32_t in_dim, uint32_t gru_hidden, uint32_t mlp_hidden, uint32_t out_dim,
                          rl_mlp **out) {
  return guarded(e, [&] {
    chain_create(e, {RL_CELL_GRU, in_dim, gru_hidden, 1, 1, mlp_hidden, out_dim}, CHAIN_TWO_ACTIONS_MLP, out);
  });
}

int32_t rl_lstm_mlp_create(rl_engine *e, uint32_t in_dim, uint32_t lstm_hidden, uint32_t mlp_hidden, uint32_t out_dim,
                           rl_mlp **out) {
  return guarded(e, [&] {
    chain_create(e, {RL_CELL_LSTM, in_dim, lstm_hidden, 1, 1, mlp_hidden, out_dim}, CHAIN_TWO_ACTIONS_MLP, out);
  });
}

int32_t rl_rnn_mlp_create(rl_engine *e, int32_t cell, uint32_t in_dim, uint32_t hidden_size, uint32_t num_layers,
                          uint32_t mlp_hidden, uint32_t out_dim, rl_mlp **out) {
  return guarded(e, [&] {
    chain_create(e, {cell, in_dim, hidden_size, num_layers, 1, mlp_hidden, out_dim}, CHAIN_TWO_ACTIONS_MLP, out);
  });
}

// (`bias`: any non-zero value builds the bias vectors — the one constructor that does not hold the flag to 0 or 1, as
// rl_rnn_linear_create and the two rl_rnn_chain_create do through chain_kind)
int32_t rl_rnn_mlp_create_config(rl_engine *e, int32_t cell, uint32_t in_dim, uint32_t hidden_size, uint32_t num_layers,
                                 int32_t bias, uint32_t mlp_hidden, uint32_t out_dim, rl_mlp **out) {
  return guarded(e, [&] {
    chain_create(e, {cell, in_dim, hidden_size, num_layers, bias != 0, mlp_hidden, out_dim}, CHAIN_TWO_ACTIONS_MLP, out);
  });
}

int32_t rl_rnn_linear_create(rl_engine *e, int32_t cell, uint32_t in_dim, uint32_t hidden_size, uint32_t num_layers,
                             int32_t rnn_bias, uint32_t out_dim, rl_mlp **out) {
  return guarded(e, [&] {
    chain_create(e, {cell, in_dim, hidden_size, num_layers, rnn_bias, 0, out_dim}, CHAIN_TWO_ACTIONS_LINEAR, out);
  });
}

// ChainConfig<GruConfig | LstmConfig, MlpConfig | LinearConfig>::build_module in one statement (modules/chain.rs:12-56,
// seq/rnn/mod.rs:20-45,223-281): the constructors above are its two-action shorthand and build the same handle for
// out_dim <= 2; out_dim 3..8 — a categorical policy over IndexSpace::new(3..8) — always runs the lane-per-thread kernels
// (ModuleShape::lane_kernels), never a twin.
int32_t rl_rnn_chain_config_default(int32_t cell, rl_rnn_chain_config *cfg) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(cfg, "cfg is NULL");
    if (cell != RL_CELL_GRU && cell != RL_CELL_LSTM) throw RlError(RL_ERR_BUILD_AGENT, "unknown recurrent cell");
    // RnnBaseConfig::default (seq/rnn/mod.rs:28-45): hidden_size 128, num_layers 1, bias vectors; ChainConfig::default
    // (modules/chain.rs:19-33) over MlpConfig::default (ff/mlp.rs:24-34): one hidden layer of 128
    cfg->cell = cell;
    cfg->in_dim = 5;
    cfg->hidden = 128;
    cfg->num_layers = 1;
    cfg->rnn_bias = 1;
    cfg->mlp_hidden = 128;
    cfg->out_dim = 2;
  });
}

int32_t rl_rnn_chain_create(rl_engine *e, const rl_rnn_chain_config *cfg, rl_mlp **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && cfg && out, "NULL argument");
    *out = nullptr;
    chain_create(e, *cfg, CHAIN_NARROW, out);
  });
}

// The same chain at in_dim 1..16 and out_dim 1..12 (the RL2 experiment's model on up to 12 arms: k + 4 inputs, k outputs
// for the policy, one for the critic).  Within in_dim <= 8 and out_dim <= 8: rl_rnn_chain_create, the same handle.
// Beyond, always the lane-per-thread kernels (ModuleShape::lane_kernels: in_dim > 5 or out_dim > 2), never a twin.
int32_t rl_rnn_chain_create_wide(rl_engine *e, const rl_rnn_chain_config *cfg, rl_mlp **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && cfg && out, "NULL argument");
    *out = nullptr;
    chain_create(e, *cfg, chain_limits_wide(*cfg), out);
  });
}

// The same chain at in_dim 1..20 (the RL2 MDP experiment's model on 10 x 5 lanes: 19 inputs, five outputs for the policy,
// one for the critic).  At in_dim <= 16: rl_rnn_chain_create_wide, the same handle.  The lane-per-thread kernels take the
// input width at run time (StackNet::D): no kernel is built for these modules that the narrower ones do not run.
int32_t rl_rnn_chain_create_wide20(rl_engine *e, const rl_rnn_chain_config *cfg, rl_mlp **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && cfg && out, "NULL argument");
    *out = nullptr;
    chain_create(e, *cfg, chain_limits_wide20(*cfg), out);
  });
}

// The same chain at in_dim 1..24 (the partition-game experiment's model: 24 inputs under the visible limit, two outputs
// for the policy, one for the critic).  At in_dim <= 20: rl_rnn_chain_create_wide20, the same handle.  As there, no
// kernel is built for these modules: the lane-per-thread kernels take the input width at run time.
int32_t rl_rnn_chain_create_wide24(rl_engine *e, const rl_rnn_chain_config *cfg, rl_mlp **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && cfg && out, "NULL argument");
    *out = nullptr;
    chain_create(e, *cfg, chain_limits_wide24(*cfg), out);
  });
}

int32_t rl_mlp_destroy(rl_mlp *m) { return destroy_child(m); }

int32_t rl_mlp_num_params(const rl_mlp *m, uint64_t *n) {
  return guarded(m ? m->eng : nullptr, [&] {
    RL_REQUIRE(m && n, "NULL argument");
    *n = m->P;
  });
}

// ---------------------------------------------------------------- parameters
// the module's flat vector from the host ([P]), and with it the end of whatever was derived from the old one
static void module_upload(rl_mlp *m, const float *host) {
  h2d(m->eng, m->d_params, host, m->P * sizeof(float));
  wimg_invalidate(m);  // (the parameters changed under the module's weight image, bf16_tile.hpp)
}

int32_t rl_mlp_init(rl_mlp *m, uint64_t seed) {
  return guarded(m ? m->eng : nullptr, [&] {
    RL_REQUIRE(m, "mlp is NULL");
    const std::vector<float> h = rl_module_is_recurrent(m->kind) ? chain_init_vector(*m, seed, rnn_default_inits())
                                                                 : mlp_init_vector(*m, seed, {GLOROT_UNIFORM, GLOROT_UNIFORM});
    module_upload(m, h.data());
  });
}

int32_t rl_mlp_init_with(rl_mlp *m, uint64_t seed, const rl_initializer *kernel_init, const rl_initializer *bias_init) {
  return guarded(m ? m->eng : nullptr, [&] {
    RL_REQUIRE(m && kernel_init, "NULL argument");
    const std::vector<float> h = mlp_init_vector(*m, seed, mlp_inits_checked(*m, kernel_init, bias_init));
    module_upload(m, h.data());
  });
}

int32_t rl_rnn_mlp_init_with(rl_mlp *m, uint64_t seed, const rl_initializer *input_weights_init,
                             const rl_initializer *hidden_weights_init, const rl_initializer *bias_init,
                             const rl_initializer *mlp_kernel_init, const rl_initializer *mlp_bias_init) {
  return guarded(m ? m->eng : nullptr, [&] {
    RL_REQUIRE(m, "module is NULL");
    const RnnInits inits = chain_inits_checked(*m, input_weights_init, hidden_weights_init, bias_init, mlp_kernel_init, mlp_bias_init);
    const std::vector<float> h = chain_init_vector(*m, seed, inits);
    module_upload(m, h.data());
  });
}

int32_t rl_params_get(rl_mlp *m, float *host, uint64_t n) {
  return guarded(m ? m->eng : nullptr, [&] {
    RL_REQUIRE(m && host, "NULL argument");
    RL_REQUIRE(n == m->P, "parameter count mismatch");
    d2h(m->eng, host, m->d_params, n * sizeof(float));
  });
}

int32_t rl_params_set(rl_mlp *m, const float *host, uint64_t n) {
  return guarded(m ? m->eng : nullptr, [&] {
    RL_REQUIRE(m && host, "NULL argument");
    RL_REQUIRE(n == m->P, "parameter count mismatch");
    module_upload(m, host);
  });
}

int32_t rl_mlp_forward(rl_mlp *m, const float *rows, uint64_t n_rows, float *out) {
  return guarded(m ? m->eng : nullptr, [&] {
    if (m && m->kind != RL_MODULE_MLP)
      throw RlError(RL_ERR_UNSUPPORTED, "row-wise forward is for feed-forward modules; use rl_seq_forward");
    RL_REQUIRE(m && rows && out, "NULL argument");
    if (n_rows == 0) return;
    rl_engine *e = m->eng;
    std::vector<float> soa((size_t)n_rows * m->in_dim), res((size_t)n_rows * m->out_dim);
    for (uint64_t r = 0; r < n_rows; ++r)
      for (uint32_t d = 0; d < m->in_dim; ++d) soa[(size_t)d * n_rows + r] = rows[r * m->in_dim + d];
    DevMem tmp;
    float *d_in = tmp.alloc<float>(soa.size()), *d_out = tmp.alloc<float>(res.size());
    h2d(e, d_in, soa.data(), soa.size() * sizeof(float));
    if (m->general) {
      rl_traj scratch{};  // (only the workspace of the per-layer kernels is used; it goes with scratch.mem)
      scratch.eng = e;
      launch_gen_forward(&scratch, m, d_in, n_rows, n_rows, d_out);
      sync(e);
    } else {
      launch_mlp_forward_host_rows(m, d_in, n_rows, d_out);
    }
    d2h(e, res.data(), d_out, res.size() * sizeof(float));
    for (uint64_t r = 0; r < n_rows; ++r)
      for (uint32_t a = 0; a < m->out_dim; ++a) out[r * m->out_dim + a] = res[(size_t)a * n_rows + r];
  });
}

}  // extern "C"
