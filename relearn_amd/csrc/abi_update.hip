// abi_update.hip — extern "C" entry points of include/relearn_hip.h, part: advantages and policy / critic updates (GAE, TRPO, PPO, REINFORCE, value fitting) (host side only; kernels live in kernels_*.hip).
#include "abi_internal.hpp"

// ---------------------------------------------------------------- one gradient / evaluation pass
// Every update entry point is made of these: choose the kernel family of the module, enqueue forward, backward and slab
// reduction, all-reduce the slice of traj->vec the pass produced.  What differs between the passes is this table:
//   backward  there is one, and it leaves the gradient: slab A is reduced (feed-forward) and vec[0..P) all-reduced
//   sums      the pass leaves per-sample sums: slab B is reduced and vec[P..P+4) all-reduced
//   fused     the single-launch form to try first (feed-forward modules, kernel variant 0); its range guard's chain
enum FusedLauncher { FUSED_NONE, FUSED_POLICY /* launch_policy_v2, RL_GUARD_POLICY */,
                     FUSED_CRITIC /* launch_critic_step_v2, RL_GUARD_CRITIC */ };
struct PassRow {
  bool backward, sums;
  FusedLauncher fused;
};
static const PassRow PASS_TABLE[RUN_KINDS] = {
    /* RUN_INIT   */ {true, true, FUSED_POLICY},
    /* RUN_EVAL   */ {false, true, FUSED_POLICY},
    /* RUN_JVP    */ {true, false, FUSED_POLICY},
    /* RUN_DQN    */ {true, true, FUSED_NONE},  // (abi_dqn.hip has tried the DQN step kernels before it asks)
    /* RUN_PPO    */ {true, true, FUSED_POLICY},
    /* RUN_CRITIC */ {true, true, FUSED_CRITIC},
};
// (the rows are positional: the kinds alias PolicyPassMode, kernels.hpp)
static_assert(RUN_INIT == 0 && RUN_EVAL == 1 && RUN_JVP == 2 && RUN_DQN == 3 && RUN_PPO == 4 && RUN_CRITIC == 5 &&
                  RUN_KINDS == 6,
              "PASS_TABLE rows are in the order of PassKind");

// a recurrent gradient comes back in the layout of the module the kernels ran (its zero-padded twin, SeqScope) and is
// gathered into the module's flat order before anything else touches the vector
static void seq_gradient_to_flat_order(const rl_mlp *mod, rl_traj *traj) {
  if (mod->exec == nullptr) return;
  launch_seq_unpad(mod, traj->vec, mod->x_tmp);
  RL_HIP_CHECK(hipMemcpyAsync(traj->vec, mod->x_tmp, mod->P * sizeof(float), hipMemcpyDeviceToDevice, traj->eng->stream));
}

// where a training forward of `mod` keeps its activation record (non-NULL asks the forward for one)
static float *seq_record(rl_traj *traj, const rl_mlp *mod) {
  return mod->lane_kernels() ? traj->seq.stack.rec : traj->seq.act;
}

SlabRows run_pass(const rl_mlp *mod, rl_traj *traj, const PassRequest &req) {
  const PassRow &row = PASS_TABLE[req.kind];
  const bool critic = req.kind == RUN_CRITIC;
  const uint32_t P = (uint32_t)mod->P;
  const uint64_t Bt = req.B_total ? req.B_total : b_total(traj);
  bool grad = row.backward;
  auto allreduce = [&] {
    rl_allreduce_sum_f32(traj->eng, traj->vec + (grad ? 0 : P), (grad ? P : 0) + (row.sums ? 4 : 0));
  };
  if (rl_module_is_recurrent(mod->kind)) {
    // teacher-forced forward (activation record) -> d loss / d outputs -> [backward through time -> weight gradients]
    // -> vec[0..P), and the per-sample sums through slab B.  A Fisher-vector product starts from the record of the last
    // pass with a backward instead: vec[0..P) <- J^T (diag(p) - p p^T) J v / B
    RL_REQUIRE(req.reduce, "a recurrent pass reduces its own sums");  // (its gradient never goes through the slabs)
    grad = row.backward && !req.forward_only;
    SeqScope sc(traj, mod);
    seq_ensure(traj, sc.x, true);
    if (req.kind == RUN_JVP) {
      const float *tangent = req.tangent;
      if (mod->exec != nullptr) {  // the tangent in the twin's layout (its padding entries stay zero)
        launch_seq_pad(mod, mod->x_tan, req.tangent);
        tangent = mod->x_tan;
      }
      launch_gru_tangent(traj, sc.x, tangent, Bt, req.skip);
    } else {
      // The record is asked for wherever the pass kind has a backward, also when this request stops before it
      // (forward_only): with a record the tile kernels run the bf16-pipe training forward, without one the f32 forward
      // (launch_gru_seq_forward), and the two round differently.  rl_ppo_update's log pi_0 must come from the forward
      // its steps recompute log pi with: then the first step's ratios are exactly 1, as the reference's are — off by
      // an ulp they are clipped samples at clip_distance = 0.
      launch_gru_seq_forward(traj, sc.x, traj->seq.out, nullptr, row.backward ? seq_record(traj, sc.x) : nullptr,
                             req.skip);
      if (critic) launch_seq_critic_dvalues(traj, Bt);
      else launch_seq_policy_dlogits(traj, req.kind, Bt, req.clip_lo, req.clip_hi, req.skip, sc.x->out_dim);
    }
    if (grad) {
      launch_gru_backward(traj, sc.x, req.skip);
      seq_gradient_to_flat_order(mod, traj);
    }
    if (row.sums) launch_reduce(traj, P, false, true, 0, traj->nbB);
    allreduce();
    return SlabRows{0, traj->nbB};
  }
  // feed-forward: the fused single launch where a kernel is built for the shape (the launcher says), else forward,
  // backward, and the slab rows of those two
  bool fused = false;
  if (traj->eng->kernel_variant == 0) {  // (1: the v1 reference kernels only)
    if (row.fused == FUSED_POLICY)
      fused = launch_policy_v2(traj, mod, req.kind, req.tangent, Bt, req.skip, req.clip_lo, req.clip_hi, req.keep);
    else if (row.fused == FUSED_CRITIC)
      fused = launch_critic_step_v2(traj, mod, Bt);
  }
  if (!fused) {
    if (critic) launch_critic_fwd(traj, mod, Bt);
    else launch_policy_pass(traj, mod, req.kind, req.tangent, Bt, req.skip, req.clip_lo, req.clip_hi);
    if (row.backward) launch_mlp_backward(traj, mod, req.skip);
  }
  const SlabRows rows = fused ? SlabRows{traj->last_rows, traj->last_rows} : SlabRows{traj->nbA, traj->nbB};
  if (req.reduce) {
    launch_reduce(traj, P, row.backward, row.sums, rows.A, rows.B);
    allreduce();
  }
  return rows;
}

extern "C" {

// ---------------------------------------------------------------- TRPO
int32_t rl_trpo_config_default(rl_trpo_config *c) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(c, "cfg is NULL");
    // ConjugateGradientOptimizerConfig::default (conjugate_gradient.rs:55-65), TrpoConfig::default (trpo.rs:29-41)
    c->iterations = 10;
    c->max_backtracks = 15;
    c->backtrack_ratio = 0.8;
    c->hpv_reg_coeff = 1e-5;
    c->max_policy_step_kl = 0.01;
    c->accept_violation = 0;
  });
}

static void check_policy(const rl_mlp *policy, const rl_traj *traj) {
  RL_REQUIRE(policy && traj, "NULL argument");
  RL_REQUIRE(policy->eng == traj->eng, "handles belong to different engines");
  RL_REQUIRE(policy->in_dim == traj->d.D && policy->out_dim >= 2, "policy shape does not match the trajectory");
  // the action space of the recorded steps: the env's of the rollout that wrote them, or — a host-written action plane —
  // at least the largest index it holds
  RL_REQUIRE(traj->n_actions == 0 || policy->out_dim == traj->n_actions,
             "policy outputs do not match the action count of the env this trajectory was collected on");
  RL_REQUIRE(policy->out_dim > traj->max_action, "the trajectory holds an action index the policy has no output for");
  // (a recurrent chain of more than two outputs runs the lane-per-thread kernels: rl_rnn_chain_create)
  if (policy->out_dim > 2 && policy->kind != RL_MODULE_MLP && !policy->lane_kernels())
    throw RlError(RL_ERR_UNSUPPORTED, "the recurrent tile kernels are built for two actions");
}

// Trpo::update (trpo.rs:97-164) on the engine's current stream, in two halves.  The head enqueues everything up to and
// including the first two line-search candidates — about fifty launches without a host round trip; the tail reads the
// acceptance flag back every second candidate and collects the statistics.  (rl_actor_critic_update enqueues the other
// chain's launches between the two: the host is then never the reason one chain's kernels start late.)
static inline void trpo_candidate(rl_mlp *policy, rl_traj *traj, const rl_trpo_config *cfg, uint64_t i, double ratio) {
  launch_ls_set_params(traj, policy, ratio);
  PassRequest eval(RUN_EVAL);
  eval.skip = &traj->trpo->ls_accepted;
  run_pass(policy, traj, eval);
  launch_ls_check(traj, (uint32_t)policy->P, b_total(traj), (int)i, ratio, cfg->max_policy_step_kl);
}

struct TrpoProgress {
  uint64_t next = 0;   // line-search candidates [0, next) are enqueued
  double ratio = 1.0;  // backtrack_ratio.powi(next - 1)
};

static TrpoProgress trpo_update_head(rl_mlp *policy, rl_traj *traj, const rl_trpo_config *cfg) {
  uint32_t P = (uint32_t)policy->P;
  uint64_t Bt = b_total(traj);
  float reg = (float)cfg->hpv_reg_coeff;
  // loss gradient at theta0 (its relu' masks and Fisher weights kept for the products of the solve: the parameters do
  // not move before the line search) and CG prologue
  PassRequest init(RUN_INIT);
  init.keep = true;
  run_pass(policy, traj, init);
  launch_trpo_begin(traj, policy, Bt);
  // x = A^-1 g by `iterations` CG steps (early exit handled on the device)
  PassRequest fvp(RUN_JVP);
  fvp.tangent = traj->cg_p;
  fvp.skip = &traj->trpo->cg_done;
  for (uint64_t it = 0; it < cfg->iterations; ++it) {
    run_pass(policy, traj, fvp);
    launch_cg_step(traj, P, reg, 1e-10f);
  }
  launch_cg_finish(traj, P);
  // step size from x^T A x
  fvp.tangent = traj->cg_x;
  fvp.skip = nullptr;
  run_pass(policy, traj, fvp);
  launch_step_size(traj, policy, reg, cfg->max_policy_step_kl);
  // backtracking line search: the first two candidates
  TrpoProgress pr;
  for (; pr.next < cfg->max_backtracks && pr.next < 2; ++pr.next) {
    if (pr.next > 0) pr.ratio *= cfg->backtrack_ratio;  // backtrack_ratio.powi(i)
    trpo_candidate(policy, traj, cfg, pr.next, pr.ratio);
  }
  return pr;
}

static void trpo_update_tail(rl_mlp *policy, rl_traj *traj, const rl_trpo_config *cfg, TrpoProgress pr,
                             rl_trpo_stats *stats) {
  rl_engine *e = traj->eng;
  double ratio = pr.ratio;
  for (uint64_t i = pr.next; i < cfg->max_backtracks; ++i) {
    // once a candidate is accepted the remaining iterations are no-ops on the device (every launch tests the flag);
    // reading the flag back every second candidate spares their launches — and, with several ranks, their
    // all-reduces.  Replicas are identical, so every rank leaves the loop at the same iteration.
    if ((i & 1) == 0) {
      int32_t accepted = 0;
      d2h(e, &accepted, &traj->trpo->ls_accepted, sizeof(accepted));
      if (accepted != 0) break;
    }
    ratio *= cfg->backtrack_ratio;
    trpo_candidate(policy, traj, cfg, i, ratio);
  }
  launch_ls_finalize(traj, policy, cfg->max_policy_step_kl, cfg->accept_violation);
  TrpoStateDev h;
  d2h(e, &h, traj->trpo, sizeof(h));
  ipc_check(e);
  range_check(traj, 1u << RL_GUARD_POLICY);
  stats->entropy = (double)h.entropy;
  stats->step_size = h.step_size;
  stats->loss_initial = (double)h.loss0;
  stats->loss_final = (double)h.ls_loss;
  stats->constraint_val_final = (double)h.ls_kl;
  stats->step_scale = h.ls_accepted ? h.ls_ratio : 0.0;
  stats->num_backtracks = h.ls_accepted ? (int64_t)h.ls_index : -1;
  stats->status = h.status;
  stats->cg_iterations = h.cg_iters;
}

static void trpo_update_impl(rl_mlp *policy, rl_traj *traj, const rl_trpo_config *cfg, rl_trpo_stats *stats) {
  trpo_update_tail(policy, traj, cfg, trpo_update_head(policy, traj, cfg), stats);
}

static void trpo_raise_nan(const rl_trpo_stats *stats) {
  if (stats->status == RL_OPT_NAN_LOSS || stats->status == RL_OPT_NAN_CONSTRAINT)
    throw RlError(RL_ERR_OPT_NAN, stats->status == RL_OPT_NAN_LOSS ? "NaN loss in policy optimization"
                                                                   : "NaN constraint in policy optimization");
}

int32_t rl_trpo_update(rl_mlp *policy, rl_traj *traj, const rl_trpo_config *cfg, rl_trpo_stats *stats) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    check_policy(policy, traj);
    RL_REQUIRE(cfg && stats, "NULL argument");
    trpo_update_impl(policy, traj, cfg, stats);
    trpo_raise_nan(stats);
  });
}

int32_t rl_policy_gradient(rl_mlp *policy, rl_traj *traj, float *grad_out, float *loss_out, float *entropy_out) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    check_policy(policy, traj);
    RL_REQUIRE(grad_out, "grad_out is NULL");
    uint32_t P = (uint32_t)policy->P;
    run_pass(policy, traj, RUN_INIT);
    std::vector<float> h(P + 4);
    d2h(traj->eng, h.data(), traj->vec, (P + 4) * sizeof(float));
    range_check(traj, 1u << RL_GUARD_POLICY);
    std::memcpy(grad_out, h.data(), P * sizeof(float));
    double inv_B = 1.0 / (double)b_total(traj);
    if (loss_out) *loss_out = (float)(-((double)h[P] * inv_B));
    if (entropy_out) *entropy_out = (float)((double)h[P + 1] * inv_B);
  });
}

int32_t rl_policy_fvp(rl_mlp *policy, rl_traj *traj, const float *v, float reg, float *out) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    check_policy(policy, traj);
    RL_REQUIRE(v && out, "NULL argument");
    uint32_t P = (uint32_t)policy->P;
    PassRequest init(RUN_INIT);  // the product is taken at the current parameters: refresh log pi_0, keep the masks
    init.keep = true;
    run_pass(policy, traj, init);
    h2d(traj->eng, traj->cg_x, v, P * sizeof(float));  // (the recurrent pass above has grown the workspace)
    PassRequest fvp(RUN_JVP);
    fvp.tangent = traj->cg_x;
    run_pass(policy, traj, fvp);
    std::vector<float> h(P);
    d2h(traj->eng, h.data(), traj->vec, P * sizeof(float));
    range_check(traj, 1u << RL_GUARD_POLICY);
    for (uint32_t i = 0; i < P; ++i) out[i] = h[i] + reg * v[i];
  });
}

int32_t rl_policy_loss_kl(rl_mlp *policy, rl_traj *traj, const float *params0, float *loss_out, float *kl_out) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    check_policy(policy, traj);
    RL_REQUIRE(params0 && loss_out && kl_out, "NULL argument");
    rl_engine *e = traj->eng;
    uint32_t P = (uint32_t)policy->P;
    uint64_t Bt = b_total(traj);
    // lp0 under params0, then evaluate the current parameters against it
    std::vector<float> cur(P);
    d2h(e, cur.data(), policy->d_params, P * sizeof(float));
    h2d(e, policy->d_params, params0, P * sizeof(float));
    wimg_invalidate(policy);  // (the parameters changed under the module's weight image, bf16_tile.hpp)
    run_pass(policy, traj, RUN_INIT);  // fills lp0 under params0
    h2d(e, policy->d_params, cur.data(), P * sizeof(float));
    wimg_invalidate(policy);  // (the parameters changed under the module's weight image, bf16_tile.hpp)
    run_pass(policy, traj, RUN_EVAL);
    float h[4];
    d2h(e, h, traj->vec + P, sizeof(h));
    range_check(traj, 1u << RL_GUARD_POLICY);
    double inv_B = 1.0 / (double)Bt;
    *loss_out = (float)(-((double)h[0] * inv_B));
    *kl_out = (float)((double)h[1] * inv_B);
  });
}

// ---------------------------------------------------------------- critic
int32_t rl_adam_config_default(rl_adam_config *c) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(c, "cfg is NULL");
    c->learning_rate = 1e-3;  // AdamConfig::default (coptimizer.rs:147-156)
    c->beta1 = 0.9;
    c->beta2 = 0.999;
    c->weight_decay = 0.0;
    c->eps = 1e-8;  // libtorch AdamOptions default
  });
}

// SgdConfig / RmsPropConfig / AdamConfig / AdamWConfig::default (coptimizer.rs:64-74, 107-118, 147-156, 184-193)
static void optimizer_config_default(int32_t kind, rl_optimizer_config *c) {
  std::memset(c, 0, sizeof(*c));
  c->kind = kind;
  c->eps = 1e-8;  // libtorch AdamOptions / AdamWOptions default; RmsPropConfig::default
  if (kind == RL_OPTIMIZER_ADAM || kind == RL_OPTIMIZER_ADAMW) {
    c->learning_rate = 1e-3;
    c->beta1 = 0.9;
    c->beta2 = 0.999;
  } else if (kind == RL_OPTIMIZER_SGD) {
    c->learning_rate = 1e-2;
  } else if (kind == RL_OPTIMIZER_RMSPROP) {
    c->learning_rate = 1e-2;
    c->alpha = 0.99;
  } else {
    throw RlError(RL_ERR_INVALID_ARGUMENT, "optimizer config: unknown kind");
  }
}

int32_t rl_optimizer_config_default(int32_t kind, rl_optimizer_config *c) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(c, "cfg is NULL");
    optimizer_config_default(kind, c);
  });
}

// what libtorch's option checks reject (torch/csrc/api/src/optim/{sgd,rmsprop,adam,adamw}.cpp of 1.12, third party); a
// NaN fails every one of these comparisons and is rejected with them
static void optimizer_config_check(const rl_optimizer_config &c) {
  const int32_t k = c.kind;
  RL_REQUIRE(k == RL_OPTIMIZER_ADAM || k == RL_OPTIMIZER_ADAMW || k == RL_OPTIMIZER_SGD || k == RL_OPTIMIZER_RMSPROP,
             "optimizer config: unknown kind");
  RL_REQUIRE(c.learning_rate >= 0.0, "optimizer config: invalid learning_rate (negative)");
  RL_REQUIRE(c.weight_decay >= 0.0, "optimizer config: invalid weight_decay (negative)");
  if (k == RL_OPTIMIZER_ADAM || k == RL_OPTIMIZER_ADAMW) {
    RL_REQUIRE(c.eps >= 0.0, "optimizer config: invalid eps (negative)");
    RL_REQUIRE(c.beta1 >= 0.0 && c.beta1 < 1.0, "optimizer config: invalid beta1 (outside [0, 1))");
    RL_REQUIRE(c.beta2 >= 0.0 && c.beta2 < 1.0, "optimizer config: invalid beta2 (outside [0, 1))");
  } else if (k == RL_OPTIMIZER_SGD) {
    RL_REQUIRE(c.momentum >= 0.0, "optimizer config: invalid momentum (negative)");
    RL_REQUIRE(!c.nesterov || (c.momentum > 0.0 && c.dampening == 0.0),
               "optimizer config: nesterov requires a momentum > 0 and zero dampening");
  } else {
    RL_REQUIRE(c.eps >= 0.0, "optimizer config: invalid eps (negative)");
    RL_REQUIRE(c.momentum >= 0.0, "optimizer config: invalid momentum (negative)");
    RL_REQUIRE(c.alpha >= 0.0, "optimizer config: invalid alpha (negative)");
  }
}

// which state slots a configuration has (kernels_update.hip opt_has_slot says the same from the step's flags)
static bool optimizer_has_slot(const rl_optimizer_config &c, int slot) {
  if (c.kind == RL_OPTIMIZER_ADAM || c.kind == RL_OPTIMIZER_ADAMW) return slot < 2;
  if (c.kind == RL_OPTIMIZER_SGD) return slot == 0 && c.momentum != 0.0;
  return slot == 0 || (slot == 1 && c.momentum > 0.0) || (slot == 2 && c.centered != 0);
}

static void optimizer_create(rl_mlp *module, const rl_optimizer_config &cfg, rl_adam **out) {
  rl_engine *e = module->eng;
  RL_HIP_CHECK(hipSetDevice(e->device));
  std::unique_ptr<rl_adam> o(new rl_adam());
  o->eng = e;
  o->mod = module;
  o->cfg = cfg;
  o->error_epoch = e->error_epoch;
  for (int s = 0; s < 3; ++s)
    if (optimizer_has_slot(cfg, s)) {
      o->d_state[s] = o->mem.alloc<float>(module->P);
      RL_HIP_CHECK(hipMemsetAsync(o->d_state[s], 0, module->P * sizeof(float), e->stream));
    }
  o->d_step = o->mem.alloc<uint64_t>(1);
  RL_HIP_CHECK(hipMemsetAsync(o->d_step, 0, sizeof(uint64_t), e->stream));
  sync(e);
  e->live_handles += 1;
  *out = o.release();
}

int32_t rl_adam_create(rl_mlp *module, const rl_adam_config *cfg, rl_adam **out) {
  return guarded(module ? module->eng : nullptr, [&] {
    RL_REQUIRE(module && cfg && out, "NULL argument");
    *out = nullptr;
    rl_optimizer_config c;  // (the fields as given: this entry point has never checked them)
    optimizer_config_default(RL_OPTIMIZER_ADAM, &c);
    c.learning_rate = cfg->learning_rate;
    c.beta1 = cfg->beta1;
    c.beta2 = cfg->beta2;
    c.weight_decay = cfg->weight_decay;
    c.eps = cfg->eps;
    optimizer_create(module, c, out);
  });
}

int32_t rl_optimizer_create(rl_mlp *module, const rl_optimizer_config *cfg, rl_adam **out) {
  return guarded(module ? module->eng : nullptr, [&] {
    RL_REQUIRE(cfg, "cfg is NULL");
    optimizer_config_check(*cfg);  // before the module is looked at
    RL_REQUIRE(module && out, "NULL argument");
    *out = nullptr;
    optimizer_create(module, *cfg, out);
  });
}

int32_t rl_adam_destroy(rl_adam *o) { return destroy_child(o); }

int32_t rl_optimizer_step_host(rl_adam *o, const float *grad) {
  return guarded(o ? o->mod->eng : nullptr, [&] {
    RL_REQUIRE(o && grad, "NULL argument");
    rl_engine *e = o->mod->eng;
    DevMem tmp;
    float *d_g = tmp.alloc<float>(o->mod->P);
    h2d(e, d_g, grad, o->mod->P * sizeof(float));
    launch_opt_step_vec(o, d_g);
    sync(e);
  });
}

int32_t rl_adam_step_host(rl_adam *o, const float *grad) { return rl_optimizer_step_host(o, grad); }

int32_t rl_optimizer_state_read(rl_adam *o, int32_t slot, float *host, uint64_t n, uint64_t *step_out) {
  return guarded(o ? o->eng : nullptr, [&] {
    RL_REQUIRE(o, "NULL argument");
    RL_REQUIRE(host == nullptr || (slot >= 0 && slot < 3 && o->d_state[slot] != nullptr),
               "optimizer state: the rule has no such slot");
    RL_REQUIRE(host == nullptr || n == o->mod->P, "optimizer state: n is not the module's parameter count");
    if (host) d2h(o->eng, host, o->d_state[slot], n * sizeof(float));
    if (step_out) d2h(o->eng, step_out, o->d_step, sizeof(uint64_t));
  });
}

static void check_critic(const rl_mlp *critic, const rl_traj *traj) {
  RL_REQUIRE(critic && traj, "NULL argument");
  RL_REQUIRE(critic->eng == traj->eng, "handles belong to different engines");
  RL_REQUIRE(critic->in_dim == traj->d.D && critic->out_dim == 1, "critic shape does not match the trajectory");
}

// n_backward_steps (src/torch/agents/mod.rs:35-72) of full-batch MSE against traj->d.tgt with Adam: the launches, on the
// engine's current stream, without any host synchronisation (feed-forward modules on a device-side collective)
static void critic_enqueue_steps(rl_mlp *critic, rl_adam *opt, rl_traj *traj, uint64_t opt_steps, uint64_t first = 0) {
  RL_REQUIRE(opt_steps <= traj->max_losses, "too many optimisation steps per update");
  uint64_t Bt = b_total(traj);
  // no separate all-reduce between the reduction and the (elementwise) optimiser step: one rank, or the peer-mailbox
  // transport, whose exchange runs inside the reduction launch
  const rl_engine *eng = traj->eng;
  // (that exchange is built for Adam only: another rule on the mailbox transport reduces, exchanges and steps in turn)
  const bool mailbox = eng->ipc_active && !eng->comm && !eng->loopback && !eng->host_allreduce &&
                       ipc_allreduce_fits(eng, critic->P + 4) && opt->cfg.kind == RL_OPTIMIZER_ADAM;
  const bool fused = critic->kind == RL_MODULE_MLP && (!eng->has_collective() || mailbox);
  PassRequest slabs_only(RUN_CRITIC);
  slabs_only.reduce = false;
  for (uint64_t k = first; k < opt_steps; ++k) {
    if (fused) {  // no all-reduce between the reduction and the (elementwise) optimiser step: one launch
      const SlabRows rows = run_pass(critic, traj, slabs_only);
      launch_reduce_opt(traj, opt, rows.A, rows.B, (int)k, Bt);
    } else {
      run_pass(critic, traj, RUN_CRITIC);
      launch_opt_step(traj, opt, (int)k, Bt);
    }
  }
}

// the losses of the steps just enqueued (synchronises the engine's current stream)
static void critic_collect(rl_traj *traj, uint64_t opt_steps, rl_critic_stats *stats, float *losses_out) {
  if (!(stats || losses_out)) {
    // nothing to read back — but the call's contract is the same: a failed exchange or a range-guard violation of THESE
    // launches is this call's error, not a later entry point's, and the guard is re-armed for the next call (ADVICE
    // round 5: both used to be skipped here)
    sync(traj->eng);
    ipc_check(traj->eng);
    range_check(traj, 1u << RL_GUARD_CRITIC);
    return;
  }
  {
    std::vector<float> h(opt_steps ? opt_steps : 1);
    if (opt_steps) d2h(traj->eng, h.data(), traj->losses, opt_steps * sizeof(float));
    else sync(traj->eng);
    ipc_check(traj->eng);
    range_check(traj, 1u << RL_GUARD_CRITIC);
    if (losses_out && opt_steps) std::memcpy(losses_out, h.data(), opt_steps * sizeof(float));
    if (stats) {
      stats->steps = opt_steps;
      stats->loss_first = opt_steps ? (double)h[0] : 0.0;
      stats->loss_last = opt_steps ? (double)h[opt_steps - 1] : 0.0;
    }
  }
}

static void critic_opt_steps(rl_mlp *critic, rl_adam *opt, rl_traj *traj, uint64_t opt_steps, rl_critic_stats *stats,
                             float *losses_out) {
  critic_enqueue_steps(critic, opt, traj, opt_steps);
  critic_collect(traj, opt_steps, stats, losses_out);
}

int32_t rl_critic_update(rl_mlp *critic, rl_adam *opt, rl_traj *traj, uint64_t opt_steps, rl_critic_stats *stats,
                         float *losses_out) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    check_critic(critic, traj);
    RL_REQUIRE(opt && opt->mod == critic, "optimizer does not belong to this module");
    traj->d.tgt = traj->d.rtg;
    critic_opt_steps(critic, opt, traj, opt_steps, stats, losses_out);
  });
}

int32_t rl_values_opt_config_default(rl_values_opt_config *c) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(c, "cfg is NULL");
    c->opt_steps_per_update = 80;                // ValuesOptConfig::default (critics/opt.rs:40-51)
    c->target = RL_VALUE_TARGET_REWARD_TO_GO;    // StepValueTarget::default (critics/mod.rs:211-215)
    c->discount_factor = 0.99f;                  // max_discount_factor
  });
}

static void check_values_opt(const rl_mlp *critic, const rl_adam *opt, const rl_traj *traj,
                             const rl_values_opt_config *cfg) {
  check_critic(critic, traj);
  RL_REQUIRE(opt && opt->mod == critic, "optimizer does not belong to this module");
  RL_REQUIRE(cfg, "cfg is NULL");
  RL_REQUIRE(cfg->target == RL_VALUE_TARGET_REWARD_TO_GO || cfg->target == RL_VALUE_TARGET_ONE_STEP_TD,
             "unknown value target");
  RL_REQUIRE(cfg->discount_factor >= 0.0f && cfg->discount_factor <= 1.0f, "discount factor must be in [0, 1]");
}

// ---------------------------------------------------------------- the value forward
// V(s_t) and the values at the successor observations of cut episodes, from `critic` as it stands, left where the scans
// read them — the helper says which of the two places, and with it which scan goes with them:
//   VALUES_IN_PLANE   traj->d.values [T+1][n] (the fused 5-H-1 forward): launch_gae / launch_value_targets
//   VALUES_IN_ARRAYS  traj->seq.out / seq.succ (the general and the recurrent forwards): launch_seq_gae /
//                     launch_seq_value_targets, which read no observation and so need no SeqScope of their own;
//                     *v_last <- V(obs[T]) of every lane where the forward has it (the general one), else NULL
enum ValueLayout { VALUES_IN_PLANE, VALUES_IN_ARRAYS };
static ValueLayout value_forward(rl_traj *traj, const rl_mlp *critic, const float **v_last) {
  *v_last = nullptr;
  if (rl_module_is_recurrent(critic->kind)) {
    SeqScope sc(traj, critic);
    seq_ensure(traj, sc.x, false);
    launch_gru_seq_forward(traj, sc.x, traj->seq.out, traj->seq.succ, nullptr);
    return VALUES_IN_ARRAYS;
  }
  if (critic->general) {
    *v_last = launch_gen_values(traj, critic);
    return VALUES_IN_ARRAYS;
  }
  launch_values(traj, critic);
  return VALUES_IN_PLANE;
}

int32_t rl_gae(rl_traj *traj, const rl_mlp *critic, float gamma, float lambda) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    RL_REQUIRE(traj && critic, "NULL argument");
    RL_REQUIRE(critic->in_dim == traj->d.D && critic->out_dim == 1, "critic shape does not match the trajectory");
    const float *v_last;
    if (value_forward(traj, critic, &v_last) == VALUES_IN_ARRAYS) launch_seq_gae(traj, gamma, lambda, v_last);
    else launch_gae(traj, critic, gamma, lambda);
  });
}

// targets: once, from the critic as it stands now (tch::no_grad, opt.rs:101-104) -> traj->td, selected as traj->d.tgt
static void values_opt_targets(rl_mlp *critic, rl_traj *traj, const rl_values_opt_config *cfg) {
  if (traj->td == nullptr) {
    RL_HIP_CHECK(hipSetDevice(traj->eng->device));
    traj->td = traj->mem.alloc<float>((size_t)traj->d.T * traj->d.n);
  }
  traj->d.tgt = traj->td;
  const float *v_last;
  if (cfg->target == RL_VALUE_TARGET_REWARD_TO_GO && traj->rtg_scan_valid && traj->rtg_gamma == cfg->discount_factor) {
    // the advantage pass's lane scan has already left exactly these targets in the return plane (same recursion, same
    // operations: k_gae_scan / k_value_targets_rtg, kernels_rollout.hip) — no second scan over the rewards
    traj->d.tgt = traj->d.rtg;
  } else if (cfg->target == RL_VALUE_TARGET_REWARD_TO_GO) {
    launch_value_targets(traj, nullptr, cfg->discount_factor);
  } else if (value_forward(traj, critic, &v_last) == VALUES_IN_ARRAYS) {
    launch_seq_value_targets(traj, cfg->discount_factor, v_last);
  } else {
    launch_value_targets(traj, critic, cfg->discount_factor);
  }
  traj->last_targets = traj->d.tgt;  // (what RL_TRAJ_TARGETS reads)
}

int32_t rl_values_opt_update(rl_mlp *critic, rl_adam *opt, rl_traj *traj, const rl_values_opt_config *cfg,
                             rl_critic_stats *stats, float *losses_out) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    check_values_opt(critic, opt, traj, cfg);
    values_opt_targets(critic, traj, cfg);
    critic_opt_steps(critic, opt, traj, cfg->opt_steps_per_update, stats, losses_out);
  });
}

// ---------------------------------------------------------------- policy and critic update side by side
// The critic chain of rl_actor_critic_update runs on the engine's auxiliary stream with a workspace of its own (slab
// rows, reduced vector) and the auxiliary collective channel: inside this scope every launcher — they all read
// traj->eng->stream and the trajectory's workspace pointers at enqueue time — serves that chain.
struct AuxChain {
  rl_engine *e;
  rl_traj *t;
  AuxChain(rl_traj *traj) : e(traj->eng), t(traj) {
    if (t->aux_slabB == nullptr) {  // (the last of the three: a failed allocation leaves a call that completes the set)
      RL_HIP_CHECK(hipSetDevice(e->device));
      DevMem &mem = t->mem;
      mem.ensure(t->aux_vec, (uint64_t)t->Pmax + 4);
      mem.ensure(t->aux_slabA, mem.count_of(t->slabA));
      mem.ensure(t->aux_slabB, mem.count_of(t->slabB));
    }
    swap();
    e->stream = e->aux_stream;
    e->chan = 1;
  }
  ~AuxChain() {
    e->stream = e->main_stream;
    e->chan = 0;
    swap();
  }
  void swap() {
    std::swap(t->vec, t->aux_vec);
    std::swap(t->slabA, t->aux_slabA);
    std::swap(t->slabB, t->aux_slabB);
    std::swap(t->last_rows, t->aux_last_rows);
  }
};

// may the two chains be in flight together?  Both must run on kernels that keep everything but the slab rows and the
// reduced vector out of the trajectory's shared workspace (the fused single-launch passes), and a multi-rank job needs
// a collective that can serve two streams at once: the mailbox channels, the second RCCL communicator, or one of the
// host-blocking test transports (which serialise the chains on the host, correctly).
static bool chains_can_overlap(const rl_mlp *policy, const rl_mlp *critic, const rl_traj *traj) {
  const rl_engine *e = traj->eng;
  // (with several ranks the environment switch is the one the ranks agreed on when the collective was installed)
  if (e->n_ranks > 1 ? e->agreed_serial_env : std::getenv("RELEARN_SERIAL_UPDATE") != nullptr) return false;
  if (e->serial_update || e->kernel_variant == 1) return false;
  // (general hidden_sizes keep P-sized vectors and activation planes in workspaces both chains would share; the output
  // counts are no further condition here: check_policy leaves a module that is not `general` two, check_critic one)
  if (!fused_5_128_fits(traj, policy, 2) || !fused_5_128_fits(traj, critic, 1)) return false;
  if (policy->P > traj->Pmax || critic->P > traj->Pmax) return false;  // (the auxiliary vector is sized Pmax + 4)
  if (e->comm != nullptr && e->comm_aux == nullptr) return false;
  return true;
}

// _begin: fork, the whole critic chain onto the auxiliary stream, the TRPO chain on the main stream, the join event
// recorded — and back to the caller with the critic chain possibly still in flight (engine->pending).
static void actor_critic_begin(rl_mlp *policy, rl_mlp *critic, rl_adam *critic_opt, rl_traj *traj,
                               const rl_trpo_config *pcfg, const rl_values_opt_config *ccfg, rl_trpo_stats *pstats) {
  check_policy(policy, traj);
  RL_REQUIRE(pcfg && pstats, "NULL argument");
  check_values_opt(critic, critic_opt, traj, ccfg);
  RL_REQUIRE(policy != critic, "policy and critic must be different modules");
  rl_engine *e = traj->eng;
  RL_REQUIRE(!e->pending.active, "an update is pending on this engine: call rl_actor_critic_update_finish first");
  const uint64_t K = ccfg->opt_steps_per_update;
  RL_REQUIRE(K <= traj->max_losses, "too many optimisation steps per update");
  rl_engine::PendingUpdate &pu = e->pending;
  pu.traj = traj;
  pu.critic = critic;
  pu.steps = K;
  pu.stats = rl_critic_stats{};
  pu.losses.assign(K ? K : 1, 0.0f);
  if (!chains_can_overlap(policy, critic, traj)) {
    // policy.update, then critic.update (actor_critic.rs:196-208).  A NaN policy step is fatal BEFORE the critic moves,
    // as in the reference (Trpo::update panics inside policy.update)
    trpo_update_impl(policy, traj, pcfg, pstats);
    trpo_raise_nan(pstats);
    values_opt_targets(critic, traj, ccfg);
    critic_opt_steps(critic, critic_opt, traj, K, &pu.stats, pu.losses.data());
    pu.active = pu.joined = pu.collected = true;
    return;
  }
  traj_ensure_range(traj);  // (both chains' kernels read the observation range: measured once, before the fork)
  // fork: the auxiliary stream sees everything enqueued so far (rollout, values, advantages)
  RL_HIP_CHECK(hipEventRecord(e->ev_fork, e->main_stream));
  RL_HIP_CHECK(hipStreamWaitEvent(e->aux_stream, e->ev_fork, 0));
  try {
    // Neither chain has a host round trip before the line search's first read-back, and enqueuing a launch costs the
    // host a few microseconds: the critic chain's ~160 launches in one go would keep the TRPO chain's first kernel
    // waiting for the HOST (measured: profiles/r04_overlap_trace_8192.csv, the policy chain starts when the critic
    // chain is nearly done).  So: a few critic steps to give the device something to do, the TRPO chain's head, the
    // rest of the critic chain, and only then the TRPO chain's read-backs.
    const uint64_t K0 = K < 6 ? K : 6;
    {
      AuxChain aux(traj);
      values_opt_targets(critic, traj, ccfg);
      critic_enqueue_steps(critic, critic_opt, traj, K0);
    }
    const TrpoProgress pr = trpo_update_head(policy, traj, pcfg);
    {
      AuxChain aux(traj);
      critic_enqueue_steps(critic, critic_opt, traj, K, K0);
    }
    RL_HIP_CHECK(hipEventRecord(e->ev_join, e->aux_stream));
    trpo_update_tail(policy, traj, pcfg, pr, pstats);  // (its read-backs wait for the main stream only)
  } catch (...) {
    (void)hipStreamSynchronize(e->aux_stream);  // nothing of this update may still be running when the error returns
    (void)hipStreamSynchronize(e->main_stream);
    range_discard(traj);  // (the other chain's guard words go with the call that set them)
    throw;
  }
  pu.active = true;
  pu.joined = pu.collected = false;
  if (pstats->status == RL_OPT_NAN_LOSS || pstats->status == RL_OPT_NAN_CONSTRAINT) {
    // fatal (the reference panics); the critic chain was already in flight beside the policy chain and has advanced the
    // critic and its optimiser state — the one ordering the side-by-side form cannot keep (include/relearn_hip.h)
    (void)hipStreamSynchronize(e->aux_stream);
    pu.active = false;
    trpo_raise_nan(pstats);
  }
}

// _finish: later work on the main stream follows the critic's last step; the chain's losses come back
static void actor_critic_finish(rl_traj *traj, rl_critic_stats *cstats, float *critic_losses_out) {
  rl_engine *e = traj->eng;
  rl_engine::PendingUpdate &pu = e->pending;
  RL_REQUIRE(pu.active, "no update is pending on this engine");
  RL_REQUIRE(pu.traj == traj, "the pending update belongs to another trajectory");
  if (!pu.collected) {
    engine_settle(e);
    try {
      AuxChain aux(traj);  // (the losses were written by the auxiliary chain: read them on its stream)
      critic_collect(traj, pu.steps, &pu.stats, pu.losses.data());
    } catch (...) {
      (void)hipStreamSynchronize(e->aux_stream);
      pu.active = false;
      throw;
    }
  }
  pu.active = false;
  if (cstats) *cstats = pu.stats;
  if (critic_losses_out && pu.steps) std::memcpy(critic_losses_out, pu.losses.data(), pu.steps * sizeof(float));
}

int32_t rl_actor_critic_update_begin(rl_mlp *policy, rl_mlp *critic, rl_adam *critic_opt, rl_traj *traj,
                                     const rl_trpo_config *pcfg, const rl_values_opt_config *ccfg,
                                     rl_trpo_stats *pstats) {
  return guarded(traj ? traj->eng : nullptr,
                 [&] { actor_critic_begin(policy, critic, critic_opt, traj, pcfg, ccfg, pstats); });
}

int32_t rl_actor_critic_update_finish(rl_traj *traj, rl_critic_stats *cstats, float *critic_losses_out) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    RL_REQUIRE(traj, "NULL argument");
    actor_critic_finish(traj, cstats, critic_losses_out);
  }, false);
}

int32_t rl_actor_critic_update(rl_mlp *policy, rl_mlp *critic, rl_adam *critic_opt, rl_traj *traj,
                               const rl_trpo_config *pcfg, const rl_values_opt_config *ccfg, rl_trpo_stats *pstats,
                               rl_critic_stats *cstats, float *critic_losses_out) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    actor_critic_begin(policy, critic, critic_opt, traj, pcfg, ccfg, pstats);
    actor_critic_finish(traj, cstats, critic_losses_out);
  });
}

int32_t rl_critic_gradient(rl_mlp *critic, rl_traj *traj, float *grad_out, float *loss_out) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    check_critic(critic, traj);
    RL_REQUIRE(grad_out, "grad_out is NULL");
    uint32_t P = (uint32_t)critic->P;
    traj->d.tgt = traj->d.rtg;  // the documented loss: MSE against RL_TRAJ_RETURNS, whatever targets an update left behind
    run_pass(critic, traj, RUN_CRITIC);
    std::vector<float> h(P + 4);
    d2h(traj->eng, h.data(), traj->vec, (P + 4) * sizeof(float));
    range_check(traj, 1u << RL_GUARD_CRITIC);
    std::memcpy(grad_out, h.data(), P * sizeof(float));
    if (loss_out) *loss_out = (float)((double)h[P] / (double)b_total(traj));
  });
}

// ---------------------------------------------------------------- PPO / REINFORCE / RewardToGo
int32_t rl_ppo_config_default(rl_ppo_config *c) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(c, "cfg is NULL");
    c->opt_steps_per_update = 10;  // PpoConfig::default (ppo.rs:27-41)
    c->clip_distance = 0.2;
  });
}

int32_t rl_ppo_update(rl_mlp *policy, rl_adam *opt, rl_traj *traj, const rl_ppo_config *cfg,
                      rl_policy_opt_stats *stats, float *losses_out) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    check_policy(policy, traj);
    RL_REQUIRE(opt && opt->mod == policy, "optimizer does not belong to this module");
    RL_REQUIRE(cfg, "cfg is NULL");
    RL_REQUIRE(cfg->opt_steps_per_update <= traj->max_losses, "too many optimisation steps per update");
    rl_engine *e = traj->eng;
    uint32_t P = (uint32_t)policy->P;
    uint64_t Bt = b_total(traj), K = cfg->opt_steps_per_update;
    // initial_log_probs and the logged entropy (ppo.rs:107-118): the PASS_INIT pass stores log pi_0
    // (only the sums are read: a recurrent module skips the backward through time)
    PassRequest init(RUN_INIT);
    init.forward_only = true;
    run_pass(policy, traj, init);
    float h0[4];
    d2h(e, h0, traj->vec + P, sizeof(h0));
    // clip(1 - d, 1 + d): f64 scalars applied to a Float tensor
    float lo = (float)(1.0 - cfg->clip_distance), hi = (float)(1.0 + cfg->clip_distance);
    PassRequest ppo(RUN_PPO);
    ppo.clip_lo = lo;
    ppo.clip_hi = hi;
    for (uint64_t k = 0; k < K; ++k) {
      // gradient of the clipped surrogate against lp0 -> vec[0..P), sum of min(...) -> vec[P]
      run_pass(policy, traj, ppo);
      launch_opt_step(traj, opt, (int)k, Bt);
    }
    std::vector<float> h(K ? K : 1, 0.0f);
    if (K) d2h(e, h.data(), traj->losses, K * sizeof(float));
    range_check(traj, 1u << RL_GUARD_POLICY);
    for (auto &v : h) v = -v;  // loss = -mean(min(...))
    if (losses_out && K) std::memcpy(losses_out, h.data(), K * sizeof(float));
    if (stats) {
      stats->entropy = (double)h0[1] / (double)Bt;
      stats->steps = K;
      stats->loss_first = K ? (double)h[0] : 0.0;
      stats->loss_last = K ? (double)h[K - 1] : 0.0;
    }
  });
}

int32_t rl_reinforce_update(rl_mlp *policy, rl_adam *opt, rl_traj *traj, rl_policy_opt_stats *stats) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    check_policy(policy, traj);
    RL_REQUIRE(opt && opt->mod == policy, "optimizer does not belong to this module");
    rl_engine *e = traj->eng;
    uint32_t P = (uint32_t)policy->P;
    uint64_t Bt = b_total(traj);
    // d(-mean(log pi(a) A))/d theta equals the surrogate gradient at ratio = 1 that PASS_INIT computes
    run_pass(policy, traj, RUN_INIT);
    float h0[4];
    d2h(e, h0, traj->vec + P, sizeof(h0));
    launch_opt_step(traj, opt, -1, Bt);
    range_check(traj, 1u << RL_GUARD_POLICY);
    if (stats) {
      stats->entropy = (double)h0[1] / (double)Bt;
      stats->steps = 1;
      stats->loss_first = stats->loss_last = -((double)h0[2] / (double)Bt);
    }
  });
}

int32_t rl_reward_to_go(rl_traj *traj, float gamma) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    RL_REQUIRE(traj, "NULL argument");
    launch_gae(traj, nullptr, gamma, 0.0f);
  });
}

}  // extern "C"
