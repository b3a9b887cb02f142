// abi_traj.hip — extern "C" entry points of include/relearn_hip.h, part: trajectories, the recurrent workspace,
// rl_seq_forward and rl_rollout (host side only; kernels live in kernels_*.hip).
#include "abi_internal.hpp"

extern "C" {

// ---------------------------------------------------------------- trajectory
static void traj_field(const rl_traj *t, int32_t field, void **ptr, uint64_t *bytes) {
  uint64_t n = t->d.n, T = t->d.T, D = t->d.D;
  switch (field) {
    case RL_TRAJ_OBS: *ptr = t->d.obs; *bytes = D * (T + 1) * n * 4; break;
    case RL_TRAJ_ACTION: *ptr = t->d.action; *bytes = T * n; break;
    case RL_TRAJ_REWARD: *ptr = t->d.reward; *bytes = T * n * 4; break;
    case RL_TRAJ_FLAG: *ptr = t->d.flag; *bytes = T * n; break;
    case RL_TRAJ_TERM_OBS: *ptr = t->d.term_obs; *bytes = D * T * n * 4; break;
    case RL_TRAJ_VALUES: *ptr = t->d.values; *bytes = (T + 1) * n * 4; break;
    case RL_TRAJ_ADVANTAGES: *ptr = t->d.adv; *bytes = T * n * 4; break;
    case RL_TRAJ_RETURNS: *ptr = t->d.rtg; *bytes = T * n * 4; break;
    case RL_TRAJ_TARGETS:
      RL_REQUIRE(t->last_targets != nullptr, "no value targets yet: they are written by rl_values_opt_update");
      *ptr = const_cast<float *>(t->last_targets);
      *bytes = T * n * 4;
      break;
    default: throw RlError(RL_ERR_INVALID_ARGUMENT, "unknown trajectory field");
  }
}

// launch geometry of the update kernels for B samples
void traj_plan(rl_traj *t, uint64_t B) {
  rl_engine *e = t->eng;
  t->B = B;
  // backward: <= 1024 workgroups of 128 threads, chunk a multiple of 8 samples
  uint64_t chunk = (B + 1023) / 1024;
  chunk = ((chunk + 7) / 8) * 8;
  if (chunk < 64) chunk = 64;
  t->bwd_chunk = (uint32_t)chunk;
  t->nbA = (uint32_t)((B + chunk - 1) / chunk);
  uint64_t nbB = (B + 255) / 256;
  if (nbB > 2048) nbB = 2048;
  t->nbB = (uint32_t)nbB;
  // v2 kernels: persistent grid, one workgroup per CU (fewer, fatter workgroups = fewer slab rows for the reduction
  // that follows every launch), one 32-sample tile per wave and iteration; policy kernels run eight waves per workgroup
  uint64_t n_tiles = (B + 31) / 32;
  uint64_t nbV2 = (n_tiles + 7) / 8;
  uint64_t max_v2 = (uint64_t)e->prop.multiProcessorCount;
  // the critic step runs one workgroup of twelve waves per CU (168 VGPRs: three waves per SIMD; 149 KB LDS)
  uint64_t nbC = (n_tiles + 11) / 12, max_c = (uint64_t)e->prop.multiProcessorCount;
  if (nbC > max_c) nbC = max_c;
  t->nbC = (uint32_t)nbC;
  if (nbV2 > max_v2) nbV2 = max_v2;
  t->nbV2 = (uint32_t)nbV2;
}

// `resizable`: the sample count changes between launches (DQN minibatches): slabs are sized for the largest grid
// any B <= n_lanes * horizon can plan
rl_traj *traj_alloc(rl_engine *e, uint64_t n_lanes, uint64_t horizon, uint32_t obs_dim, bool resizable, TrajLevel level) {
  RL_REQUIRE(n_lanes > 0 && n_lanes < (1ull << 31), "bad n_lanes");
  RL_REQUIRE(horizon > 0 && horizon < (1ull << 20), "bad horizon");
  // (what reads a trajectory checks its own width against the planes')
  // up to 16 planes (the wide meta-bandit lanes) every entry point is rl_traj_create, up to 20 (the meta-MDP lanes of
  // rl_env_create_meta_mdp_wide) the two wider ones are rl_traj_create_wide, and rl_traj_create_wide24 ends at 24 (the
  // PartitionGame lanes): the words are those of the level a width falls in
  if (level >= TRAJ_LEVEL_WIDE24 && obs_dim > traj_max_obs_dim(TRAJ_LEVEL_WIDE))
    RL_REQUIRE(obs_dim <= traj_max_obs_dim(TRAJ_LEVEL_WIDE24), "rl_traj_create_wide24: obs_dim must be in 1..24");
  else if (level >= TRAJ_LEVEL_WIDE && obs_dim > traj_max_obs_dim(TRAJ_LEVEL_BASE))
    RL_REQUIRE(obs_dim <= traj_max_obs_dim(TRAJ_LEVEL_WIDE), "rl_traj_create_wide: obs_dim must be in 1..20");
  else
    RL_REQUIRE(obs_dim >= 1 && obs_dim <= traj_max_obs_dim(TRAJ_LEVEL_BASE), "obs_dim must be in 1..16");
  RL_REQUIRE(n_lanes * horizon < (1ull << 32), "T * n must fit 32 bits");
  RL_HIP_CHECK(hipSetDevice(e->device));
  std::unique_ptr<rl_traj> t(new rl_traj());
  t->eng = e;
  t->d.n = (uint32_t)n_lanes;
  t->d.T = (uint32_t)horizon;
  t->d.D = obs_dim;
  // (at least five observation planes whatever the logical width: the fused recurrent kernels are built for five features
  // and read the planes past the module's in_dim as zeros)
  uint64_t n = n_lanes, T = horizon, D = obs_dim > 5 ? obs_dim : 5;
  DevMem &mem = t->mem;
  t->d.obs = mem.alloc<float>(D * (T + 1) * n);
  RL_HIP_CHECK(hipMemsetAsync(t->d.obs, 0, D * (T + 1) * n * 4, e->stream));
  t->d.action = mem.alloc<uint8_t>(T * n);
  t->d.reward = mem.alloc<float>(T * n);
  t->d.flag = mem.alloc<uint8_t>(T * n);
  t->d.term_obs = mem.alloc<float>(D * T * n);
  t->d.values = mem.alloc<float>((T + 1) * n);
  t->d.adv = mem.alloc<float>(T * n);
  t->d.rtg = mem.alloc<float>(T * n);
  t->d.tgt = t->d.rtg;  // the critic regresses on the returns unless rl_values_opt_update selects other targets
  t->d.range = mem.alloc<uint32_t>(RL_RANGE_ALLOC_WORDS);
  RL_HIP_CHECK(hipMemsetAsync(t->d.range, 0, RL_RANGE_ALLOC_WORDS * sizeof(uint32_t), e->stream));
  {
    t->h_range_err = mem.alloc_host<uint32_t>(16, /*mapped=*/true);
    static_cast<volatile uint32_t *>(t->h_range_err)[RL_GUARD_POLICY] = 0u;
    static_cast<volatile uint32_t *>(t->h_range_err)[RL_GUARD_CRITIC] = 0u;
    void *dp = nullptr;
    RL_HIP_CHECK(hipHostGetDevicePointer(&dp, t->h_range_err, 0));
    t->d.range_err = static_cast<uint32_t *>(dp);
  }
  t->lp0 = mem.alloc<float>(2 * n * T);
  t->dz = mem.alloc<float>(2 * n * T);
  t->Pmax = 128 * 5 + 128 + 2 * 128 + 2;
  traj_plan(t.get(), n * T);
  uint32_t rows = t->nbA;
  if (t->nbV2 > rows) rows = t->nbV2;
  if (t->nbC > rows) rows = t->nbC;
  uint32_t rowsB = t->nbB > rows ? t->nbB : rows;
  if (resizable) {
    uint32_t cap = 8u * (uint32_t)e->prop.multiProcessorCount;
    if (cap < 2048) cap = 2048;
    rows = rowsB = cap;
  }
  t->slabA = mem.alloc<double>((size_t)rows * t->Pmax);
  t->slabB = mem.alloc<double>((size_t)rowsB * 4);
  t->vec = mem.alloc<float>(t->Pmax + 4);
  t->cg_x = mem.alloc<float>(t->Pmax);
  t->cg_r = mem.alloc<float>(t->Pmax);
  t->cg_p = mem.alloc<float>(t->Pmax);
  t->prev_params = mem.alloc<float>(t->Pmax);
  t->descent = mem.alloc<float>(t->Pmax);
  t->max_losses = 4096;
  t->losses = mem.alloc<float>(t->max_losses);
  t->trpo = mem.alloc<TrpoStateDev>(1);
  RL_HIP_CHECK(hipMemsetAsync(t->d.term_obs, 0, D * T * n * 4, e->stream));
  RL_HIP_CHECK(hipMemsetAsync(t->d.values, 0, (T + 1) * n * 4, e->stream));
  RL_HIP_CHECK(hipMemsetAsync(t->d.adv, 0, T * n * 4, e->stream));
  RL_HIP_CHECK(hipMemsetAsync(t->d.rtg, 0, T * n * 4, e->stream));
  RL_HIP_CHECK(hipMemsetAsync(t->trpo, 0, sizeof(TrpoStateDev), e->stream));
  RL_HIP_CHECK(hipStreamSynchronize(e->stream));
  e->live_handles += 1;
  return t.release();
}

int32_t rl_traj_create(rl_engine *e, uint64_t n_lanes, uint64_t horizon, uint32_t obs_dim, rl_traj **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && out, "NULL argument");
    *out = nullptr;
    *out = traj_alloc(e, n_lanes, horizon, obs_dim, false);
  });
}

// The same trajectory with up to 20 observation planes; up to 16 it is rl_traj_create's, refusals and words included
int32_t rl_traj_create_wide(rl_engine *e, uint64_t n_lanes, uint64_t horizon, uint32_t obs_dim, rl_traj **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && out, "NULL argument");
    *out = nullptr;
    *out = traj_alloc(e, n_lanes, horizon, obs_dim, false, TRAJ_LEVEL_WIDE);
  });
}

// ... with up to 24 (PartitionGame lanes under a visible limit); up to 20 it is rl_traj_create_wide's
int32_t rl_traj_create_wide24(rl_engine *e, uint64_t n_lanes, uint64_t horizon, uint32_t obs_dim, rl_traj **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && out, "NULL argument");
    *out = nullptr;
    *out = traj_alloc(e, n_lanes, horizon, obs_dim, false, TRAJ_LEVEL_WIDE24);
  });
}

int32_t rl_traj_destroy(rl_traj *t) {
  if (t && t->eng->pending.traj == t) t->eng->pending.active = false;  // (its pending update dies with it)
  return destroy_child(t);
}

int32_t rl_traj_field_bytes(const rl_traj *t, int32_t field, uint64_t *bytes) {
  return guarded(t ? t->eng : nullptr, [&] {
    RL_REQUIRE(t && bytes, "NULL argument");
    void *p;
    traj_field(t, field, &p, bytes);
  });
}

int32_t rl_traj_read(rl_traj *t, int32_t field, void *host, uint64_t bytes) {
  return guarded(t ? t->eng : nullptr, [&] {
    RL_REQUIRE(t && host, "NULL argument");
    void *p;
    uint64_t need;
    traj_field(t, field, &p, &need);
    RL_REQUIRE(bytes == need, "byte count mismatch for trajectory field");
    d2h(t->eng, host, p, bytes);
  });
}

int32_t rl_traj_write(rl_traj *t, int32_t field, const void *host, uint64_t bytes) {
  return guarded(t ? t->eng : nullptr, [&] {
    RL_REQUIRE(t && host, "NULL argument");
    void *p;
    uint64_t need;
    traj_field(t, field, &p, &need);
    RL_REQUIRE(bytes == need, "byte count mismatch for trajectory field");
    h2d(t->eng, p, host, bytes);
    if (field == RL_TRAJ_ACTION) {  // host-made actions: no env names their space; a policy must at least cover them
      const uint8_t *a = static_cast<const uint8_t *>(host);
      uint8_t hi = 0;
      for (uint64_t i = 0; i < bytes; ++i) hi = a[i] > hi ? a[i] : hi;
      t->n_actions = 0;
      t->max_action = hi;
    }
    if (field == RL_TRAJ_OBS) t->range_valid = t->range_reset = false;  // (the range guard reads the planes' magnitudes)
    t->rtg_scan_valid = false;  // (whatever was written, the return plane is no longer known to match the rewards)
  });
}

// ---------------------------------------------------------------- recurrent workspace
// the P-sized vectors of the update workspace grow with the module: all six, or none and Pmax = 0 (the next call then
// starts over instead of finding Pmax large enough and some vectors missing)
void traj_ensure_pvec(rl_traj *t, uint64_t P) {
  if (t->Pmax >= P) return;
  float **const vecs[] = {&t->vec, &t->cg_x, &t->cg_r, &t->cg_p, &t->prev_params, &t->descent};
  t->Pmax = 0;
  for (float **p : vecs) t->mem.release(*p);
  try {
    for (float **p : vecs) *p = t->mem.alloc<float>(P + (p == &t->vec ? 4 : 0));
  } catch (...) {
    for (float **p : vecs) t->mem.release(*p);
    throw;
  }
  t->Pmax = (uint32_t)P;
}

void seq_ensure(rl_traj *t, const rl_mlp *mod, bool training) {
  RL_REQUIRE(rl_module_is_recurrent(mod->kind), "not a recurrent module");
  if (mod->lane_kernels()) return stack_ensure(t, mod, training);  // lane-per-thread kernels: no tile or width condition
  RL_REQUIRE(t->d.n % 32 == 0, "the recurrent kernels work on tiles of 32 lanes: n_lanes must be a multiple of 32");
  RL_REQUIRE(t->d.D == 5 && mod->in_dim == 5, "recurrent path: built for 5 observation features");
  SeqDev &q = t->seq;
  uint64_t n = t->d.n, T = t->d.T;
  q.tiles = (uint32_t)(n / 32);  // (the output planes may already exist: the general-MLP path shares them)
  seq_ensure_outputs(t);
  if (training && q.dpre == nullptr) {
    uint64_t blocks = T * q.tiles;
    t->mem.ensure(q.act, blocks * RL_SEQ_ACT_ARRAYS * 128 * 32);
    q.dpre = t->mem.alloc<float>(blocks * RL_SEQ_DPRE_ARRAYS * 128 * 32);
    // weight-gradient partials: contiguous runs of (t, tile) blocks per workgroup, <= 1024 workgroups and at most
    // ~2048 samples accumulated in f32 before the f64 reduction
    uint64_t bpc = (blocks + 1023) / 1024;
    if (bpc < 1) bpc = 1;
    if (bpc > 64) bpc = 64;
    q.blocks_per_chunk = (uint32_t)bpc;
    q.chunks = (uint32_t)((blocks + bpc - 1) / bpc);
  }
  if (training) {
    // + the rows of the head kernel (head columns) and of the backward recurrence (one per tile, input-side columns)
    t->mem.ensure(q.wg_slab, (uint64_t)(q.chunks + (q.tiles > RL_SEQ_HEAD_ROWS ? q.tiles : RL_SEQ_HEAD_ROWS)) * mod->P);
    traj_ensure_pvec(t, mod->P);
  }
}

int32_t rl_seq_forward(rl_mlp *mod, rl_traj *traj, float *out, float *succ_out) {
  return guarded(traj ? traj->eng : nullptr, [&] {
    RL_REQUIRE(mod && traj && out, "NULL argument");
    RL_REQUIRE(mod->eng == traj->eng, "handles belong to different engines");
    RL_REQUIRE(rl_module_is_recurrent(mod->kind), "not a recurrent module");
    {
      SeqScope sc(traj, mod);
      seq_ensure(traj, sc.x, false);
      launch_gru_seq_forward(traj, sc.x, traj->seq.out, succ_out ? traj->seq.succ : nullptr, nullptr);
    }
    uint64_t bytes = (uint64_t)mod->out_dim * traj->d.T * traj->d.n * sizeof(float);
    d2h(traj->eng, out, traj->seq.out, bytes);
    if (succ_out) d2h(traj->eng, succ_out, traj->seq.succ, bytes);
  });
}

// ---------------------------------------------------------------- rollout + GAE
int32_t rl_rollout(rl_env *env, const rl_mlp *policy, rl_traj *traj) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(env && policy && traj, "NULL argument");
    RL_REQUIRE(env->eng == traj->eng && env->eng == policy->eng, "handles belong to different engines");
    // A critic chain left in flight by rl_actor_critic_update_begin reads its own trajectory and the critic: a rollout
    // into ANOTHER trajectory touches neither (it reads the policy the TRPO chain has already finished with) and goes
    // ahead beside it on the main stream; anything else waits for the chain like every other call.
    if (traj == env->eng->pending.traj || policy == env->eng->pending.critic) engine_settle(env->eng);
    traj->range_valid = traj->range_reset = false;  // new observations: the range guard has them measured again
    traj->rtg_scan_valid = false;                   // new rewards: the return plane belongs to the old ones
    rollout_check_env_kind(env->kind, *policy);
    RL_REQUIRE(traj->d.n == env->cfg.n_lanes && traj->d.D == env->D, "trajectory shape does not match the env");
    rollout_check_shapes(env->D, env->A, *policy);
    traj->n_actions = env->A;
    const RolloutPath path = rollout_path(env, policy);  // (or the refusal of this pair)
    switch (path) {
      case ROLL_GENERAL: launch_gen_rollout(env, policy, traj); break;
      case ROLL_STACK:
        stack_ensure(traj, policy, false);
        launch_stack_rollout(env, policy, traj);
        break;
      case ROLL_TILE_RECURRENT: {
        SeqScope sc(traj, policy);
        seq_ensure(traj, sc.x, false);
        launch_rollout_gru(env, sc.x, traj);
        break;
      }
      case ROLL_INDEX_MLP: launch_rollout_chain_mlp(env, policy, traj); break;
      case ROLL_CARTPOLE: launch_rollout(env, policy, traj); break;
    }
    if (!rollout_path_counts_steps(path)) env->t_global += traj->d.T;
  }, false);
}

}  // extern "C"
