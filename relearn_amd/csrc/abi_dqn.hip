// abi_dqn.hip — extern "C" entry points of include/relearn_hip.h, part: DQN with the replay store in HBM (host side only; kernels live in kernels_*.hip).
#include "abi_internal.hpp"

extern "C" {

// ---------------------------------------------------------------- DQN (src/torch/agents/dqn.rs)
int32_t rl_dqn_config_default(rl_dqn_config *c) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(c, "cfg is NULL");
    std::memset(c, 0, sizeof(*c));
    c->target = RL_DQN_TARGET_REWARD_TO_GO;               // StepValueTarget::default (critics/mod.rs:211-215)
    c->exploration_kind = RL_SCHEDULE_LINEAR_ANNEALED;    // schedules.rs:23-31
    c->exploration_start = 1.0;
    c->exploration_end = 0.1;
    c->exploration_period = 10000000;
    c->minibatch_steps = 100000;                          // dqn.rs:63-70
    c->opt_steps_per_update = 50;
    c->buffer_capacity = 0;
    c->episode_capacity = 0;
    c->update_kind = RL_COLLECT_FIRST_REST;
    c->update_first = 1000000;
    c->update_rest = 100000;
    c->discount_factor = 0.99f;
  });
}

static double dqn_exploration_rate(const rl_dqn *q, bool training) {
  if (!training) return 0.0;  // schedules.rs:38
  if (q->cfg.exploration_kind == RL_SCHEDULE_CONSTANT) return q->cfg.exploration_start;
  double frac = (double)q->global_steps / (double)q->cfg.exploration_period;
  if (!(frac < 1.0)) frac = 1.0;  // f64::min(1.0)
  return frac * (q->cfg.exploration_end - q->cfg.exploration_start) + q->cfg.exploration_start;
}

static ReplayDev replay_alloc(rl_engine *e, DevMem &mem, uint32_t N, uint32_t C, uint32_t E, uint32_t D) {
  ReplayDev r{};
  r.N = N;
  r.C = C;
  r.E = E;
  r.D = D;
  size_t cn = (size_t)C * N;
  r.rec = mem.alloc<ReplayRec>(cn);
  r.next = mem.alloc<ReplayNext>(cn);
  r.hi = D > 5 ? mem.alloc<float4>(cn) : nullptr;
  r.head = mem.alloc<uint32_t>(N);
  r.count = mem.alloc<uint32_t>(N);
  r.ep_head = mem.alloc<uint32_t>(N);
  r.ep_count = mem.alloc<uint32_t>(N);
  r.total = mem.alloc<uint32_t>(N);
  r.ep_end = mem.alloc<uint32_t>((size_t)E * N);
  r.actor_pos = mem.alloc<uint64_t>(N);
  r.error = mem.alloc<int32_t>(1);
  uint32_t *zero_u32[] = {r.head, r.count, r.ep_head, r.ep_count, r.total};
  for (uint32_t *p : zero_u32) RL_HIP_CHECK(hipMemsetAsync(p, 0, (size_t)N * 4, e->stream));
  RL_HIP_CHECK(hipMemsetAsync(r.actor_pos, 0, (size_t)N * 8, e->stream));
  RL_HIP_CHECK(hipMemsetAsync(r.error, 0, 4, e->stream));
  RL_HIP_CHECK(hipMemsetAsync(r.next, 0, cn * sizeof(ReplayNext), e->stream));
  return r;
}

// what a DQN handle holds besides memory (also the clean-up of a failed rl_dqn_create): the draw stream, the events and
// the minibatch workspace; the device and pinned memory goes with `mem` after this body
rl_dqn::~rl_dqn() {
  if (draw_stream) {
    (void)hipStreamSynchronize(draw_stream);
    (void)hipStreamDestroy(draw_stream);
  }
  for (hipEvent_t ev : draw_events) (void)hipEventDestroy(ev);
  if (main_event) (void)hipEventDestroy(main_event);
  if (mb) rl_traj_destroy(mb);
  if (roll) rl_traj_destroy(roll);
  if (seq) rl_traj_destroy(seq);
}

// With several ranks a failure must be raised on ALL of them: a rank that throws before a collective leaves its peers
// blocked in it.  One float travels through the update workspace; true when any rank reports a failure.
static bool dqn_any_rank_failed(rl_dqn *q, bool local_failure) {
  rl_engine *e = q->eng;
  if (e->n_ranks <= 1) return local_failure;
  float flag = local_failure ? 1.0f : 0.0f;
  h2d(e, q->mb->vec, &flag, sizeof(flag));
  rl_allreduce_sum_f32(e, q->mb->vec, 1);
  d2h(e, &flag, q->mb->vec, sizeof(flag));
  return flag > 0.0f;
}

static void dqn_build(rl_env *env, rl_mlp *qnet, rl_adam *opt, const rl_dqn_config *cfg, rl_dqn **out, bool recurrent);

// what every constructor checks first.  `who`: the messages' prefix — the entry point's name and a colon, or nothing
// (rl_dqn_create's messages carry none)
static void dqn_check_handles(const std::string &who, rl_env *env, rl_mlp *qnet, rl_adam *opt, const rl_dqn_config *cfg,
                              rl_dqn **out) {
  RL_REQUIRE(env && qnet && opt && cfg && out, who + "NULL argument");
  *out = nullptr;
  RL_REQUIRE(qnet->eng == env->eng && opt->eng == env->eng, who + "handles belong to different engines");
  RL_REQUIRE(opt->mod == qnet, who + "optimizer does not belong to the action-value module");
}

// The env table of the two-action constructors (relearn_hip.h): the collection kernels step CartPole lanes of 4 or 5
// observation features and the index-env lanes (Chain, MemoryGame, the bandit) of 4..8.  Anything else is refused here,
// by name: no env is collected by another env's code.  rl_dqn_create_recurrent's messages begin with its name.
static void dqn_check_env(const rl_env *env, bool recurrent) {
  const std::string name = recurrent ? "rl_dqn_create_recurrent" : "rl_dqn_create";
  if (env->kind == RL_ENV_TABULAR_MDP)
    throw RlError(RL_ERR_UNSUPPORTED,
                  name + " is not built for RL_ENV_TABULAR_MDP lanes" + (recurrent ? "" : " (rl_dqn_create_finite is)"));
  if (env->kind == RL_ENV_META_BANDIT)
    throw RlError(RL_ERR_UNSUPPORTED, name + " is not built for RL_ENV_META_BANDIT lanes");
  if (env->kind == RL_ENV_META_MDP)
    throw RlError(RL_ERR_UNSUPPORTED, name + " is not built for RL_ENV_META_MDP lanes");
  if (env->kind == RL_ENV_PARTITION)
    throw RlError(RL_ERR_UNSUPPORTED, name + " is not built for RL_ENV_PARTITION lanes");
  const bool index_env = env->kind == RL_ENV_CHAIN || env->kind == RL_ENV_MEMORY || env->kind == RL_ENV_BANDIT;
  if (env->kind != RL_ENV_CARTPOLE && !index_env)
    throw RlError(RL_ERR_UNSUPPORTED, (recurrent ? name + ": " : "") +
                                          "DQN collection is built for CartPole, Chain, MemoryGame and bandit lanes");
  if (env->D < RL_ENV_MIN_OBS_DIM || env->D > (index_env ? RL_TRAJ_MAX_OBS_DIM : 5u))
    throw RlError(RL_ERR_UNSUPPORTED, (recurrent ? name : "DQN") + (index_env ? " on index-env lanes: 4..8 observation features"
                                                                              : " on CartPole lanes: 4 or 5 observation features"));
}

int32_t rl_dqn_create(rl_env *env, rl_mlp *qnet, rl_adam *opt, const rl_dqn_config *cfg, rl_dqn **out) {
  return guarded(env ? env->eng : nullptr, [&] {
    dqn_check_handles("", env, qnet, opt, cfg, out);
    if (qnet->out_dim > 2) throw RlError(RL_ERR_UNSUPPORTED, "DQN kernels are built for 2 actions");
    RL_REQUIRE(qnet->in_dim == env->D && qnet->out_dim == env->A, "action-value module does not match the env");
    RL_REQUIRE(env->A == 2, "DQN kernels are built for 2-action envs");
    dqn_check_env(env, /*recurrent=*/false);
    if (env->D > 5 && !qnet->general && !rl_module_is_recurrent(qnet->kind))
      throw RlError(RL_ERR_UNSUPPORTED, "DQN over 6..8 observation features: the fused collection kernel takes 4 or 5");
    // DqnConfig<MB> is generic over the module (dqn.rs:26-39): feed-forward modules of any MlpConfig build (the fused
    // 5-128-2 shape on the fused kernels, others on the per-layer kernels); recurrent action-value modules do not
    if (rl_module_is_recurrent(qnet->kind))
      throw RlError(RL_ERR_BUILD_AGENT, "DQN is built for feed-forward action-value modules");
    dqn_build(env, qnet, opt, cfg, out, /*recurrent=*/false);
  });
}

// DqnConfig<VB> over a sequence module (dqn.rs:75-86: VB::Module: SeqPacked + SeqIterative): the actor carries the
// module's state through an episode (DqnActor::EpisodeState, dqn.rs:354-358) and the update runs seq_packed over whole
// sampled episodes.  The env table of rl_dqn_create; every recurrent chain of two outputs.
int32_t rl_dqn_create_recurrent(rl_env *env, rl_mlp *qnet, rl_adam *opt, const rl_dqn_config *cfg, rl_dqn **out) {
  return guarded(env ? env->eng : nullptr, [&] {
    dqn_check_handles("rl_dqn_create_recurrent: ", env, qnet, opt, cfg, out);
    if (!rl_module_is_recurrent(qnet->kind))
      throw RlError(RL_ERR_BUILD_AGENT,
                    "rl_dqn_create_recurrent takes a recurrent action-value module; use rl_dqn_create for a feed-forward one");
    dqn_check_env(env, /*recurrent=*/true);
    if (qnet->out_dim > 2 || env->A > 2)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_dqn_create_recurrent: the DQN kernels are built for 2 actions");
    RL_REQUIRE(qnet->in_dim == env->D && qnet->out_dim == env->A,
               "rl_dqn_create_recurrent: action-value module does not match the env");
    dqn_build(env, qnet, opt, cfg, out, /*recurrent=*/true);
  });
}

// DqnConfig over any finite action space (dqn.rs:75-86, AS: FiniteSpace; the actor's action_space.sample(rng) and argmax,
// dqn.rs:360-379; the one-step TD target's amax(-1), dqn.rs:300-309).  Two actions: what the two constructors above build,
// through them.  3..8 actions: the index-env lanes that have them — the bandit of 3..8 arms, MemoryGame(k >= 3, h) — with
// a feed-forward module (always on the per-layer kernels: step-wise collection) or a recurrent chain of one output per
// action (rl_rnn_chain_create: k_stack_collect_dqn<.., NA>).
int32_t rl_dqn_create_finite(rl_env *env, rl_mlp *qnet, rl_adam *opt, const rl_dqn_config *cfg, rl_dqn **out) {
  if (env && qnet && env->A <= 2 && qnet->out_dim <= 2 && env->kind != RL_ENV_META_BANDIT &&
      env->kind != RL_ENV_TABULAR_MDP && env->kind != RL_ENV_META_MDP && env->kind != RL_ENV_PARTITION)
    return rl_module_is_recurrent(qnet->kind) ? rl_dqn_create_recurrent(env, qnet, opt, cfg, out)
                                              : rl_dqn_create(env, qnet, opt, cfg, out);
  return guarded(env ? env->eng : nullptr, [&] {
    dqn_check_handles("rl_dqn_create_finite: ", env, qnet, opt, cfg, out);
    if (env->kind == RL_ENV_META_BANDIT)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_dqn_create_finite is not built for RL_ENV_META_BANDIT lanes");
    if (env->kind == RL_ENV_META_MDP)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_dqn_create_finite is not built for RL_ENV_META_MDP lanes");
    if (env->kind == RL_ENV_PARTITION)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_dqn_create_finite is not built for RL_ENV_PARTITION lanes");
    RL_REQUIRE(qnet->in_dim == env->D && qnet->out_dim == env->A,
               "rl_dqn_create_finite: action-value module does not match the env's (obs_dim, n_actions)");
    if (env->kind == RL_ENV_TABULAR_MDP) {
      // tabular-MDP lanes: every action count 2..8 and every width 2..8 through the step-wise collection
      // (k_dqn_lane_step<MdpOps, D, A>), which reads the outputs of a module on the per-layer kernels
      if (rl_module_is_recurrent(qnet->kind))
        throw RlError(RL_ERR_UNSUPPORTED,
                      "rl_dqn_create_finite: recurrent DQN is not built for RL_ENV_TABULAR_MDP lanes");
      if (qnet->kind != RL_MODULE_MLP || !qnet->general)
        throw RlError(RL_ERR_UNSUPPORTED,
                      "rl_dqn_create_finite on RL_ENV_TABULAR_MDP lanes: the action-value module runs the per-layer "
                      "kernels; a module of the fused shape (4 or 5 inputs, one ReLU layer of at most 128 units, two "
                      "outputs, with biases) is not collected on these lanes");
      dqn_build(env, qnet, opt, cfg, out, false);
      return;
    }
    // (env->A > 2 from here on: the two-action envs went to the older constructors)
    if (env->kind != RL_ENV_MEMORY && env->kind != RL_ENV_BANDIT)
      throw RlError(RL_ERR_UNSUPPORTED,
                    "rl_dqn_create_finite over more than two actions: MemoryGame and bandit lanes");
    if (env->A > 8) throw RlError(RL_ERR_UNSUPPORTED, "rl_dqn_create_finite: 2..8 actions");
    if (env->D < RL_ENV_MIN_OBS_DIM || env->D > RL_TRAJ_MAX_OBS_DIM)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_dqn_create_finite on index-env lanes: 4..8 observation features");
    const bool recurrent = rl_module_is_recurrent(qnet->kind);
    if (recurrent) {
      if (!qnet->lane_kernels())
        throw RlError(RL_ERR_UNSUPPORTED,
                      "rl_dqn_create_finite: a recurrent module of more than two outputs comes from rl_rnn_chain_create");
    } else if (qnet->kind != RL_MODULE_MLP || !qnet->general) {
      throw RlError(RL_ERR_UNSUPPORTED,
                    "rl_dqn_create_finite: a feed-forward module of more than two outputs runs the per-layer kernels");
    }
    dqn_build(env, qnet, opt, cfg, out, recurrent);
  });
}


// what the constructors share: the configuration's checks, the replay store, the sampler's lists and the minibatch
// workspace (+ the recurrent agent's two trajectory-shaped workspaces)
static void dqn_build(rl_env *env, rl_mlp *qnet, rl_adam *opt, const rl_dqn_config *cfg, rl_dqn **out, bool recurrent) {
  rl_engine *e = env->eng;
  RL_REQUIRE(cfg->target == RL_DQN_TARGET_REWARD_TO_GO || cfg->target == RL_DQN_TARGET_ONE_STEP_TD, "bad target");
  RL_REQUIRE(cfg->minibatch_steps > 0 && cfg->minibatch_steps < (1ull << 30), "bad minibatch_steps");
  RL_REQUIRE(cfg->buffer_capacity > 0 && cfg->buffer_capacity < (1ull << 31), "bad buffer_capacity");
  uint64_t E = cfg->episode_capacity ? cfg->episode_capacity : cfg->buffer_capacity;
  RL_REQUIRE(E <= cfg->buffer_capacity, "episode_capacity exceeds buffer_capacity");
  RL_REQUIRE(cfg->opt_steps_per_update <= 4096, "too many optimisation steps per update");
  if (cfg->exploration_kind == RL_SCHEDULE_LINEAR_ANNEALED)
    RL_REQUIRE(cfg->exploration_period > 0, "exploration_period must be positive");
  uint64_t N = env->cfg.n_lanes;
  // (a step: its record, its successor observation, and features 5..7 of an observation wider than the record)
  const uint64_t step_bytes = sizeof(ReplayRec) + sizeof(ReplayNext) + (env->D > 5 ? sizeof(float4) : 0);
  RL_REQUIRE(cfg->buffer_capacity * N * step_bytes < (200ull << 30), "replay store would not fit in HBM");
  RL_HIP_CHECK(hipSetDevice(e->device));
  std::unique_ptr<rl_dqn> q(new rl_dqn());
  q->eng = e;
  q->env = env;
  q->qnet = qnet;
  q->opt = opt;
  q->cfg = *cfg;
  q->cfg.episode_capacity = E;
  q->A = env->A;
  DevMem &mem = q->mem;
  q->rp = replay_alloc(e, mem, (uint32_t)N, (uint32_t)cfg->buffer_capacity, (uint32_t)E, env->D);
  q->d_agent_pos = mem.alloc<uint64_t>(1);
  RL_HIP_CHECK(hipMemsetAsync(q->d_agent_pos, 0, 8, e->stream));
  // take_while accepts episodes while total < minibatch_steps and every episode has >= 1 step
  q->max_eps = (uint32_t)cfg->minibatch_steps;
  q->max_steps_mb = cfg->minibatch_steps - 1 + cfg->buffer_capacity;
  // the episode lists of all opt_steps_per_update minibatches of an update are drawn in one launch
  const size_t nb = cfg->opt_steps_per_update ? cfg->opt_steps_per_update : 1;
  for (uint32_t **list : {&q->eps.lane, &q->eps.start, &q->eps.len, &q->eps.off})
    *list = mem.alloc<uint32_t>(nb * q->max_eps);
  q->d_counts = mem.alloc<DqnCountsDev>(nb);
  RL_HIP_CHECK(hipMemsetAsync(q->d_counts, 0, nb * sizeof(DqnCountsDev), e->stream));
  q->mb = traj_alloc(e, q->max_steps_mb, 1, env->D, true);
  // (dz: one plane per action, sized while the workspace still has its allocation's sample count)
  traj_ensure_action_planes(q->mb, q->A);
  {  // the fused step's range guard (bf16_tile.hpp): the words hold the magnitude range of every observation the
     // collection kernel has put into the store so far (k_rollout_dqn folds what it writes, one fold per wave
     // and launch; never reset, so they bound every minibatch drawn from the store from outside).  Rounds 3-5 kept fixed bounds here, 2^-64 .. 2^16,
     // under which a Q-network with a zero bias could never pass the guard.
    std::vector<uint32_t> words(RL_RANGE_WORDS, 0u);  // every slot of the minima / the maxima (bf16_tile.hpp)
    for (int s = 0; s < 64; ++s) words[(size_t)s * 32] = 0x7F7FFFFFu;  // "nothing seen": largest finite minimum, maximum 0
    h2d(e, q->mb->d.range, words.data(), words.size() * sizeof(uint32_t));
    q->mb->range_fixed = true;  // (maintained by the builders: no measuring pass over the workspace)
  }
  q->own_obs = q->mb->d.obs;
  q->own_target = q->mb->d.adv;
  q->own_action = q->mb->d.action;
  q->own_flag = q->mb->d.flag;
  if (recurrent) {
    q->recurrent = true;
    q->roll = traj_alloc(e, N, 1, env->D, false);
    stack_ensure(q->roll, qnet, false);
    q->seq = traj_alloc(e, 1, 1, env->D, true);
  }
  sync(e);
  e->live_handles += 1;
  *out = q.release();
}

int32_t rl_dqn_destroy(rl_dqn *q) { return destroy_child(q); }

int32_t rl_dqn_exploration_rate(const rl_dqn *q, int32_t training, double *rate_out) {
  return guarded(q ? q->eng : nullptr, [&] {
    RL_REQUIRE(q && rate_out, "NULL argument");
    *rate_out = dqn_exploration_rate(q, training != 0);
  });
}

int32_t rl_dqn_min_update_size(const rl_dqn *q, uint64_t *min_steps_out, uint64_t *slack_steps_out) {
  return guarded(q ? q->eng : nullptr, [&] {
    RL_REQUIRE(q && min_steps_out && slack_steps_out, "NULL argument");
    // DataCollectionSchedule::update_size (schedules.rs:58-68)
    uint64_t min_steps;
    if (q->cfg.update_kind == RL_COLLECT_CONSTANT) min_steps = q->cfg.update_first;
    else min_steps = q->global_steps < q->cfg.update_first ? q->cfg.update_first : q->cfg.update_rest;
    *min_steps_out = min_steps;
    // HistoryDataBound::with_default_slack (src/agents/buffers/mod.rs:54-63): 1 % of min_steps, between 5 and 1000
    uint64_t slack = min_steps / 100;
    slack = slack < 5 ? 5 : (slack > 1000 ? 1000 : slack);
    *slack_steps_out = slack;
  });
}

int32_t rl_dqn_collect(rl_dqn *q, uint64_t horizon, rl_dqn_collect_stats *stats) {
  return guarded(q ? q->eng : nullptr, [&] {
    RL_REQUIRE(q, "NULL argument");
    RL_REQUIRE(horizon > 0 && horizon < (1ull << 31), "bad horizon");
    rl_engine *e = q->eng;
    uint64_t N = q->rp.N;
    q->mem.ensure(q->d_flags, horizon * N);
    // DqnAgent::actor(Training) (dqn.rs:200-211) + Bernoulli::new(p) of rand 0.8.5: p_int = (p * 2^64) as u64,
    // p == 1.0 always true without a draw
    double eps = dqn_exploration_rate(q, true);
    RL_REQUIRE(eps >= 0.0 && eps <= 1.0, "exploration rate outside [0, 1]");
    int always = rl_bernoulli_always(eps);
    uint64_t p_int = always ? ~0ull : rl_bernoulli_p_int(eps);
    if (q->recurrent) {
      launch_stack_collect_dqn(q->env, q->qnet, q->roll, q->rp, (uint32_t)horizon, p_int, always, q->d_flags);
    } else if (q->qnet->general) {
      if (!q->d_q) q->d_q = q->mem.alloc<float>((size_t)q->A * q->rp.N);
      launch_rollout_dqn_general(q->env, q->qnet, q->mb, q->d_q, q->rp, (uint32_t)horizon, p_int, always, q->d_flags);
    } else {
      launch_rollout_dqn(q->env, q->qnet, q->rp, (uint32_t)horizon, p_int, always, q->d_flags, q->mb->d.range);
    }
    q->env->t_global += horizon;
    q->steps_per_lane += horizon;
    q->last_horizon = horizon;
    int32_t err = 0;
    d2h(e, &err, q->rp.error, sizeof(err));
    if (dqn_any_rank_failed(q, err != 0))
      throw RlError(RL_ERR_BUFFER_FULL, err != 0 ? "replay buffer full: an episode outgrew the lane capacity"
                                                 : "replay buffer full on another rank");
    if (stats) {
      std::vector<uint8_t> fl(horizon * N);
      d2h(e, fl.data(), q->d_flags, fl.size());
      uint64_t ended = 0;
      for (uint8_t f : fl) ended += f != RL_SUCC_CONTINUE;
      stats->exploration_rate = eps;
      stats->steps = horizon * N;
      stats->episodes_ended = ended;
    }
  });
}

static AgentKey dqn_key(const rl_dqn *q) {
  AgentKey k;
  std::memcpy(k.w, q->cfg.agent_key, sizeof(k.w));
  return k;
}

// the sampler's verdict on `n` minibatches: RL_OK, or the first failure and what it was
static int32_t dqn_check_counts(const rl_dqn *q, const DqnCountsDev *counts, size_t n, const char **what) {
  for (size_t i = 0; i < n; ++i) {
    const DqnCountsDev &c = counts[i];
    if (c.error == 2) {
      *what = "minibatch sampling from a lane without a complete episode";
      return RL_ERR_INVALID_ARGUMENT;
    } else if (c.error != 0) {
      *what = "replay buffer full";
      return RL_ERR_BUFFER_FULL;
    } else if (c.n_eps > q->max_eps || c.n_steps > q->max_steps_mb) {
      *what = "minibatch exceeds its workspace";
      return RL_ERR_INVALID_ARGUMENT;
    } else if (c.n_steps == 0) {
      *what = "empty minibatch";
      return RL_ERR_INVALID_ARGUMENT;
    }
  }
  return RL_OK;
}

// the episode lists of minibatch `k` of the last draw
static EpisodeLists dqn_lists(const rl_dqn *q, uint64_t k) {
  const size_t o = (size_t)k * q->max_eps;
  return EpisodeLists{q->eps.lane + o, q->eps.start + o, q->eps.len + o, q->eps.off + o};
}

// draw the episode lists of `n_batches` consecutive minibatches (dqn.rs:280-291) in one launch and read back their
// sizes: the draws do not depend on the network, so the whole update needs this one host round trip
static void dqn_draw_minibatches(rl_dqn *q, int sequential, uint32_t n_batches, std::vector<DqnCountsDev> &counts,
                                 std::vector<uint64_t> &totals) {
  rl_engine *e = q->eng;
  launch_dqn_sample(e, e->stream, q->rp, dqn_key(q), q->d_agent_pos, (uint32_t)q->cfg.minibatch_steps, q->max_eps,
                    dqn_lists(q, 0), q->d_counts, sequential, n_batches);
  // (a recurrent agent lays a minibatch out by its longest episode: the length rides in the counts' spare word)
  if (q->recurrent) launch_dqn_longest(e, dqn_lists(q, 0), q->max_eps, q->d_counts, n_batches);
  counts.resize(n_batches);
  d2h(e, counts.data(), q->d_counts, n_batches * sizeof(DqnCountsDev));
  // local validation first, the verdict only after every rank has reported (a rank that throws here alone would leave
  // its peers blocked in the count all-reduce below)
  const char *what = "";
  const int32_t code = dqn_check_counts(q, counts.data(), counts.size(), &what);
  if (dqn_any_rank_failed(q, code != RL_OK))
    throw RlError(code != RL_OK ? code : RL_ERR_COMM, code != RL_OK ? what : "minibatch sampling failed on another rank");
  // the loss is a mean over all ranks' samples: sum the per-rank counts (two 16-bit halves each, exact in f32)
  totals.resize(n_batches);
  for (uint32_t k = 0; k < n_batches; ++k) totals[k] = counts[k].n_steps;
  if (e->n_ranks > 1) {
    std::vector<float> halves(2 * n_batches);
    for (uint32_t k = 0; k < n_batches; ++k) {
      halves[2 * k] = (float)(counts[k].n_steps & 0xffffu);
      halves[2 * k + 1] = (float)(counts[k].n_steps >> 16);
    }
    RL_REQUIRE(2 * n_batches <= q->mb->Pmax, "too many minibatches for the exchange buffer");
    h2d(e, q->mb->vec, halves.data(), halves.size() * sizeof(float));
    rl_allreduce_sum_f32(e, q->mb->vec, halves.size());
    d2h(e, halves.data(), q->mb->vec, halves.size() * sizeof(float));
    for (uint32_t k = 0; k < n_batches; ++k) totals[k] = (uint64_t)halves[2 * k] + ((uint64_t)halves[2 * k + 1] << 16);
  }
}

// ---------------------------------------------------------------- the current minibatch
// Which minibatch the workspace holds, for rl_dqn_minibatch_read / _gradient and the update's statistics.  Set: minibatch
// `k` of the last draw — c.n_steps steps here, `total` over all ranks — with `mb` planned to its size.  Cleared: none;
// the readers refuse, and `mb` points back at its own sample arrays (an all-at-once update leaves it looking at its last
// minibatch inside the big arrays; the pointers are views: destroying `mb` frees nothing it does not own, DevMem).
static void dqn_set_current(rl_dqn *q, uint64_t k, const DqnCountsDev &c, uint64_t total) {
  q->last_n_eps = c.n_eps;
  q->last_n_steps = c.n_steps;
  q->last_total_steps = total;
  q->last_batch_index = (uint32_t)k;
  q->last_longest = c.pad;  // (a recurrent agent's draw: launch_dqn_longest)
  q->mb->d.n = c.n_steps;
  q->mb->d.T = 1;
  traj_plan(q->mb, c.n_steps);
}
static void dqn_clear_current(rl_dqn *q) {
  q->mb->d.obs = q->own_obs;
  q->mb->d.adv = q->own_target;
  q->mb->d.action = q->own_action;
  q->mb->d.flag = q->own_flag;
  q->td_in_kernel = false;
  q->last_n_eps = q->last_n_steps = 0;
}

// gather minibatch `k` of the last draw into the workspace's own arrays, as the only minibatch of the all-at-once
// builder: with its reward-to-go targets, or (`td`) with rewards, successor codes and successor observations (time slot
// 1) for one-step TD targets formed behind it
static void dqn_gather_one(rl_dqn *q, uint32_t k, const DqnCountsDev &c, bool td) {
  rl_traj *mb = q->mb;
  launch_dqn_build_all(q->eng, q->rp, 1, c.n_eps, q->max_eps, dqn_lists(q, k), q->d_counts + k, mb->d.obs, 0,
                       mb->d.action, mb->d.adv, 0, q->cfg.discount_factor, td ? mb->d.flag : (uint8_t *)nullptr);
}

// ---------------------------------------------------------------- a recurrent action-value module
// (rl_dqn_create_recurrent; the workspace's layout and its kernels: kernels_dqn.hip, the forward / backward:
// kernels_seq_stack.hip — every recurrent chain runs the lane-per-thread kernels here, at its own widths)

// seq_packed(observations) over the workspace (dqn.rs:316-318), with the activation record; `succ`: also the outputs at
// the successor observations of Interrupts (the extended sequence of the one-step TD targets)
static void rdqn_forward(rl_dqn *q, bool succ) {
  rl_traj *s = q->seq;
  launch_stack_forward(s, q->qnet, s->seq.out, succ ? s->seq.succ : (float *)nullptr, /*record=*/true, nullptr);
  q->seq_fwd_epoch = q->eng->call_epoch;
}

// gather minibatch `k` of the last draw — episode after episode into `mb` (what rl_dqn_minibatch_read serves), one
// episode per lane column into `seq` — and compute its targets (dqn.rs:293-314).  No minibatch is current until the
// workspace is whole.
static void rdqn_build_minibatch(rl_dqn *q, uint32_t k, const DqnCountsDev &c, uint64_t total) {
  rl_traj *mb = q->mb, *s = q->seq;
  const bool td = q->cfg.target == RL_DQN_TARGET_ONE_STEP_TD;
  dqn_gather_one(q, k, c, td);
  const uint64_t n = c.n_eps, T = c.pad, B = n * T, Dp = q->rp.D > 5 ? q->rp.D : 5;
  RL_REQUIRE(T > 0 && T <= q->rp.C && B >= c.n_steps, "minibatch without its longest episode's length");
  RL_REQUIRE(Dp * (T + 1) * n < (1ull << 31), "recurrent minibatch workspace: episodes x longest episode too large");
  s->d.n = (uint32_t)n;
  s->d.T = (uint32_t)T;
  DevMem &mem = s->mem;
  mem.ensure(s->d.obs, Dp * (T + 1) * n);
  mem.ensure(s->d.term_obs, Dp * B);
  mem.ensure(s->d.action, B);
  mem.ensure(s->d.flag, B);
  mem.ensure(s->d.reward, B);
  mem.ensure(s->d.adv, B);
  mem.ensure(s->dz, (uint64_t)q->A * B);
  traj_plan(s, B);
  stack_ensure(s, q->qnet, true);
  const EpisodeLists eps = dqn_lists(q, k);
  launch_dqn_build_seq(s, q->rp, eps, td ? (const float *)nullptr : mb->d.adv);
  q->seq_fwd_epoch = 0;
  if (td) {  // under no_grad with the parameters of this optimisation step (dqn.rs:299-311): the forward the gradient reuses
    rdqn_forward(q, true);
    launch_dqn_seq_td_targets(s, eps, q->A, q->cfg.discount_factor, mb->d.adv);
  }
  dqn_set_current(q, k, c, total);
}

// gradient of mean((Q(s)[a] - target)^2) over the sampled steps of the current minibatch -> seq->vec[0..P), loss sum ->
// seq->vec[P]; `step_opt`: also the optimiser's step, the loss into slot `loss_slot` of seq->losses
static void rdqn_gradient(rl_dqn *q, rl_adam *step_opt, int loss_slot) {
  rl_traj *s = q->seq;
  const uint32_t P = (uint32_t)q->qnet->P;
  if (q->seq_fwd_epoch != q->eng->call_epoch) rdqn_forward(q, false);
  launch_dqn_seq_terms(s, dqn_lists(q, q->last_batch_index), q->A, q->last_total_steps);
  launch_stack_backward(s, q->qnet, nullptr);
  launch_reduce(s, P, false, true, 0, s->nbB);
  if (step_opt) {
    launch_opt_step(s, step_opt, loss_slot, q->last_total_steps);
    q->seq_fwd_epoch = 0;  // (the outputs are those of the parameters before the step)
  }
}

// gather minibatch `k` of the last draw and compute its targets (dqn.rs:293-314)
static void dqn_build_minibatch(rl_dqn *q, uint32_t k, const DqnCountsDev &c, uint64_t total) {
  dqn_clear_current(q);
  if (q->recurrent) return rdqn_build_minibatch(q, k, c, total);
  dqn_set_current(q, k, c, total);
  rl_traj *mb = q->mb;
  const bool td = q->cfg.target == RL_DQN_TARGET_ONE_STEP_TD;
  if (td && q->qnet->general) {
    // the builder's in-kernel forward is the fused module's; any other module: gather with rewards, successor codes and
    // successor observations, the module's layer kernels over the successor observations, then the targets
    dqn_gather_one(q, k, c, true);
    q->mem.ensure(q->d_q_next, (uint64_t)q->A * q->max_steps_mb);  // (c.n_steps <= max_steps_mb: allocated once)
    launch_gen_forward(mb, q->qnet, mb->d.obs + c.n_steps, (size_t)2 * c.n_steps, c.n_steps, q->d_q_next);
    launch_dqn_td_targets(q->eng, mb->d.adv, mb->d.flag, q->d_q_next, c.n_steps, q->A, q->cfg.discount_factor);
    return;
  }
  launch_dqn_build_minibatch(q->eng, q->rp, c.n_eps, dqn_lists(q, k), mb->d.obs, (size_t)2 * c.n_steps, mb->d.action,
                             mb->d.adv, q->cfg.discount_factor, td ? 1 : 0, q->qnet);
}


// gradient of mean((Q(s)[a] - target)^2) over the current minibatch -> mb->vec[0..P), loss sum -> mb->vec[P]
// `step_opt` != nullptr: also take the optimiser step, recording the loss in slot `loss_slot`; without an all-reduce
// between them the reduction and the (elementwise) step are one launch
static void dqn_gradient(rl_dqn *q, rl_adam *step_opt = nullptr, int loss_slot = -1) {
  if (q->recurrent) return rdqn_gradient(q, step_opt, loss_slot);
  rl_traj *mb = q->mb;
  // targets given (reward-to-go, or one-step TD built beforehand): two critic-step channels per SIMD
  // (kernels_critic.hip, k_critic_step_mfma<2>); targets formed inside the launch (one-step TD on the current network):
  // k_dqn_step_bf16
  bool fused = false;
  if (q->eng->kernel_variant == 0)
    fused = q->td_in_kernel ? launch_dqn_step_bf16(mb, q->qnet, q->last_total_steps, q->cfg.discount_factor)
                            : launch_dqn_step_pair(mb, q->qnet, q->last_total_steps);
  // the other kernels: the RUN_DQN row of the update passes (abi_update.hip), up to the slabs.  (A drawn minibatch has
  // at least one step, so the count is never the 0 that would ask for the workspace's own.)
  PassRequest pass(RUN_DQN);
  pass.B_total = q->last_total_steps;
  pass.reduce = false;
  // (the two fused launchers report their rows in nbV2)
  const SlabRows rows = fused ? SlabRows{mb->nbV2, mb->nbV2} : run_pass(q->qnet, mb, pass);
  if (step_opt && !q->eng->has_collective()) {
    launch_reduce_opt(mb, step_opt, rows.A, rows.B, loss_slot, q->last_total_steps);
    return;
  }
  const uint32_t P = (uint32_t)q->qnet->P;
  launch_reduce(mb, P, true, true, rows.A, rows.B);
  rl_allreduce_sum_f32(q->eng, mb->vec, P + 4);
  if (step_opt) launch_opt_step(mb, step_opt, loss_slot, q->last_total_steps);
}

// What an all-or-nothing update puts back when it fails: the parameters, every state slot the optimiser's rule has (none
// for plain SGD, three for centered RMSProp with momentum) and the step count, on the device and on the host, as of
// save().  Held by the update, which restores in its `catch` — not from a destructor: nothing here runs while another
// exception unwinds.  (A few device copies of <= 4 KB each, in q->snap.)
struct DqnSnapshot {
  bool saved = false;
  uint64_t host_step = 0;
  // the copies of either direction on the engine's stream; the first failure
  static hipError_t copy(rl_dqn *q, bool restore) {
    const uint64_t P = q->qnet->P;
    hipError_t err = hipSuccess;
    auto cp = [&](void *live, float *kept, size_t bytes) {
      const hipError_t r = hipMemcpyAsync(restore ? live : (void *)kept, restore ? (const void *)kept : live, bytes,
                                          hipMemcpyDeviceToDevice, q->eng->stream);
      if (err == hipSuccess) err = r;
    };
    cp(q->qnet->d_params, q->snap, P * sizeof(float));
    size_t slot = 1;  // (of P floats in q->snap: the parameters, one per state slot, then the step count)
    for (float *state : q->opt->d_state) {
      if (state) cp(state, q->snap + slot * P, P * sizeof(float));
      ++slot;
    }
    cp(q->opt->d_step, q->snap + slot * P, sizeof(uint64_t));
    return err;
  }
  void save(rl_dqn *q) {
    if (!q->snap) q->snap = q->mem.alloc<float>((std::size(q->opt->d_state) + 1) * q->qnet->P + 2);
    RL_HIP_CHECK(copy(q, false));
    host_step = q->opt->host_step;
    saved = true;
  }
  void restore(rl_dqn *q) {
    if (!saved) return;
    (void)copy(q, true);
    wimg_invalidate(q->qnet);
    (void)hipStreamSynchronize(q->eng->stream);
    q->opt->host_step = host_step;
  }
};

// DqnAgent::batch_update (dqn.rs:270-340): opt_steps_per_update x {sample_minibatch; gradient; optimiser step}, all or
// nothing.  The draws do not depend on the network, so the episode lists come from the sampler ahead of the steps and
// their sizes are the update's only read-backs.  What differs between the agents is decided once, at the top:
//   all_at_once  feed-forward, reward-to-go targets (or one-step TD targets the fused 5-128-2 gradient kernel forms itself
//                from the successor observations in time slot 1): a chunk's minibatches are gathered in one launch
//   pipelined    ... on one rank, not profiling: the draws — one sequential chain through the agent's Prng, 12 us per
//                minibatch on one CU — run on a second stream in chunks of 2, 4, 8, ... minibatches while the main stream
//                trains on the chunks already drawn (the draw is the faster: only the first chunk is waited for)
//   otherwise    one draw launch, which validates every minibatch before the first step; minibatches are built one at a
//                time with the parameters of their step.  A recurrent agent (one rank) walks the 2, 4, 8, ... chunks too.
// RELEARN_DQN_FAIL_CHUNK=c (test facility, tests/test_gpu_dqn.py) fails chunk c of a chunked update as a sampler error would.
int32_t rl_dqn_update(rl_dqn *q, rl_dqn_update_stats *stats, float *losses_out) {
  return guarded(q ? q->eng : nullptr, [&] {
    RL_REQUIRE(q, "NULL argument");
    rl_engine *e = q->eng;
    const bool rec = q->recurrent;
    if (rec && e->n_ranks > 1)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_dqn_update: an agent of rl_dqn_create_recurrent updates on one rank");
    // self.global_steps = sum of total_step_count over the buffers (dqn.rs:276); every lane of every rank has
    // taken the same number of steps and the horizon rule drops none
    q->global_steps = q->steps_per_lane * (uint64_t)q->rp.N * (uint64_t)e->n_ranks;
    const uint64_t K = q->cfg.opt_steps_per_update, D = q->rp.D, cap = q->max_steps_mb;
    const bool td = q->cfg.target == RL_DQN_TARGET_ONE_STEP_TD;
    // Do the fused 5-128-2 kernels take this handle's minibatches?  Asked once per update, before the minibatch sizes
    // are known: without the element-offset term, which the launchers test per minibatch.  (Two outputs and a
    // feed-forward module are rl_dqn_create's conditions; the workspace has the store's D features.)
    const bool fused_shape = e->kernel_variant == 0 && fused_5_128_fits(q->mb, q->qnet, 2, /*offsets=*/false);
    const bool all_at_once = !rec && K > 1 && (!td || fused_shape) && K * cap * (8 * D + 6) <= (8ull << 30);
    const bool pipelined = all_at_once && e->n_ranks == 1 && !e->profiling;
    const bool chunked = pipelined || rec;
    if (all_at_once) {  // (allocated by the first such update: K and cap are the handle's constants)
      q->mem.ensure(q->all_obs, K * D * 2 * cap);
      q->mem.ensure(q->all_target, K * cap);
      q->mem.ensure(q->all_action, K * cap);
      if (td) q->mem.ensure(q->all_flag, K * cap);
    }
    std::vector<DqnCountsDev> counts;
    std::vector<uint64_t> totals;
    std::vector<uint32_t> chunk_end;  // minibatches [chunk_end[c - 1], chunk_end[c]) form chunk c
    if (chunked)
      for (uint64_t first = 0, size = 2; first < K; first += size, size *= 2)
        chunk_end.push_back((uint32_t)(first + size < K ? first + size : K));
    else
      chunk_end.push_back((uint32_t)K);
    if (pipelined) {
      if (!q->draw_stream) RL_HIP_CHECK(hipStreamCreateWithFlags(&q->draw_stream, hipStreamNonBlocking));
      if (!q->main_event) RL_HIP_CHECK(hipEventCreateWithFlags(&q->main_event, hipEventDisableTiming));
      if (!q->h_counts) q->h_counts = q->mem.alloc_host<DqnCountsDev>(K, /*mapped=*/false);
      while (q->draw_events.size() < chunk_end.size()) {
        hipEvent_t ev;
        RL_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        q->draw_events.push_back(ev);
      }
      // the store is as the main stream's collection left it
      RL_HIP_CHECK(hipEventRecord(q->main_event, e->stream));
      RL_HIP_CHECK(hipStreamWaitEvent(q->draw_stream, q->main_event, 0));
      for (size_t c = 0; c < chunk_end.size(); ++c) {
        const uint32_t first = c ? chunk_end[c - 1] : 0, size = chunk_end[c] - first;
        launch_dqn_sample(e, q->draw_stream, q->rp, dqn_key(q), q->d_agent_pos, (uint32_t)q->cfg.minibatch_steps,
                          q->max_eps, dqn_lists(q, first), q->d_counts + first, 0, size);
        RL_HIP_CHECK(hipMemcpyAsync(q->h_counts + first, q->d_counts + first, size * sizeof(DqnCountsDev),
                                    hipMemcpyDeviceToHost, q->draw_stream));
        RL_HIP_CHECK(hipEventRecord(q->draw_events[c], q->draw_stream));
      }
      counts.resize(K);
      totals.resize(K);
    } else if (K) {  // (the one-launch draw validates every minibatch before the first step)
      dqn_draw_minibatches(q, 0, (uint32_t)K, counts, totals);
    }
    // All or nothing.  With pipelined draws a sampler error can surface in a LATER chunk, after the earlier chunks'
    // optimisation steps have run; the fused gradient kernel's range guard reports after the steps it could not vouch
    // for have run; a recurrent update's launches fail where the stream is drained.
    DqnSnapshot snapshot;
    if (chunked || fused_shape) snapshot.save(q);
    try {
      for (size_t c = 0; c < chunk_end.size(); ++c) {
        const uint32_t first = c ? chunk_end[c - 1] : 0, size = chunk_end[c] - first;
        if (pipelined) {
          RL_HIP_CHECK(hipEventSynchronize(q->draw_events[c]));
          const char *what = "";
          const int32_t code = dqn_check_counts(q, q->h_counts + first, size, &what);
          if (code != RL_OK) throw RlError(code, what);
        }
        if (chunked)
          if (const char *inj = std::getenv("RELEARN_DQN_FAIL_CHUNK"))
            if ((size_t)std::atoi(inj) == c) throw RlError(RL_ERR_INVALID_ARGUMENT, "injected sampler failure");
        if (pipelined)
          for (uint32_t k = first; k < first + size; ++k) {
            counts[k] = q->h_counts[k];
            totals[k] = counts[k].n_steps;
          }
        if (all_at_once && size) {
          uint32_t widest = 0;
          for (uint32_t k = first; k < first + size; ++k) widest = counts[k].n_eps > widest ? counts[k].n_eps : widest;
          launch_dqn_build_all(e, q->rp, size, widest, q->max_eps, dqn_lists(q, first), q->d_counts + first,
                               q->all_obs + first * D * 2 * cap, (size_t)(D * 2 * cap), q->all_action + first * cap,
                               q->all_target + first * cap, (size_t)cap, q->cfg.discount_factor,
                               td ? q->all_flag + first * cap : (uint8_t *)nullptr);
        }
        for (uint64_t k = first; k < first + size; ++k) {
          if (all_at_once) {
            rl_traj *mb = q->mb;
            dqn_set_current(q, k, counts[k], totals[k]);
            mb->d.obs = q->all_obs + k * D * 2 * cap;
            mb->d.action = q->all_action + k * cap;
            mb->d.adv = q->all_target + k * cap;
            if (td) mb->d.flag = q->all_flag + k * cap;
            q->td_in_kernel = td;
          } else {
            dqn_build_minibatch(q, (uint32_t)k, counts[k], totals[k]);
          }
          dqn_gradient(q, q->opt, (int)k);
        }
      }
      // a launch that failed surfaces here, inside the all-or-nothing scope; so does the range guard's word (the stream
      // is drained first: the word is host memory the kernels write across the bus)
      if (rec || (fused_shape && K)) sync(e);
      if (fused_shape && K) range_check(q->mb, 1u << RL_GUARD_POLICY);
    } catch (...) {
      if (pipelined) (void)hipStreamSynchronize(q->draw_stream);  // the later chunks' draws still advance the agent's Prng
      snapshot.restore(q);
      dqn_clear_current(q);  // no minibatch to read after a failed update
      throw;
    }
    // (after an all-at-once update `mb` keeps looking at the last minibatch: rl_dqn_minibatch_read / _gradient work;
    // with in-kernel TD targets the workspace holds rewards, not targets: the last minibatch is built once more by the
    // one-at-a-time builder, with the targets of the parameters the update ends on)
    if (all_at_once && td && K) dqn_build_minibatch(q, (uint32_t)(K - 1), counts[K - 1], totals[K - 1]);
    std::vector<float> h(K ? K : 1, 0.0f);
    if (K) d2h(e, h.data(), (rec ? q->seq : q->mb)->losses, K * sizeof(float));
    if (!rec) range_check(q->mb, 1u << RL_GUARD_POLICY);
    if (losses_out && K) std::memcpy(losses_out, h.data(), K * sizeof(float));
    if (stats) {
      stats->opt_steps = K;
      stats->loss_first = K ? (double)h[0] : 0.0;
      stats->loss_last = K ? (double)h[K - 1] : 0.0;
      stats->global_steps = q->global_steps;
      stats->last_minibatch_steps = q->last_n_steps;
      stats->last_minibatch_episodes = q->last_n_eps;
    }
  });
}


static void replay_field(const rl_dqn *q, int32_t field, void **ptr, uint64_t *bytes) {
  const ReplayDev &r = q->rp;
  uint64_t N = r.N, C = r.C, E = r.E, D = r.D;
  *ptr = nullptr;
  switch (field) {
    case RL_REPLAY_HEAD: *ptr = r.head; *bytes = N * 4; break;
    case RL_REPLAY_COUNT: *ptr = r.count; *bytes = N * 4; break;
    case RL_REPLAY_EP_HEAD: *ptr = r.ep_head; *bytes = N * 4; break;
    case RL_REPLAY_EP_COUNT: *ptr = r.ep_count; *bytes = N * 4; break;
    case RL_REPLAY_TOTAL: *ptr = r.total; *bytes = N * 4; break;
    case RL_REPLAY_EP_END: *ptr = r.ep_end; *bytes = E * N * 4; break;
    // step data lives in records (engine.hpp): *ptr stays NULL, the read goes through launch_replay_planes
    case RL_REPLAY_OBS: *bytes = D * C * N * 4; break;
    case RL_REPLAY_NEXT_OBS: *bytes = D * C * N * 4; break;
    case RL_REPLAY_ACTION: *bytes = C * N; break;
    case RL_REPLAY_REWARD: *bytes = C * N * 4; break;
    case RL_REPLAY_FLAG: *bytes = C * N; break;
    case RL_REPLAY_ACTOR_POS: *ptr = r.actor_pos; *bytes = N * 8; break;
    case RL_REPLAY_LAST_FLAGS: *ptr = q->d_flags; *bytes = q->last_horizon * N; break;
    default: throw RlError(RL_ERR_INVALID_ARGUMENT, "unknown replay field");
  }
}

int32_t rl_dqn_replay_field_bytes(const rl_dqn *q, int32_t field, uint64_t *bytes) {
  return guarded(q ? q->eng : nullptr, [&] {
    RL_REQUIRE(q && bytes, "NULL argument");
    void *p;
    replay_field(q, field, &p, bytes);
  });
}

int32_t rl_dqn_replay_read(rl_dqn *q, int32_t field, void *host, uint64_t bytes) {
  return guarded(q ? q->eng : nullptr, [&] {
    RL_REQUIRE(q && host, "NULL argument");
    void *p;
    uint64_t need;
    replay_field(q, field, &p, &need);
    RL_REQUIRE(bytes == need, "byte count mismatch for replay field");
    if (!bytes) return;
    if (p) {
      d2h(q->eng, host, p, bytes);
      return;
    }
    RL_HIP_CHECK(hipSetDevice(q->eng->device));
    DevMem tmp;
    void *planes = tmp.alloc<uint8_t>(bytes);
    launch_replay_planes(q->eng, q->rp, field, planes);
    d2h(q->eng, host, planes, bytes);
  });
}

int32_t rl_dqn_minibatch_sample(rl_dqn *q, int32_t sequential, uint64_t *n_episodes_out, uint64_t *n_steps_out) {
  return guarded(q ? q->eng : nullptr, [&] {
    RL_REQUIRE(q, "NULL argument");
    std::vector<DqnCountsDev> counts;
    std::vector<uint64_t> totals;
    dqn_draw_minibatches(q, sequential, 1, counts, totals);
    dqn_build_minibatch(q, 0, counts[0], totals[0]);
    if (n_episodes_out) *n_episodes_out = q->last_n_eps;
    if (n_steps_out) *n_steps_out = q->last_n_steps;
  });
}

int32_t rl_dqn_minibatch_read(rl_dqn *q, int32_t field, void *host, uint64_t bytes) {
  return guarded(q ? q->eng : nullptr, [&] {
    RL_REQUIRE(q && host, "NULL argument");
    uint64_t ne = q->last_n_eps, ns = q->last_n_steps, D = q->rp.D;
    RL_REQUIRE(ns > 0, "no minibatch has been sampled");
    rl_engine *e = q->eng;
    switch (field) {
      case RL_MB_EP_LANE:
      case RL_MB_EP_START:
      case RL_MB_EP_LEN:
      case RL_MB_EP_OFFSET: {
        const EpisodeLists ep = dqn_lists(q, q->last_batch_index);
        RL_REQUIRE(bytes == ne * 4, "byte count mismatch");
        d2h(e, host, field == RL_MB_EP_LANE ? ep.lane : field == RL_MB_EP_START ? ep.start : field == RL_MB_EP_LEN ? ep.len : ep.off,
            bytes);
        break;
      }
      case RL_MB_OBS: {
        RL_REQUIRE(bytes == D * ns * 4, "byte count mismatch");
        // feature planes are 2 * n_steps apart in the workspace (T = 1 trajectory layout)
        for (uint64_t d = 0; d < D; ++d)
          d2h(e, (char *)host + d * ns * 4, q->mb->d.obs + d * 2 * ns, ns * 4);
        break;
      }
      case RL_MB_ACTION: RL_REQUIRE(bytes == ns, "byte count mismatch"); d2h(e, host, q->mb->d.action, bytes); break;
      case RL_MB_TARGET: RL_REQUIRE(bytes == ns * 4, "byte count mismatch"); d2h(e, host, q->mb->d.adv, bytes); break;
      default: throw RlError(RL_ERR_INVALID_ARGUMENT, "unknown minibatch field");
    }
  });
}

int32_t rl_dqn_minibatch_gradient(rl_dqn *q, float *grad_out, float *loss_out) {
  return guarded(q ? q->eng : nullptr, [&] {
    RL_REQUIRE(q && grad_out, "NULL argument");
    RL_REQUIRE(q->last_n_steps > 0, "no minibatch has been sampled");
    uint32_t P = (uint32_t)q->qnet->P;
    dqn_gradient(q);
    std::vector<float> h(P + 4);
    d2h(q->eng, h.data(), (q->recurrent ? q->seq : q->mb)->vec, (P + 4) * sizeof(float));
    range_check(q->mb, 1u << RL_GUARD_POLICY);
    std::memcpy(grad_out, h.data(), P * sizeof(float));
    if (loss_out) *loss_out = (float)((double)h[P] / (double)q->last_total_steps);
  });
}

int32_t rl_dqn_agent_rng_pos(rl_dqn *q, uint64_t *pos_out) {
  return guarded(q ? q->eng : nullptr, [&] {
    RL_REQUIRE(q && pos_out, "NULL argument");
    d2h(q->eng, pos_out, q->d_agent_pos, sizeof(uint64_t));
  });
}

}  // extern "C"
