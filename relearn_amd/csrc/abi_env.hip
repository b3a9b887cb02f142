// abi_env.hip — extern "C" entry points of include/relearn_hip.h, part: environments.  What a constructor decides is
// handle_spec.hpp (the env_spec_* functions); env_build here is what it allocates.
#include "abi_internal.hpp"
#include "env_lanes.hpp"

extern "C" {

// ---------------------------------------------------------------- env
int32_t rl_cartpole_params_default(rl_cartpole_params *p) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(p, "params is NULL");
    // PhysicalConstants::default / EnvironmentParams::default (reference src/envs/cartpole.rs:178-216)
    p->gravity = 9.8;
    p->mass_cart = 1.0;
    p->mass_pole = 0.1;
    p->length_half_pole = 0.5;
    p->friction_cart = 0.01;
    p->friction_pole = 0.01;
    p->time_step = 0.02;
    p->action_force = 10.0;
    p->max_pos = 2.4;
    p->max_angle = 12.0 * (3.14159265358979323846 / 180.0);  // 12.0f64.to_radians()
    p->discount_factor = 0.99;
  });
}

// The allocating half of every env constructor (what `spec` holds was decided and checked in handle_spec.hpp: nothing is
// refused from here on, only a HIP call can fail).  `e` and `out` not NULL.
static void env_build(rl_engine *e, const EnvSpec &spec, rl_env **out) {
  RL_HIP_CHECK(hipSetDevice(e->device));
  std::unique_ptr<rl_env> env(new rl_env());
  env->eng = e;
  env->cfg = spec.cfg;
  env->kind = spec.cfg.kind;
  env->D = spec.D;
  env->A = spec.A;
  env->dev = spec.dev;
  const size_t n = spec.cfg.n_lanes;
  DevMem &mem = env->mem;
  env->st.x = mem.alloc<double>(n);
  env->st.xdot = mem.alloc<double>(n);
  env->st.th = mem.alloc<double>(n);
  env->st.thdot = mem.alloc<double>(n);
  env->st.nv_pos = mem.alloc<uint8_t>(n);
  env->st.steps_remaining = mem.alloc<uint32_t>(n);
  env->st.reset_count = mem.alloc<uint32_t>(n);
  env->d_actions = mem.alloc<uint8_t>(n);
  env->d_flag = mem.alloc<uint8_t>(n);
  env->d_reward = mem.alloc<float>(n);
  env->d_obs = mem.alloc<float>(n * env->D);
  env->d_term_obs = mem.alloc<float>(n * env->D);
  if (spec.mdp.S != 0) {
    // the tables: one allocation of the handle, the f64 tables first so that both are aligned
    const MdpTables &t = spec.mdp;
    const size_t rows = (size_t)t.S * t.A, bytes = rows * 16 + rows * t.S * sizeof(float);
    uint8_t *tab = mem.alloc<uint8_t>(bytes);
    std::vector<uint8_t> img(bytes);
    std::memcpy(img.data(), t.mean.data(), rows * 8);
    std::memcpy(img.data() + rows * 8, t.stddev.data(), rows * 8);
    std::memcpy(img.data() + rows * 16, t.cum.data(), rows * t.S * sizeof(float));
    h2d(e, tab, img.data(), bytes);
    env->dev.mdp.mean = reinterpret_cast<const double *>(tab);
    env->dev.mdp.stddev = reinterpret_cast<const double *>(tab + rows * 8);
    env->dev.mdp.cum = reinterpret_cast<const float *>(tab + rows * 16);
  }
  if (spec.meta_mdp_rows != 0) {
    // every lane's own tables, written by the lanes' reset below: one allocation of the handle, the rows
    // of running sums first — 32 bytes each from an aligned base, so both 16-byte halves of a row are aligned — then the
    // f64 means
    // (above eight states a row is sixteen floats, 64 bytes: meta_mdp_row_floats)
    const size_t rows = n * spec.meta_mdp_rows, row_bytes = meta_mdp_row_floats(spec.dev.mm.states) * sizeof(float);
    uint8_t *tab = mem.alloc<uint8_t>(rows * row_bytes + rows * sizeof(double));
    env->dev.mm.cum = reinterpret_cast<float *>(tab);
    env->dev.mm.mean = reinterpret_cast<double *>(tab + rows * row_bytes);
  }
  RL_HIP_CHECK(hipMemsetAsync(env->st.reset_count, 0, n * sizeof(uint32_t), e->stream));
  for (double *p : {env->st.x, env->st.xdot, env->st.th, env->st.thdot})
    RL_HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(double), e->stream));
  RL_HIP_CHECK(hipMemsetAsync(env->st.nv_pos, 0, n, e->stream));
  RL_HIP_CHECK(hipMemsetAsync(env->d_actions, 0, n, e->stream));
  RL_HIP_CHECK(hipMemsetAsync(env->d_term_obs, 0, n * env->D * sizeof(float), e->stream));
  launch_env_reset(env.get());
  sync(e);
  e->live_handles += 1;
  *out = env.release();
}

int32_t rl_env_create(rl_engine *e, const rl_env_config *cfg, rl_env **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && cfg && out, "NULL argument");
    *out = nullptr;
    env_build(e, env_spec_basic(*cfg), out);
  });
}

// UniformBernoulliBandits::default (bandits.rs:140-144), TrialEpisodeLimit::default (meta.rs:557-564)
int32_t rl_meta_bandit_config_default(rl_meta_bandit_config *meta) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(meta, "config is NULL");
    meta->n_arms = 2;
    meta->distribution = RL_BANDITS_UNIFORM_BERNOULLI;
    meta->episodes_per_trial = 10;
  });
}

static int32_t meta_bandit_create(rl_engine *e, const rl_env_config *cfg, const rl_meta_bandit_config *meta, bool wide,
                                  rl_env **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && cfg && meta && out, "NULL argument");
    *out = nullptr;
    env_build(e, env_spec_meta(*cfg, *meta, wide), out);
  });
}

// MetaEnv::new(distribution).wrap(TrialEpisodeLimit::new(episodes_per_trial)) (meta.rs:128-203, 541-617)
int32_t rl_env_create_meta_bandit(rl_engine *e, const rl_env_config *cfg, const rl_meta_bandit_config *meta,
                                  rl_env **out) {
  return meta_bandit_create(e, cfg, meta, false, out);
}

// The same lanes at 2..12 arms (6..16 observation features).  Two to four arms: the older constructor, the same handle.
// Above four, the lanes serve what takes their width: the standalone env calls, recurrent chains of
// rl_rnn_chain_create_wide (rl_rollout and every update on what it collected) and rl_bandit_agent_*; feed-forward
// modules of more than eight inputs do not build, and DQN, rl_env_get_state / rl_env_set_state and actor documents
// refuse every meta lane by name.
int32_t rl_env_create_meta_bandit_wide(rl_engine *e, const rl_env_config *cfg, const rl_meta_bandit_config *meta,
                                       rl_env **out) {
  return meta_bandit_create(e, cfg, meta, true, out);
}

int32_t rl_env_create_bandit(rl_engine *e, const rl_env_config *cfg, const double *values, uint32_t n_arms,
                             rl_env **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && cfg && values && out, "NULL argument");
    *out = nullptr;
    env_build(e, env_spec_bandit(*cfg, values, n_arms), out);
  });
}

// TabularMdp<_, Normal<f64>> (src/envs/mdps.rs:12-85) under the index lanes' step limit
int32_t rl_env_create_tabular_mdp(rl_engine *e, const rl_env_config *cfg, const rl_tabular_mdp_config *mdp,
                                  const float *transitions, const double *reward_mean, const double *reward_stddev,
                                  rl_env **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && cfg && mdp && transitions && reward_mean && out, "rl_env_create_tabular_mdp: NULL argument");
    *out = nullptr;
    env_build(e, env_spec_mdp(*cfg, *mdp, transitions, reward_mean, reward_stddev), out);
  });
}

// DirichletRandomMdps::default (mdps.rs:111-122) but for the sizes — 10 x 5 has 19 observation features, this constructor
// ends at 16 (rl_env_create_meta_mdp_wide takes it) — under a LatentStepLimit of 10 steps and TrialEpisodeLimit::default (meta.rs:557-564); reward stddev mdps.rs:163
int32_t rl_meta_mdp_config_default(rl_meta_mdp_config *meta) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(meta, "config is NULL");
    meta->n_states = 5;
    meta->n_actions = 5;
    meta->alpha = 1.0;
    meta->reward_prior_mean = 1.0;
    meta->reward_prior_stddev = 1.0;
    meta->reward_stddev = 1.0;
    meta->discount_factor = 1.0;
    meta->max_inner_steps = 10;
    meta->episodes_per_trial = 10;
  });
}

// MetaEnv::new(DirichletRandomMdps{..}.wrap(LatentStepLimit::new(L))).wrap(TrialEpisodeLimit::new(E))
int32_t rl_env_create_meta_mdp(rl_engine *e, const rl_env_config *cfg, const rl_meta_mdp_config *meta, rl_env **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && cfg && meta && out, "rl_env_create_meta_mdp: NULL argument");
    *out = nullptr;
    env_build(e, env_spec_meta_mdp(*cfg, *meta), out);
  });
}

// The same lanes at n_states 2..10 with S + A + 4 <= 20 features (DirichletRandomMdps::default is 10 x 5: 19).  Wherever
// rl_env_create_meta_mdp builds, this is that handle; at nine and ten states the rows of running sums have sixteen floats
// and the lanes run MetaMdpWideOps (env_lanes.hpp).
int32_t rl_env_create_meta_mdp_wide(rl_engine *e, const rl_env_config *cfg, const rl_meta_mdp_config *meta, rl_env **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && cfg && meta && out, "rl_env_create_meta_mdp_wide: NULL argument");
    *out = nullptr;
    env_build(e, env_spec_meta_mdp_wide(*cfg, *meta), out);
  });
}

// PartitionGame (src/envs/partition.rs) under the index lanes' step limit: PartitionOps (env_lanes.hpp)
int32_t rl_env_create_partition(rl_engine *e, const rl_env_config *cfg, rl_env **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && cfg && out, "rl_env_create_partition: NULL argument");
    *out = nullptr;
    env_build(e, env_spec_partition(*cfg), out);
  });
}

// the current trial's tables as the lanes read them: the padding of the rows' eight (or sixteen) floats is dropped
int32_t rl_env_meta_mdp_read_tables(rl_env *env, uint64_t first_lane, uint64_t n, float *cum_out, double *mean_out) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(env, "env is NULL");
    if (env->kind != RL_ENV_META_MDP)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_env_meta_mdp_read_tables is built for RL_ENV_META_MDP lanes");
    RL_REQUIRE(n >= 1 && first_lane < env->cfg.n_lanes && n <= env->cfg.n_lanes - first_lane,
               "rl_env_meta_mdp_read_tables: lanes outside the env");
    const size_t S = env->dev.mm.states, rows = S * env->dev.mm.actions;
    if (mean_out) d2h(env->eng, mean_out, env->dev.mm.mean + first_lane * rows, n * rows * sizeof(double));
    if (cum_out) {
      const size_t W = meta_mdp_row_floats(env->dev.mm.states);
      std::vector<float> padded(n * rows * W);
      d2h(env->eng, padded.data(), env->dev.mm.cum + first_lane * rows * W, padded.size() * sizeof(float));
      for (size_t r = 0; r < n * rows; ++r)
        for (size_t j = 0; j < S; ++j) cum_out[r * S + j] = padded[r * W + j];
    }
  });
}

// DirichletRandomMdps::default (mdps.rs:111-122)
int32_t rl_random_mdps_config_default(rl_random_mdps_config *cfg) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(cfg, "config is NULL");
    cfg->num_states = 10;
    cfg->num_actions = 5;
    cfg->transition_prior_dirichlet_alpha = 1.0;
    cfg->reward_prior_mean = 1.0;
    cfg->reward_prior_stddev = 1.0;
    cfg->discount_factor = 1.0;
  });
}

// DirichletRandomMdps::sample_environment (mdps.rs:151-170) on the host: one stream, consumed in the reference's order
int32_t rl_random_mdps_sample(const rl_random_mdps_config *cfg, uint64_t seed, uint64_t stream, float *transitions,
                              double *reward_mean) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(cfg && transitions && reward_mean, "rl_random_mdps_sample: NULL argument");
    // (the sampler is the host mirror's, host/envs.hpp: it needs no engine and no device; what it refuses is an
    // std::invalid_argument naming the field -> RL_ERR_INVALID_ARGUMENT)
    relearn::DirichletRandomMdps d;
    d.num_states = cfg->num_states;
    d.num_actions = cfg->num_actions;
    d.transition_prior_dirichlet_alpha = cfg->transition_prior_dirichlet_alpha;
    d.reward_prior_mean = cfg->reward_prior_mean;
    d.reward_prior_stddev = cfg->reward_prior_stddev;
    d.discount_factor = cfg->discount_factor;
    d.sample_tables(seed, stream, transitions, reward_mean);
  });
}

// Index::from_index of the env's action space: an index >= num_actions is no action
static void check_actions(const rl_env *env, const uint8_t *actions) {
  for (uint64_t i = 0; i < env->cfg.n_lanes; ++i)
    RL_REQUIRE(actions[i] < env->A, "action index outside the env's action space");
}

int32_t rl_env_destroy(rl_env *env) { return destroy_child(env); }

int32_t rl_env_dims(const rl_env *env, uint32_t *obs_dim, uint32_t *n_actions) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(env, "env is NULL");
    if (obs_dim) *obs_dim = env->D;
    if (n_actions) *n_actions = env->A;
  });
}

int32_t rl_env_reset(rl_env *env) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(env, "env is NULL");
    launch_env_reset(env);
  });
}

int32_t rl_env_observe(rl_env *env, float *obs_out) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(env && obs_out, "NULL argument");
    launch_env_observe(env, env->d_obs);
    d2h(env->eng, obs_out, env->d_obs, env->cfg.n_lanes * env->D * sizeof(float));
  });
}

// one thread per word: block = word / 16 of the stream, the word's position in it
__global__ void k_debug_stream_words(AgentKey key, uint64_t stream, uint64_t first_word, uint32_t n_words,
                                     uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_words) return;
  const uint64_t w = first_word + i;
  out[i] = stream_word(key.w, stream, w);
}

int32_t rl_debug_stream_words(rl_engine *engine, uint64_t seed, uint64_t stream, uint64_t first_word, uint32_t n_words,
                              uint32_t *words_out) {
  return guarded(engine, [&] {
    RL_REQUIRE(engine && words_out, "NULL argument");
    RL_REQUIRE(n_words > 0 && n_words <= (1u << 20), "n_words must be in [1, 2^20]");
    AgentKey key;
    rl_seed_from_u64(seed, key.w);
    DevMem tmp;
    uint32_t *d = tmp.alloc<uint32_t>(n_words);
    hipLaunchKernelGGL(k_debug_stream_words, dim3((n_words + 255) / 256), dim3(256), 0, engine->stream, key, stream,
                       first_word, n_words, d);
    RL_HIP_CHECK(hipGetLastError());
    d2h(engine, words_out, d, (size_t)n_words * sizeof(uint32_t));
  });
}

int32_t rl_env_upload_actions(rl_env *env, const uint8_t *actions) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(env && actions, "NULL argument");
    check_actions(env, actions);
    h2d(env->eng, env->d_actions, actions, env->cfg.n_lanes);
  });
}

int32_t rl_env_step_resident(rl_env *env) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(env, "env is NULL");
    launch_env_step(env);
    env->t_global += 1;
  });
}

int32_t rl_env_step(rl_env *env, const uint8_t *actions, float *reward_out, uint8_t *flag_out, float *obs_out,
                    float *term_obs_out) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(env && actions, "NULL argument");
    check_actions(env, actions);
    rl_engine *e = env->eng;
    size_t n = env->cfg.n_lanes;
    RL_HIP_CHECK(hipMemcpyAsync(env->d_actions, actions, n, hipMemcpyHostToDevice, e->stream));
    launch_env_step(env);
    env->t_global += 1;
    if (reward_out)
      RL_HIP_CHECK(hipMemcpyAsync(reward_out, env->d_reward, n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (flag_out) RL_HIP_CHECK(hipMemcpyAsync(flag_out, env->d_flag, n, hipMemcpyDeviceToHost, e->stream));
    if (obs_out)
      RL_HIP_CHECK(
          hipMemcpyAsync(obs_out, env->d_obs, n * env->D * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (term_obs_out)
      RL_HIP_CHECK(hipMemcpyAsync(term_obs_out, env->d_term_obs, n * env->D * sizeof(float), hipMemcpyDeviceToHost,
                                  e->stream));
    sync(e);
  });
}

int32_t rl_env_get_state(rl_env *env, double *state4, int32_t *nv_pos, uint64_t *steps_remaining,
                         uint64_t *reset_count) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(env && state4 && nv_pos && steps_remaining && reset_count, "NULL argument");
    if (env->kind == RL_ENV_META_BANDIT)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_env_get_state is not built for RL_ENV_META_BANDIT lanes");
    if (env->kind == RL_ENV_META_MDP)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_env_get_state is not built for RL_ENV_META_MDP lanes");
    if (env->kind == RL_ENV_PARTITION)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_env_get_state is not built for RL_ENV_PARTITION lanes");
    rl_engine *e = env->eng;
    size_t n = env->cfg.n_lanes;
    d2h(e, state4 + 0 * n, env->st.x, n * sizeof(double));
    d2h(e, state4 + 1 * n, env->st.xdot, n * sizeof(double));
    d2h(e, state4 + 2 * n, env->st.th, n * sizeof(double));
    d2h(e, state4 + 3 * n, env->st.thdot, n * sizeof(double));
    std::vector<uint8_t> nv(n);
    std::vector<uint32_t> a(n), b(n);
    d2h(e, nv.data(), env->st.nv_pos, n);
    d2h(e, a.data(), env->st.steps_remaining, n * sizeof(uint32_t));
    d2h(e, b.data(), env->st.reset_count, n * sizeof(uint32_t));
    for (size_t i = 0; i < n; ++i) {
      nv_pos[i] = nv[i];
      steps_remaining[i] = a[i];
      reset_count[i] = b[i];
    }
  });
}

int32_t rl_env_set_state(rl_env *env, const double *state4, const int32_t *nv_pos, const uint64_t *steps_remaining,
                         const uint64_t *reset_count) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(env && state4 && nv_pos && steps_remaining && reset_count, "NULL argument");
    if (env->kind == RL_ENV_META_BANDIT)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_env_set_state is not built for RL_ENV_META_BANDIT lanes");
    if (env->kind == RL_ENV_META_MDP)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_env_set_state is not built for RL_ENV_META_MDP lanes");
    if (env->kind == RL_ENV_PARTITION)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_env_set_state is not built for RL_ENV_PARTITION lanes");
    rl_engine *e = env->eng;
    size_t n = env->cfg.n_lanes;
    if (env->kind == RL_ENV_TABULAR_MDP)  // the lane's state indexes the tables; its stream position is an even word
      for (size_t i = 0; i < n; ++i) {
        const double st = state4[i], pos = state4[2 * n + i];
        RL_REQUIRE(st >= 0.0 && st < (double)env->dev.mdp.states && st == std::floor(st),
                   "rl_env_set_state: tabular-MDP lanes: state index outside 0 .. n_states - 1");
        RL_REQUIRE(pos >= 0.0 && pos < 9007199254740992.0 && pos == 2.0 * std::floor(pos / 2.0),
                   "rl_env_set_state: tabular-MDP lanes: env-stream position must be an even word below 2^53");
      }
    std::vector<uint8_t> nv(n);
    std::vector<uint32_t> a(n), b(n);
    for (size_t i = 0; i < n; ++i) {
      nv[i] = nv_pos[i] ? 1 : 0;
      RL_REQUIRE(steps_remaining[i] < (1ull << 32) && reset_count[i] < (1ull << 32), "state value out of range");
      a[i] = (uint32_t)steps_remaining[i];
      b[i] = (uint32_t)reset_count[i];
    }
    h2d(e, env->st.x, state4 + 0 * n, n * sizeof(double));
    h2d(e, env->st.xdot, state4 + 1 * n, n * sizeof(double));
    h2d(e, env->st.th, state4 + 2 * n, n * sizeof(double));
    h2d(e, env->st.thdot, state4 + 3 * n, n * sizeof(double));
    h2d(e, env->st.nv_pos, nv.data(), n);
    h2d(e, env->st.steps_remaining, a.data(), n * sizeof(uint32_t));
    h2d(e, env->st.reset_count, b.data(), n * sizeof(uint32_t));
  });
}

}  // extern "C"
