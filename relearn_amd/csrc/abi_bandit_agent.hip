// abi_bandit_agent.hip — the bandit baselines of the C ABI (include/relearn_hip.h, rl_bandit_agent_*): the classical
// agents of relearn_experiments/src/bin/rl2-bandits.rs `eval` (:166-261) run over RL_ENV_META_BANDIT lanes; the kernel
// is in kernels_bandit_agent.hip.
#include "abi_internal.hpp"
#include "bandit_agent.hpp"

namespace {
bool known_kind(int32_t kind) {  // (3 is unassigned)
  return kind == RL_BANDIT_AGENT_RANDOM || kind == RL_BANDIT_AGENT_TABULAR_Q || kind == RL_BANDIT_AGENT_UCB1 ||
         kind == RL_BANDIT_AGENT_THOMPSON;
}
}  // namespace

extern "C" {

// TabularQLearningAgentConfig::default (tabular.rs:43-51), UCB1AgentConfig::default (ucb.rs:36-42),
// BetaThompsonSamplingAgentConfig::default (thompson_sampling.rs: num_samples 1, carried by initial_action_count)
int32_t rl_bandit_agent_config_default(int32_t kind, rl_bandit_agent_config *cfg) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(cfg, "config is NULL");
    RL_REQUIRE(known_kind(kind), "rl_bandit_agent_config_default: unknown kind");
    cfg->kind = kind;
    cfg->reserved = 0;
    cfg->exploration_rate = kind == RL_BANDIT_AGENT_TABULAR_Q || kind == RL_BANDIT_AGENT_UCB1 ? 0.2 : 0.0;
    cfg->initial_action_count = kind == RL_BANDIT_AGENT_THOMPSON ? 1 : 0;
    cfg->initial_action_value = 0.0;
  });
}

int32_t rl_bandit_agent_create(rl_env *env, const rl_bandit_agent_config *cfg, rl_bandit_agent **out) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(env && cfg && out, "NULL argument");
    *out = nullptr;
    if (env->kind != RL_ENV_META_BANDIT)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_bandit_agent_create is built for RL_ENV_META_BANDIT lanes");
    const int32_t kind = cfg->kind;
    RL_REQUIRE(known_kind(kind), "rl_bandit_agent_create: unknown kind");
    RL_REQUIRE(cfg->reserved == 0, "rl_bandit_agent_create: reserved must be 0");
    const bool thompson = kind == RL_BANDIT_AGENT_THOMPSON;
    if (thompson) {  // initial_action_count carries num_samples
      RL_REQUIRE(cfg->initial_action_count != 0,
                 "rl_bandit_agent_create: num_samples (initial_action_count of a THOMPSON agent) must not be 0");
      if (cfg->initial_action_count > RL_BANDIT_NUM_SAMPLES_MAX)
        throw RlError(RL_ERR_UNSUPPORTED, "rl_bandit_agent_create: num_samples (initial_action_count of a THOMPSON "
                                          "agent) is at most 1024: every pull draws k * num_samples Beta samples "
                                          "within the one launch");
    }
    if (kind == RL_BANDIT_AGENT_TABULAR_Q || kind == RL_BANDIT_AGENT_UCB1) {
      RL_REQUIRE(std::isfinite(cfg->exploration_rate) && cfg->exploration_rate >= 0.0,
                 "rl_bandit_agent_create: exploration_rate must be finite and not negative");
      RL_REQUIRE(kind != RL_BANDIT_AGENT_TABULAR_Q || cfg->exploration_rate <= 1.0,
                 "rl_bandit_agent_create: exploration_rate of a TABULAR_Q agent must not exceed 1");
    }
    if (kind == RL_BANDIT_AGENT_TABULAR_Q)
      RL_REQUIRE(std::isfinite(cfg->initial_action_value) && cfg->initial_action_value >= 0.0,
                 "rl_bandit_agent_create: initial_action_value must be finite and not negative");
    rl_engine *e = env->eng;
    const uint64_t n = env->cfg.n_lanes, E = env->dev.max_steps;
    const uint32_t k = env->dev.meta_arms;
    if (kind == RL_BANDIT_AGENT_UCB1 && E > RL_BANDIT_LN_TABLE_MAX)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_bandit_agent_create: a UCB1 agent takes at most 1048576 episodes per trial "
                                        "(its table of 2 ln(visit) has one entry per pull of a trial)");
    RL_HIP_CHECK(hipSetDevice(e->device));
    std::unique_ptr<rl_bandit_agent> a(new rl_bandit_agent());
    a->eng = e;
    a->cfg = *cfg;
    a->n = n;
    a->k = k;
    a->E = E;
    BanditAgentDev &d = a->d;
    d.rate = cfg->exploration_rate;
    d.init_value = cfg->initial_action_value;
    d.init_count = cfg->initial_action_count;
    uint64_t *pos = a->mem.alloc<uint64_t>(n);
    d.pos = pos;
    RL_HIP_CHECK(hipMemsetAsync(pos, 0, n * sizeof(uint64_t), e->stream));
    if (thompson) {  // BetaThompsonSamplingAgent::new: one low and one high reward per arm
      d.num_samples = (uint32_t)cfg->initial_action_count;
      uint64_t *low = a->mem.alloc<uint64_t>(k * n), *high = a->mem.alloc<uint64_t>(k * n);
      d.low = low;
      d.high = high;
      const std::vector<uint64_t> ones(k * n, 1);
      h2d(e, low, ones.data(), k * n * sizeof(uint64_t));
      h2d(e, high, ones.data(), k * n * sizeof(uint64_t));
    } else if (kind != RL_BANDIT_AGENT_RANDOM) {  // a fresh inner agent per lane (the kernel makes one again at every trial's start)
      const bool ucb = kind == RL_BANDIT_AGENT_UCB1;
      d.count = a->mem.alloc<uint64_t>(k * n);
      d.value = a->mem.alloc<double>(k * n);
      const std::vector<uint64_t> count(k * n, ucb ? 2 : cfg->initial_action_count);
      const std::vector<double> value(k * n, ucb ? 0.5 : cfg->initial_action_value);
      h2d(e, d.count, count.data(), k * n * sizeof(uint64_t));
      h2d(e, d.value, value.data(), k * n * sizeof(double));
      if (ucb) {
        d.visit = a->mem.alloc<uint64_t>(n);
        const std::vector<uint64_t> visit(n, 2ull * k);
        h2d(e, d.visit, visit.data(), n * sizeof(uint64_t));
        // ln is taken of integers only: 2.0 * (visit as f64).ln() (ucb.rs:217-218) for every visit count a trial reaches
        std::vector<double> ln2(E);
        for (uint64_t j = 0; j < E; ++j) ln2[j] = 2.0 * std::log((double)(2ull * k + j));
        double *table = a->mem.alloc<double>(E);
        h2d(e, table, ln2.data(), E * sizeof(double));
        d.ln2 = table;
      }
    }
    sync(e);
    e->live_handles += 1;
    *out = a.release();
  });
}

int32_t rl_bandit_agent_destroy(rl_bandit_agent *agent) { return destroy_child(agent); }

// `settle` false, as rl_rollout: a critic chain in flight reads its own trajectory
int32_t rl_bandit_agent_rollout(rl_bandit_agent *agent, rl_env *env, rl_traj *traj) {
  return guarded(env ? env->eng : nullptr, [&] {
    RL_REQUIRE(agent && env && traj, "NULL argument");
    RL_REQUIRE(env->eng == traj->eng && env->eng == agent->eng, "handles belong to different engines");
    if (traj == env->eng->pending.traj) engine_settle(env->eng);
    if (env->kind != RL_ENV_META_BANDIT)
      throw RlError(RL_ERR_UNSUPPORTED, "rl_bandit_agent_rollout is built for RL_ENV_META_BANDIT lanes");
    RL_REQUIRE(env->cfg.n_lanes == agent->n && env->dev.meta_arms == agent->k && env->dev.max_steps == agent->E,
               "rl_bandit_agent_rollout: the env has other lanes, arms or episodes per trial than the agent was made on");
    traj->range_valid = traj->range_reset = false;  // new observations: the range guard has them measured again
    traj->rtg_scan_valid = false;                   // new rewards: the return plane belongs to the old ones
    RL_REQUIRE(traj->d.n == env->cfg.n_lanes && traj->d.D == env->D, "trajectory shape does not match the env");
    traj->n_actions = env->A;
    launch_bandit_agent_rollout(agent, env, traj);  // (advances t_global)
  }, false);
}

int32_t rl_bandit_agent_state_read(rl_bandit_agent *agent, int32_t field, void *host, uint64_t bytes) {
  return guarded(agent ? agent->eng : nullptr, [&] {
    RL_REQUIRE(agent && host, "NULL argument");
    const BanditAgentDev &d = agent->d;
    const void *src = nullptr;
    uint64_t want = 0;
    switch (field) {
      case RL_BANDIT_STATE_ACTOR_POS: src = d.pos, want = agent->n * sizeof(uint64_t); break;
      case RL_BANDIT_STATE_COUNTS: src = d.count, want = agent->k * agent->n * sizeof(uint64_t); break;
      case RL_BANDIT_STATE_VALUES: src = d.value, want = agent->k * agent->n * sizeof(double); break;
      case RL_BANDIT_STATE_VISITS: src = d.visit, want = agent->n * sizeof(uint64_t); break;
      case RL_BANDIT_STATE_LN_TABLE: src = d.ln2, want = agent->E * sizeof(double); break;
      case RL_BANDIT_STATE_LOW_COUNTS: src = d.low, want = agent->k * agent->n * sizeof(uint64_t); break;
      case RL_BANDIT_STATE_HIGH_COUNTS: src = d.high, want = agent->k * agent->n * sizeof(uint64_t); break;
      default: throw RlError(RL_ERR_INVALID_ARGUMENT, "rl_bandit_agent_state_read: unknown field");
    }
    RL_REQUIRE(src != nullptr, "rl_bandit_agent_state_read: an agent of this kind has no such field");
    RL_REQUIRE(bytes == want, "rl_bandit_agent_state_read: wrong byte count for this field");
    d2h(agent->eng, host, src, want);
  });
}

}  // extern "C"
