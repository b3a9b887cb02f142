// abi_summary.hip — the step summaries of the C ABI (include/relearn_hip.h, rl_summary_*): OnlineStepsSummary per lane
// and the completed StepsSummary on the device (src/simulation/summary.rs:11-18,198-214), kernels in
// kernels_summary.hip; rl_steps_summary_merge on the host.
#include "abi_internal.hpp"
#include "summary.hpp"

extern "C" {

// OnlineStepsSummary::default per lane (summary.rs:186-194)
int32_t rl_summary_create(rl_engine *e, uint64_t n_lanes, rl_summary **out) {
  return guarded(e, [&] {
    RL_REQUIRE(e && out, "NULL argument");
    *out = nullptr;
    RL_REQUIRE(n_lanes > 0 && n_lanes < (1ull << 31), "bad lane count");
    RL_HIP_CHECK(hipSetDevice(e->device));
    std::unique_ptr<rl_summary> s(new rl_summary());
    s->eng = e;
    s->n = n_lanes;
    s->max_groups = ((n_lanes + 3) / 4 + 3) / 4;  // workgroups cover at least 4 lane quads (kernels_summary.hip)
    s->carry_len = s->mem.alloc<uint64_t>(n_lanes);
    s->carry_ret = s->mem.alloc<double>(n_lanes);
    s->acc = s->mem.alloc<rl_steps_summary>(1);
    s->part = s->mem.alloc<rl_steps_summary>(s->max_groups);
    RL_HIP_CHECK(hipMemsetAsync(s->carry_len, 0, n_lanes * sizeof(uint64_t), e->stream));
    RL_HIP_CHECK(hipMemsetAsync(s->carry_ret, 0, n_lanes * sizeof(double), e->stream));
    RL_HIP_CHECK(hipMemsetAsync(s->acc, 0, sizeof(rl_steps_summary), e->stream));
    sync(e);
    e->live_handles += 1;
    *out = s.release();
  });
}

int32_t rl_summary_destroy(rl_summary *s) { return destroy_child(s); }

// OnlineStepsSummary::push (summary.rs:198-214) over the trajectory's steps.  `settle` false: the two planes it reads
// are written by rollouts (main stream) and rl_traj_write only, never by an update chain, so it need not wait for a
// critic chain in flight (rl_actor_critic_update_begin).
int32_t rl_summary_push(rl_summary *s, const rl_traj *t) {
  return guarded(
      s ? s->eng : nullptr,
      [&] {
        RL_REQUIRE(s && t, "NULL argument");
        RL_REQUIRE(t->eng == s->eng, "trajectory of another engine");
        RL_REQUIRE(t->d.n == s->n, "lane count of the trajectory does not match the summary");
        launch_summary_planes(s, t->d.reward, t->d.flag, t->d.T);
      },
      /*settle=*/false);
}

int32_t rl_summary_push_dqn(rl_summary *s, const rl_dqn *q) {
  return guarded(
      s ? s->eng : nullptr,
      [&] {
        RL_REQUIRE(s && q, "NULL argument");
        RL_REQUIRE(q->eng == s->eng, "DQN agent of another engine");
        RL_REQUIRE(q->rp.N == s->n, "lane count of the DQN agent does not match the summary");
        RL_REQUIRE(q->last_horizon > 0, "no collection to summarise (rl_dqn_collect first)");
        RL_REQUIRE(q->last_horizon <= q->rp.C, "the last collection outgrew the replay ring: its early rewards are gone");
        launch_summary_replay(s, q->rp.rec, q->rp.total, q->rp.C, q->d_flags, (uint32_t)q->last_horizon);
      },
      /*settle=*/false);
}

int32_t rl_summary_read(rl_summary *s, rl_steps_summary *out) {
  return guarded(
      s ? s->eng : nullptr,
      [&] {
        RL_REQUIRE(s && out, "NULL argument");
        d2h(s->eng, out, s->acc, sizeof(rl_steps_summary));
      },
      /*settle=*/false);
}

int32_t rl_summary_clear(rl_summary *s, int32_t forget_episodes_in_progress) {
  return guarded(
      s ? s->eng : nullptr,
      [&] {
        RL_REQUIRE(s, "NULL argument");
        hipStream_t st = s->eng->stream;
        RL_HIP_CHECK(hipMemsetAsync(s->acc, 0, sizeof(rl_steps_summary), st));
        if (forget_episodes_in_progress) {
          RL_HIP_CHECK(hipMemsetAsync(s->carry_len, 0, s->n * sizeof(uint64_t), st));
          RL_HIP_CHECK(hipMemsetAsync(s->carry_ret, 0, s->n * sizeof(double), st));
        }
      },
      /*settle=*/false);
}

// impl Add for StepsSummary (stats.rs:184-209 per statistic), empty sides returned unchanged
int32_t rl_steps_summary_merge(const rl_steps_summary *a, const rl_steps_summary *b, rl_steps_summary *out) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(a && b && out, "NULL argument");
    *out = ss_merge(*a, *b);
  });
}

}  // extern "C"
