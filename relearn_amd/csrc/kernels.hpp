// kernels.hpp — host launchers implemented in the .hip translation units.
#pragma once
#include <cstdlib>
#include <functional>
// arrays of [128 units][32 lanes] floats per (step, tile) block in the recurrent training workspace (kernels_seq.hip)
#define RL_SEQ_ACT_ARRAYS 9
#define RL_SEQ_DPRE_ARRAYS 6
#include "engine.hpp"

// kernels_rollout.hip
void launch_env_reset(rl_env *env);  // the standalone env kernels: every env kind
void launch_env_observe(rl_env *env, float *d_obs);
void launch_env_step(rl_env *env);
void launch_rollout(rl_env *env, const rl_mlp *policy, rl_traj *traj);  // feed-forward policy on CartPole lanes
void launch_values(rl_traj *traj, const rl_mlp *critic);
void launch_gae(rl_traj *traj, const rl_mlp *critic, float gamma, float lambda);  // critic NULL: adv = rtg only
// critic regression targets into traj->d.tgt: one-step TD from traj->d.values (critic != NULL) or reward-to-go (NULL)
void launch_value_targets(rl_traj *traj, const rl_mlp *critic, float gamma);
void launch_mlp_forward_host_rows(rl_mlp *mlp, const float *d_in_soa, size_t rows, float *d_out_soa);
// magnitude range of the trajectory's observation planes -> traj->d.range[0..1] (the fused kernels' range guard)
void launch_obs_range(rl_traj *traj);
// ... once per content of the planes: whoever rewrites them (rollouts, rl_traj_write) clears `range_valid`
inline void traj_ensure_range(rl_traj *traj) {
  if (traj->range_valid || traj->range_fixed) return;
  launch_obs_range(traj);
  traj->range_valid = true;
}
// Do the fused 5-128 kernels (kernels_mfma.hip, kernels_critic.hip, kernels_dqn.hip) take module `m` on the planes of
// `t`?  A feed-forward module with one hidden layer of 128 units and `out_dim` outputs over five observation features,
// and planes the kernels' 32-bit element offsets reach.  The one statement of it: the launchers decline by it, and the
// host decisions that have to agree with them (may two chains overlap, is a DQN update snapshotted, are TD targets
// formed in the kernel) are taken by it.  `offsets` false leaves the last term out, for a decision taken before the
// sample count is known.  (rl_engine::kernel_variant is not part of it: that is the caller's question, asked where
// a fused launcher of either family — these kernels or gen_mfma_fits' — is about to be tried.)
inline bool fused_5_128_fits(const rl_traj *t, const rl_mlp *m, uint32_t out_dim, bool offsets = true) {
  return m->kind == RL_MODULE_MLP && !m->general && t->d.D == 5 && m->hidden == 128 && m->out_dim == out_dim &&
         (!offsets || (uint64_t)(t->d.T + 1) * t->d.n * 5 < (1ull << 30));
}
// rl_rollout's path for this env and policy, or the refusal of the pair (handle_spec.hpp has the table)
inline RolloutPath rollout_path(const rl_env *env, const rl_mlp *policy) {
  return rollout_path(env->kind, env->D, env->A, env->dev.chain_size, *policy);
}
// The persistent grid of a fused 5-128 launch over the planes of `t`: one workgroup per `walkers` 32-sample tiles (its
// tile-walking waves), at most one per CU — fewer, fatter workgroups are fewer slab rows for the reduction that follows
// every launch.
inline uint32_t fused_grid(const rl_traj *t, uint32_t walkers) {
  const uint64_t n_tiles = (t->B + 31) / 32, cus = (uint64_t)t->eng->prop.multiProcessorCount;
  const uint64_t nb = (n_tiles + walkers - 1) / walkers;
  return (uint32_t)(nb > cus ? cus : nb);
}
// The planes a fused 5-128 launch runs on.  The numeric range guard belongs to the first launch of a chain in a call
// (engine.hpp): `guard_next` is the chain's flag (rl_traj::guard_next_policy / _critic), consumed here; every other launch
// gets no range words.
inline TrajDev fused_traj_dev(const rl_traj *t, bool &guard_next) {
  TrajDev d = t->d;
  if (!guard_next) d.range = nullptr;
  guard_next = false;
  return d;
}

// The weight image of a 5 -> 128 -> A module (bf16_tile.hpp): valid for one C-ABI call at a time.
//   wimg_ensure       a fused launcher about to read it: builds it (one small launch on the engine's current stream)
//                     unless this call already did, returns it
//   wimg_if_current   a launcher whose kernel writes the module's parameters one lane per parameter: the image to keep
//                     current beside them, or NULL when this call has not built one (nothing to keep)
//   wimg_invalidate   anything else that writes the parameters on the device inside a call
const uint32_t *wimg_ensure(const rl_mlp *m);
inline uint32_t *wimg_if_current(const rl_mlp *m) {
  return m->d_wimg != nullptr && m->wimg_epoch == m->eng->call_epoch ? m->d_wimg : nullptr;
}
inline void wimg_invalidate(const rl_mlp *m) { m->wimg_epoch = 0; }

// the output planes seq.out / seq.succ [2][T][n]: the recurrent paths and the general-MLP value pass share them
inline void seq_ensure_outputs(rl_traj *t) {
  const uint64_t B = (uint64_t)t->d.T * t->d.n;
  t->mem.ensure(t->seq.out, 2 * B);
  t->mem.ensure(t->seq.succ, 2 * B);
}

// kernels_update.hip
enum PolicyPassMode { PASS_INIT = 0, PASS_EVAL = 1, PASS_JVP = 2, PASS_DQN = 3, PASS_PPO = 4 };
// PASS_INIT : lp0 <- log pi(.|s); dz <- d(-mean(ratio*A))/dz at theta0; slabB <- {sum A, sum entropy}
// PASS_EVAL : slabB <- {sum ratio*A, sum KL(pi0||pi)}                      (skipped when *skip_flag != 0)
// PASS_JVP  : dz <- (diag(p) - p p^T) J v / B_total                         (skipped when *skip_flag != 0)
// PASS_PPO  : dz <- d(-mean(min(ratio A, clip(ratio, lo, hi) A)))/dz against lp0; slabB <- {sum min(..)}  (ppo.rs:124-137)
// PASS_DQN  : outputs are action values; dz[a] <- [a == action] 2 (Q_a - target) / B_total with the target in
//             `adv`; slabB <- {sum (Q_a - target)^2}                        (dqn.rs:316-326)
void launch_policy_pass(rl_traj *traj, const rl_mlp *policy, int mode, const float *d_tangent, uint64_t B_total,
                        const int32_t *d_skip_flag, float clip_lo = 0.0f, float clip_hi = 0.0f);
void launch_critic_fwd(rl_traj *traj, const rl_mlp *critic, uint64_t B_total);
// J^T dz accumulated per block into slabA (lane = hidden unit, samples broadcast through scalar loads)
void launch_mlp_backward(rl_traj *traj, const rl_mlp *mlp, const int32_t *d_skip_flag);
// vec[0..P) <- sum_blocks slabA (if useA), vec[P..P+4) <- sum_blocks slabB; deterministic order
void launch_reduce(rl_traj *traj, uint32_t P, bool useA, bool useB, uint32_t rowsA, uint32_t rowsB);

void launch_trpo_begin(rl_traj *traj, rl_mlp *policy, uint64_t B_total);                 // after grad reduce
void launch_cg_step(rl_traj *traj, uint32_t P, float reg, float tol);                    // after HVP reduce
void launch_cg_finish(rl_traj *traj, uint32_t P);                                        // nan_to_num, tangent <- x
void launch_step_size(rl_traj *traj, rl_mlp *policy, float reg, double max_kl);          // after HVP(x) reduce
void launch_ls_set_params(rl_traj *traj, rl_mlp *policy, double ratio);
void launch_ls_check(rl_traj *traj, uint32_t P, uint64_t B_total, int index, double ratio, double max_kl);
void launch_ls_finalize(rl_traj *traj, rl_mlp *policy, double max_kl, int accept_violation);
void launch_opt_step(rl_traj *traj, rl_adam *opt, int loss_slot, uint64_t B_total);      // after critic reduce
void launch_opt_step_vec(rl_adam *opt, const float *d_grad);
// reduce(A + B) and the optimiser's step in one launch (single-rank runs: no all-reduce between the two)
void launch_reduce_opt(rl_traj *traj, rl_adam *opt, uint32_t rowsA, uint32_t rowsB, int loss_slot, uint64_t B_total);

// kernels_critic.hip, kernels_mfma.hip ("v2"): the fused critic step and policy passes of a 5-128 module on the bf16
// matrix pipe (bf16_tile.hpp); a module with several hidden layers goes on to launch_gen_mfma
// return false when the shape is not built (the caller has the v1 kernels)
bool launch_critic_step_v2(rl_traj *traj, const rl_mlp *critic, uint64_t B_total);
// `keep` (PASS_INIT of a 5-128-2 module): the gradient pass also leaves its relu' masks and Fisher weights in the
// trajectory's kept planes for the PASS_JVP launches of the same call, which read them and refuse to run without
// (rl_traj::kept_epoch); every other kernel family ignores it
bool launch_policy_v2(rl_traj *traj, const rl_mlp *policy, int mode, const float *d_tangent, uint64_t B_total,
                      const int32_t *d_skip_flag, float clip_lo = 0.0f, float clip_hi = 0.0f, bool keep = false);

// kernels_dqn.hip
// d_range (may be NULL): the collected observations' magnitude range is folded there (the fused gradient's range guard)
void launch_rollout_dqn(rl_env *env, const rl_mlp *qnet, const ReplayDev &rp, uint32_t T, uint64_t p_int,
                        int always_explore, uint8_t *d_flags, uint32_t *d_range = nullptr);
// an action-value module of any shape (rl_mlp::general): one launch sequence per step; `ws` lends the layer kernels their
// workspace, d_q [n_actions][n] receives the module's outputs of every step (n_actions: the env's, 2..8)
void launch_rollout_dqn_general(rl_env *env, const rl_mlp *qnet, rl_traj *ws, float *d_q, const ReplayDev &rp, uint32_t T,
                                uint64_t p_int, int always_explore, uint8_t *d_flags);
// d_target += gamma * amax over the n_actions planes of d_q_next [n_actions][n], 0 beyond a Terminate
void launch_dqn_td_targets(rl_engine *eng, float *d_target, const uint8_t *d_flag, const float *d_q_next, uint32_t n,
                           uint32_t n_actions, float gamma);
struct AgentKey { uint32_t w[8]; };
// `ep` (EpisodeLists, engine.hpp): the episode lists of one minibatch; the two launchers that take `n_batches` of them
// take the first one's and find minibatch b at b * max_eps
void launch_dqn_sample(rl_engine *eng, hipStream_t stream, const ReplayDev &rp, const AgentKey &key, uint64_t *d_agent_pos,
                       uint32_t minibatch_steps, uint32_t max_eps, const EpisodeLists &ep, DqnCountsDev *d_counts,
                       int sequential, uint32_t n_batches = 1);
// gather + reward-to-go targets of `n_batches` minibatches; d_flag != NULL: rewards, successor codes and successor
// observations (time slot 1) instead, for one-step TD targets formed later
void launch_dqn_build_all(rl_engine *eng, const ReplayDev &rp, uint32_t n_batches, uint32_t widest_eps, uint32_t max_eps,
                          const EpisodeLists &ep, const DqnCountsDev *d_counts, float *d_obs, size_t obs_stride,
                          uint8_t *d_action, float *d_target, size_t step_stride, float gamma, uint8_t *d_flag);
void launch_replay_planes(rl_engine *eng, const ReplayDev &rp, int field, void *d_out);
// the DQN gradient with the one-step TD targets formed in the launch (the workspace holds rewards)
bool launch_dqn_step_bf16(rl_traj *mb, const rl_mlp *qnet, uint64_t B_total, float gamma);
// kernels_critic.hip: the same gradient with the targets given, as two critic-step channels per SIMD
bool launch_dqn_step_pair(rl_traj *mb, const rl_mlp *qnet, uint64_t B_total);
// one minibatch's gather and targets: reward-to-go, or one-step TD from the fused module's forward inside the launch
void launch_dqn_build_minibatch(rl_engine *eng, const ReplayDev &rp, uint32_t n_eps, const EpisodeLists &ep, float *d_obs,
                                size_t out_plane, uint8_t *d_action, float *d_target, float gamma, int one_step_td,
                                const rl_mlp *qnet);
// recurrent action-value modules (rl_dqn_create_recurrent): the sampled episodes of one minibatch as the lane columns of
// a trajectory-shaped workspace `seq` (n = episodes, T = the longest one; kernels_dqn.hip has the layout)
// the longest episode of each minibatch of a draw -> d_counts[b].pad
void launch_dqn_longest(rl_engine *eng, const EpisodeLists &ep, uint32_t max_eps, DqnCountsDev *d_counts, uint32_t n_batches);
// ring -> workspace planes; targets from `d_given` (episode-after-episode order), or NULL: the rewards
void launch_dqn_build_seq(rl_traj *seq, const ReplayDev &rp, const EpisodeLists &ep, const float *d_given);
// one-step TD targets from seq.out / seq.succ -> the workspace's targets and `d_compact` (episode-after-episode order)
void launch_dqn_seq_td_targets(rl_traj *seq, const EpisodeLists &ep, uint32_t n_actions, float gamma, float *d_compact);
// seq.out, targets -> dz (zero on padding) and the loss sum in slab B
void launch_dqn_seq_terms(rl_traj *seq, const EpisodeLists &ep, uint32_t n_actions, uint64_t B_total);
// kernels_seq_stack.hip: all `T` collection steps of a recurrent action-value module in one launch; `roll` lends the
// per-lane states and the observation planes ([D][2][N])
void launch_stack_collect_dqn(rl_env *env, const rl_mlp *qnet, rl_traj *roll, const ReplayDev &rp, uint32_t T,
                              uint64_t p_int, int always_explore, uint8_t *d_flags);

// kernels_seq.hip (recurrent configuration: GRU -> ReLU -> MLP module; tiles of 32 lanes)
void launch_rollout_gru(rl_env *env, const rl_mlp *policy, rl_traj *traj);        // recurrent policy, either env kind
void launch_rollout_chain_mlp(rl_env *env, const rl_mlp *policy, rl_traj *traj);  // feed-forward policy on Chain lanes
// teacher-forced forward: d_out [A][T][n]; d_succ (may be NULL) [A][T][n]; d_act (may be NULL) activation record
void launch_gru_seq_forward(rl_traj *traj, const rl_mlp *mod, float *d_out, float *d_succ, float *d_act,
                            const int32_t *d_skip = nullptr);
// kernels_general.hip: MLPs of any hidden_sizes (per-layer kernels; rl_mlp::general)
void gen_ensure(rl_traj *t, const rl_mlp *m, uint64_t rows, bool tangent, bool backward);
void launch_gen_forward(rl_traj *t, const rl_mlp *m, const float *x, size_t x_stride, uint64_t rows, float *out);
void launch_gen_policy_pass(rl_traj *t, const rl_mlp *m, int mode, const float *d_tangent, uint64_t B_total,
                            const int32_t *d_skip, float clip_lo, float clip_hi);
void launch_gen_critic_fwd(rl_traj *t, const rl_mlp *m, uint64_t B_total);
void launch_gen_backward(rl_traj *t, const rl_mlp *m, const int32_t *d_skip);
void traj_ensure_slabs(rl_traj *t, uint64_t rowsA, uint64_t P, uint64_t rowsB);
void traj_ensure_action_planes(rl_traj *t, uint32_t n_actions);  // lp0, dz: [n_actions][B]
// kernels_gen_mfma.hip: the passes of a several-hidden-layer MLP as one fused matrix-pipe launch (false: shape not built)
constexpr int RL_GEN_CRITIC = 100;  // mode: mean((V - target)^2); else PASS_INIT / PASS_PPO / PASS_EVAL / PASS_JVP
bool gen_mfma_fits(const rl_traj *t, const rl_mlp *m);
bool launch_gen_mfma(rl_traj *t, const rl_mlp *m, int mode, const float *d_tangent, uint64_t B_total,
                     const int32_t *d_skip, float clip_lo, float clip_hi);
const float *launch_gen_values(rl_traj *t, const rl_mlp *critic);  // -> seq.out / seq.succ (plane 0); returns V(obs[T]) [n]
void launch_gen_rollout(rl_env *env, const rl_mlp *policy, rl_traj *t);
void launch_rollout_stepwise(rl_env *env, rl_traj *t, const float *z, const std::function<void(uint32_t)> &forward);
void launch_gen_wgrad_planes(rl_traj *t, const float *dY, size_t dys, int N, const float *X, size_t xs, int K, size_t S,
                             uint32_t chunk, uint32_t rows, uint32_t P, uint32_t offW, uint32_t offB,
                             const int32_t *d_skip);
// kernels_seq_stack.hip: recurrent chains with RnnBaseConfig::num_layers > 1 (one thread per lane, the unit loop of a
// layer dealt to a workgroup's waves; no lane-tile or width restriction)
void stack_ensure(rl_traj *t, const rl_mlp *mod, bool training);
void launch_stack_rollout(rl_env *env, const rl_mlp *policy, rl_traj *traj);
void launch_stack_forward(rl_traj *traj, const rl_mlp *mod, float *d_out, float *d_succ, bool record,
                          const int32_t *d_skip);
void launch_stack_backward(rl_traj *traj, const rl_mlp *mod, const int32_t *d_skip);  // dz, record -> vec[0..P)
void launch_stack_tangent(rl_traj *traj, const rl_mlp *mod, const float *d_tangent, const int32_t *d_skip);  // -> seq.out
// a recurrent chain of other widths embedded in the kernels' shape (rl_mlp::exec): copy the flat vector `real_src`
// (layout of `real`) into the padded layout `exec_dst` / gather the padded vector `exec_src` into the flat layout
void launch_seq_pad(const rl_mlp *real, float *exec_dst, const float *real_src);
void launch_seq_unpad(const rl_mlp *real, const float *exec_src, float *real_dst);
// kernels_seq_train.hip: the GRU chain's training passes with the recurrence on the bf16 matrix pipe
void launch_gru_train_forward(rl_traj *traj, const rl_mlp *mod, float *d_out, float *d_act, const int32_t *d_skip);
void launch_lstm_train_forward(rl_traj *traj, const rl_mlp *mod, float *d_out, float *d_act, const int32_t *d_skip);
void launch_seq_train_head_forward(rl_traj *traj, const rl_mlp *mod, float *d_out, float *d_act, const int32_t *d_skip);
void launch_gru_train_head_backward(rl_traj *traj, const rl_mlp *mod, float *d_slab, const int32_t *d_skip);
void launch_gru_train_recur_backward(rl_traj *traj, const rl_mlp *mod, const int32_t *d_skip);
void launch_gru_train_wgrad(rl_traj *traj, const rl_mlp *mod, const int32_t *d_skip);
constexpr uint32_t RL_SEQ_HEAD_ROWS = 512;  // rows of head-gradient partials behind the weight-gradient kernel's chunks
// v_last: [n] V(obs[T]) of every lane for slot T of the value plane (a general critic's: launch_gen_values), or NULL
void launch_seq_gae(rl_traj *traj, float gamma, float lambda, const float *v_last);
// one-step TD targets from traj->seq.out / succ (plane 0) -> d.tgt
void launch_seq_value_targets(rl_traj *traj, float gamma, const float *v_last);
void launch_seq_policy_dlogits(rl_traj *traj, int mode, uint64_t B_total, float clip_lo, float clip_hi,
                               const int32_t *d_skip = nullptr, uint32_t n_out = 2);  // n_out: logit planes (2..8)
void launch_seq_critic_dvalues(rl_traj *traj, uint64_t B_total);
void launch_gru_backward(rl_traj *traj, const rl_mlp *mod, const int32_t *d_skip = nullptr);  // dz, seq.act -> vec[0..P)
// Fisher-vector product pieces: static tangent terms (dpre, seq.succ) from the tangent parameters, then the recurrent
// tangent pass -> seq.out = d logits . tangent, then dz <- (diag(p) - p p^T) (.) / B
void launch_gru_tangent(rl_traj *traj, const rl_mlp *mod, const float *d_tangent, uint64_t B_total,
                        const int32_t *d_skip);
